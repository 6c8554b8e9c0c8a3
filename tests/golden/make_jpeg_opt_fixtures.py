"""Writes tests/golden/pillow_opt_*.jpg: the three pictures of
make_jpeg_fixtures.py saved with optimize=True, so each file carries Huffman
tables of its own in DHT instead of the Annex K.3 ones (still SOF0, one
interleaved scan).  Each stays below 2 KiB.  Run once, by hand:

    python tests/golden/make_jpeg_opt_fixtures.py
"""
import io
import os

from PIL import Image

from make_jpeg_fixtures import FIXTURES, HERE, picture


def main():
    for name, (h, w, ch, opts) in FIXTURES.items():
        buf = io.BytesIO()
        Image.fromarray(picture(h, w, ch)).save(buf, "JPEG", optimize=True, **opts)
        data = buf.getvalue()
        assert len(data) < 2048, (name, len(data))
        out = name.replace("pillow_", "pillow_opt_")
        with open(os.path.join(HERE, out), "wb") as f:
            f.write(data)
        print(out, len(data), "bytes")


if __name__ == "__main__":
    main()
