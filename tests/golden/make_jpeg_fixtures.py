"""Writes tests/golden/pillow_*.jpg, the three files of another writer that the
entropy decoder's tests read (Pillow / libjpeg-turbo, optimize=False: the Annex
K.3 Huffman tables).  Each stays below 2 KiB.  Run once, by hand:

    python tests/golden/make_jpeg_fixtures.py

The pictures are synthetic: two gradients, a ripple and a few hard edges, so the
scans hold DC steps, short and long zero runs and some larger coefficients.
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def picture(h, w, channels):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(channels):
        p = 40 + 150 * xx / w + 50 * yy / h * (1 if c != 1 else -1) + 25 * np.sin(xx / (3.0 + c) + yy / 5.0)
        p[h // 3:h // 2, w // 4:w // 2] += 60 - 40 * c
        p[(yy.astype(int) // 4 + xx.astype(int) // 4) % 7 == 0] -= 20
        planes.append(p)
    a = np.clip(np.rint(np.stack(planes, -1)), 0, 255).astype(np.uint8)
    return a[..., 0] if channels == 1 else a


FIXTURES = {
    # name: (height, width, channels, save options)
    "pillow_grey_rows.jpg": (43, 61, 1, dict(quality=60, restart_marker_rows=1)),
    "pillow_420_blocks3.jpg": (45, 70, 3, dict(quality=50, subsampling="4:2:0", restart_marker_blocks=3)),
    "pillow_444_norestart.jpg": (24, 40, 3, dict(quality=50, subsampling="4:4:4")),
}


def main():
    for name, (h, w, ch, opts) in FIXTURES.items():
        buf = io.BytesIO()
        Image.fromarray(picture(h, w, ch)).save(buf, "JPEG", optimize=False, **opts)
        data = buf.getvalue()
        assert len(data) < 2048, (name, len(data))
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
        print(name, len(data), "bytes")


if __name__ == "__main__":
    main()
