"""Baseline-JPEG entropy decoding, the CPU side (no GPU, no kernel runs):

- tests/jpeg_unscan.py, the plain-Python restatement of hpdct_decode_scan's rules
  that the GPU tests compare the kernels with: it inverts jpeg_scan.encode, and
  the corrupt corpus (tests/unscan_corpus.py) reaches every status code;
- hpdct_jpeg_parse: the inverse of hpdct_jpeg_header, three Pillow-written files
  (tests/golden/pillow_*.jpg) and every refusal;
- hpdct_decode_scan and hpdct_decode_workspace_bytes validate every argument
  before any device work (the pointers here are never dereferenced); the
  wrappers' own checks; the policy rows of the launches;
- a stand-alone program under ASan + UBSan: the refusals, the parser on every
  truncation and corruption of a file, and the walker the decode kernel wraps
  over the whole corpus.
"""
import ctypes
import io
import os

import numpy as np
import pytest

import host_programs
import jpeg_scan as J
import jpeg_unscan as U
import unscan_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
S444, S420 = 0, 1
FIXTURES = ["pillow_grey_rows.jpg", "pillow_420_blocks3.jpg", "pillow_444_norestart.jpg"]


def frame_blocks(sampling, seed):
    """Sparse random blocks in range for a small frame of each sampling: (components, shapes)."""
    shapes = {"grey": [(3, 7)], "444": [(2, 5)] * 3, "420": [(4, 6), (2, 3), (2, 3)]}[sampling]
    return [unscan_corpus.sparse_blocks(s, seed + i) for i, s in enumerate(shapes)], shapes


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ri", [0, 1, 2, 5])
@pytest.mark.parametrize("sampling", ["grey", "444", "420"])
def test_restatement_inverts_the_coder(sampling, ri):
    comps, shapes = frame_blocks(sampling, 11)
    data, offs = J.encode(comps, sampling, ri)
    for offsets in (None, offs):
        back, status, found, errors = U.decode(data, sampling, shapes, ri, offsets)
        assert all(np.array_equal(a, b) for a, b in zip(back, comps))
        assert not status.any() and len(status) == len(offs) - 1
        assert (found, errors) == ((len(offs) - 2, 0) if offsets is None else (0, 0))
    assert all(np.array_equal(a, b) for a, b in zip(J.decode(data, sampling, shapes, ri), comps))


def test_corpus_reaches_every_status():
    """A condition on the corpus, not on the code under test: every code 1..8 occurs, the clean scans are clean."""
    cases, results = unscan_corpus.cases_and_expected()
    seen = set()
    for _, status, _, _ in results:
        seen |= set((status & np.uint64(255)).tolist())
    assert seen == set(range(9)), sorted(seen)
    blocks, data, offs = unscan_corpus.base_grey()
    assert 1000 <= len(data) <= 1400
    for k in (0, 1):
        assert cases[k]["name"].startswith("clean") and not results[k][1].any()
        assert np.array_equal(results[k][0][0], blocks)
    assert results[0][2:] == (10, 0) and results[1][2:] == (0, 0)
    flips = [r for c, r in zip(cases, results) if c["name"].startswith("flip") and "offsets" not in c["name"]]
    assert len(flips) == 8 * len(data)
    # most flips still decode clean, to other blocks: the status alone does not tell a damaged scan
    clean_but_different = sum(1 for r in flips if not r[1].any() and not np.array_equal(r[0][0], blocks))
    assert clean_but_different > len(flips) // 4
    by_name = {c["name"]: r for c, r in zip(cases, results)}
    assert by_name["dc overflow"][1].tolist() == [U.DC + 256 * 16]
    assert by_name["no bytes"][1].tolist() == [U.END] + [U.MISSING] * 10
    assert set(by_name["offsets 2^63"][1].tolist()) == {U.RANGE}
    assert by_name["ff as last byte"][1][-1] in (U.END + 256 * 0, U.TAIL)
    assert by_name["marker 4 renumbered 3"][3] == 1 and not by_name["marker 4 renumbered 3"][1].any()
    assert by_name["marker 9 deleted"][1][-1] == U.MISSING


# ---------------------------------------------------------------------------
# hpdct_jpeg_parse
# ---------------------------------------------------------------------------
SCAN = b"\x12\x34\xff\x00\x56\xff\xd0\x78\xff\xd1\x9a"


@pytest.mark.parametrize("ri", [0, 1, 5, 65535])
@pytest.mark.parametrize("components,sub", [(1, "444"), (3, "444"), (3, "420")])
def test_parse_inverts_the_header(hp, components, sub, ri):
    ql = np.arange(1, 65, dtype=np.float32).reshape(8, 8)
    qc = np.arange(65, 129, dtype=np.float32).reshape(8, 8)
    head = hp.jpeg_header(45, 77, components=components, subsampling=sub, q_luma=ql, q_chroma=qc, restart_interval=ri)
    lay = hp.jpeg_parse(head + SCAN + b"\xff\xd9")
    assert (lay["height"], lay["width"], lay["components"], lay["restart_interval"]) == (45, 77, components, ri)
    assert lay["subsampling"] == (sub if components == 3 else "444")
    assert lay["scan_offset"] == len(head) and lay["scan_bytes"] == len(SCAN)
    assert np.array_equal(lay["q_luma"], ql)
    assert lay["q_chroma"] is None if components == 1 else np.array_equal(lay["q_chroma"], qc)
    # bytes after EOI are not read as part of the scan
    assert hp.jpeg_parse(head + SCAN + b"\xff\xd9junk")["scan_bytes"] == len(SCAN)


def fixture_layout(hp, name):
    data = open(os.path.join(GOLDEN, name), "rb").read()
    lay = hp.jpeg_parse(data)
    side = 16 if lay["subsampling"] == "420" else 8
    hpad, wpad = -(-lay["height"] // side) * side, -(-lay["width"] // side) * side
    sampling = "grey" if lay["components"] == 1 else lay["subsampling"]
    shapes = [(hpad // 8, wpad // 8)] + [(hpad // side, wpad // side)] * (lay["components"] - 1)
    scan = data[lay["scan_offset"]:lay["scan_offset"] + lay["scan_bytes"]]
    return data, lay, sampling, shapes, scan, (hpad, wpad)


@pytest.mark.parametrize("name", FIXTURES)
def test_parse_reads_pillow_files(hp, name):
    data, lay, sampling, shapes, scan, _ = fixture_layout(hp, name)
    assert len(data) < 2048
    want = {"pillow_grey_rows.jpg": (43, 61, 1, "444", 8), "pillow_420_blocks3.jpg": (45, 70, 3, "420", 3),
            "pillow_444_norestart.jpg": (24, 40, 3, "444", 0)}[name]
    assert (lay["height"], lay["width"], lay["components"], lay["subsampling"], lay["restart_interval"]) == want
    assert data[lay["scan_offset"] + lay["scan_bytes"]:] == b"\xff\xd9"
    blocks, status, found, errors = U.decode(scan, sampling, shapes, lay["restart_interval"])
    assert not status.any() and errors == 0 and found == len(status) - 1
    # the restatement's blocks through the exact IDCT lie within 1.0 of Pillow's pixels (luma)
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    if lay["components"] == 3:
        im.draft("YCbCr", im.size)
        assert im.mode == "YCbCr"
    px = np.asarray(im).astype(np.float64)
    luma = px if lay["components"] == 1 else px[..., 0]
    mine = np.clip(J.plane(J.idct(blocks[0], lay["q_luma"].reshape(64))), 0.0, 255.0)
    err = float(np.abs(mine[:lay["height"], :lay["width"]] - luma).max())
    print("%s: max |Pillow - float64 IDCT| = %.3f" % (name, err))
    assert err <= 1.0


def _segments(data):
    """{marker: offset of its FF} of the header's segments (the first of each kind)."""
    out, i = {}, 2
    while data[i + 1] != 0xda:
        out.setdefault(data[i + 1], i)
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    out[0xda] = i
    return out


def test_parse_refusals(hp):
    head = bytearray(hp.jpeg_header(45, 77, components=3, subsampling="420", restart_interval=5))
    seg = _segments(head)
    sof, dqt, dht, sos = seg[0xc0], seg[0xdb], seg[0xc4], seg[0xda]

    def status(h=head, tail=SCAN + b"\xff\xd9", patch=()):
        h = bytearray(h)
        for at, value in patch:
            h[at] = value
        with pytest.raises(hp.HpdctError) as e:
            hp.jpeg_parse(bytes(h) + tail)
        return e.value.status, str(e.value)

    assert hp.jpeg_parse(bytes(head) + SCAN + b"\xff\xd9")["components"] == 3
    unsupported = {
        "SOF0": [(sof + 1, 0xc2)],                        # a progressive frame
        "8 only": [(sof + 4, 12)],                        # 12-bit samples
        "16-bit DQT": [(dqt + 4, 0x10)],
        "components": [(sof + 9, 4)],
        "sampling": [(sof + 11, 0x21)],                   # 4:2:2
        "Huffman": [(dht + 5 + 16 + 3, 7)],               # a symbol of the DC luminance table
        "Ss / Se": [(sos + 4 + 1 + 6 + 1, 62)],
    }
    for text, patch in unsupported.items():
        st, msg = status(patch=patch)
        assert st == 2 and text in msg, (text, st, msg)
    st, msg = status(patch=[(sos + 4 + 1 + 6 + 2, 0x01)])              # Al = 1
    assert st == 2 and "Ss / Se" in msg
    st, msg = status(patch=[(dht + 5 + 16 + 12 + 1 + 2, 9)])             # a length count of the AC luminance table
    assert st in (1, 2)
    # Cb and Cr on different tables: a third table, selected by Cr
    third = bytes([0xff, 0xdb, 0, 67, 2]) + bytes([7] * 64)
    h3 = bytearray(head[:2] + third + head[2:])
    st, msg = status(h=h3, patch=[(len(third) + sof + 10 + 3 * 2 + 2, 2)])
    assert st == 2 and "Cb and Cr" in msg
    same = bytes([0xff, 0xdb, 0, 67, 2]) + bytes(head[dqt + 4 + 65 + 1:dqt + 4 + 130])
    h4 = bytearray(head[:2] + same + head[2:])
    h4[len(same) + sof + 10 + 3 * 2 + 2] = 2
    assert hp.jpeg_parse(bytes(h4) + SCAN + b"\xff\xd9")["components"] == 3     # equal contents are accepted
    # more than one scan: a second SOS where EOI belongs, or a scan of one component of three
    st, msg = status(tail=SCAN + bytes(head[sos:]) + SCAN + b"\xff\xd9")
    assert st == 2 and "more than one scan" in msg
    one = bytearray(head[:sos]) + bytes([0xff, 0xda, 0, 8, 1, 1, 0x00, 0, 63, 0])
    st, msg = status(h=one)
    assert st == 2 and "more than one scan" in msg
    # malformed and truncated files
    whole = bytes(head) + SCAN + b"\xff\xd9"
    for bad in (b"", b"\xff", b"\xff\xd8", whole[1:], whole[:-2], whole[:-1], whole[:len(head) - 3], whole[:sof + 6],
                bytes(head) + SCAN, bytes(head) + SCAN + b"\xff\xc0\x00\x02\xff\xd9", b"\x00" * 700):
        with pytest.raises(hp.HpdctError) as e:
            hp.jpeg_parse(bad)
        assert e.value.status == 1, (len(bad), str(e.value))
    st, msg = status(patch=[(sof + 2, 0xff), (sof + 3, 0xff)])           # a segment longer than the file
    assert st == 1
    L = hp.load_library()
    lay = (ctypes.c_uint8 * 600)()
    assert L.hpdct_jpeg_parse(None, 10, lay) == 1 and L.hpdct_jpeg_parse(lay, 10, None) == 1
    assert L.hpdct_jpeg_parse(lay, -1, lay) == 1
    assert ctypes.sizeof(hp._JpegLayout) == 4 * 8 + 2 * 4 + 8 + 2 * 256 == 560


# ---------------------------------------------------------------------------
# argument validation (fake pointers, never dereferenced)
# ---------------------------------------------------------------------------
Y, CB, CR, SC, INFO, OFFS, WS, ST = (1 << n for n in range(30, 38))


def _p(x):
    return None if x is None else ctypes.c_void_p(x)


def _dec(L, scan=SC, nbytes=4096, offs=OFFS, y=Y, cb=CB, cr=CR, h=16, w=32, sub=S420, ri=0, flags=0, info=INFO, st=ST,
         ws=WS, wsb=1 << 20):
    return L.hpdct_decode_scan(_p(scan), nbytes, _p(offs), _p(y), _p(cb), _p(cr), h, w, sub, ri, flags, _p(info), _p(st),
                               _p(ws), wsb, None)


def test_decode_scan_arguments_rejected(hp):
    L = hp.load_library()
    err = L.hpdct_last_error_string

    def passes_every_check(**kw):
        """The call gets as far as the workspace size, the last thing judged."""
        return _dec(L, wsb=0, **kw) == 1 and b"workspace too small" in err()

    assert passes_every_check()
    assert passes_every_check(cb=None, cr=None, h=8, w=8, sub=77)          # grey: sub is not read
    assert passes_every_check(offs=None) and passes_every_check(st=None) and passes_every_check(offs=None, st=None)
    assert passes_every_check(scan=SC + 1, nbytes=0) and passes_every_check(scan=SC + 3)   # no alignment rule
    for name in ("y", "scan", "info", "ws"):
        assert _dec(L, **{name: None}) == 1 and b"null" in err()
    assert _dec(L, cb=None) == 1 and b"null" in err()
    assert _dec(L, cr=None) == 1 and b"null" in err()
    for h, w, sub in ((0, 32, S420), (16, -16, S420), (24, 32, S420), (16, 40, S420), (12, 32, S444), (8, 20, S444)):
        assert _dec(L, h=h, w=w, sub=sub) == 1 and b"multiples of" in err()
    assert _dec(L, cb=None, cr=None, h=8, w=12) == 1 and b"multiples of 8" in err()
    assert passes_every_check(h=24, w=40, sub=S444) and passes_every_check(cb=None, cr=None, h=24, w=1016)
    assert _dec(L, h=1 << 23, w=1 << 23) == 1 and b"too large" in err()
    for sub in (2, -1):
        assert _dec(L, sub=sub) == 1 and b"subsampling" in err()
    for ri in (-1, 65536, 1 << 40):
        assert _dec(L, ri=ri) == 1 and b"restart_interval" in err()
    assert passes_every_check(ri=65535) and passes_every_check(ri=1)
    assert _dec(L, flags=0x80) == 2 and _dec(L, flags=hp.BLOCKS_NATURAL | 0x2) == 2
    assert passes_every_check(flags=hp.BLOCKS_NATURAL)
    assert _dec(L, nbytes=-1) == 1 and b"negative" in err()
    for name, base in (("y", Y), ("cb", CB), ("cr", CR), ("ws", WS), ("offs", OFFS), ("st", ST)):
        assert _dec(L, **{name: base + 8}) == 1 and b"aligned" in err()
    assert _dec(L, info=INFO + 4) == 1 and b"aligned" in err()
    assert passes_every_check(info=INFO + 8)
    # the workspace: 8 bytes per interval and per 4096 bytes of scan, each part a multiple of 16
    ws = L.hpdct_decode_workspace_bytes
    assert ws(16, 32, 3, S420, 0, 4096) == 32 and ws(16, 32, 3, S420, 1, 4096) == 32
    assert ws(16, 32, 3, S420, 0, 0) == 32 and ws(16, 32, 3, S420, 0, 4097) == 32 and ws(16, 32, 3, S420, 0, 8193) == 48
    assert ws(24, 1016, 1, 99, 1, 100000) == 8 * 382 + 8 * 26
    assert ws(8192, 8192, 1, 0, 1024, 1 << 25) == 8 * 1024 + 8 * 8192
    assert ws(16, 32, 2, S420, 0, 0) == -1 and ws(16, 24, 3, S420, 0, 0) == -1 and ws(16, 32, 3, 5, 0, 0) == -1
    assert ws(16, 32, 3, S420, 65536, 0) == -1 and ws(16, 32, 3, S420, 0, -1) == -1
    assert _dec(L, wsb=31) == 1 and b"workspace too small" in err()
    assert _dec(L, nbytes=8193, wsb=47) == 1 and b"workspace too small" in err()
    assert _dec(L, wsb=-5) == 1
    with pytest.raises(hp.HpdctError):
        hp.decode_workspace_bytes(16, 24, components=3)
    assert hp.decode_workspace_bytes(16, 32, components=3, scan_bytes=8193) == 48


def test_decode_scan_overlaps_rejected(hp):
    L = hp.load_library()
    err = L.hpdct_last_error_string

    def overlap(**kw):
        """Whether the sweep refuses the call; a call it lets through ends at the workspace size, judged last."""
        st = _dec(L, wsb=0, **kw)
        assert st == 1 and (b"overlap" in err() or b"workspace too small" in err()), (st, err())
        return b"overlap" in err()

    # 16 x 32 4:2:0: y 1024 bytes, cb and cr 256 each, scan 4096, info 16, offsets 16 (ri 1: 24), status 8 (16),
    # workspace 32
    assert overlap(cb=Y + 1008) and overlap(cr=CB + 240) and overlap(cr=Y)
    assert overlap(scan=Y + 1023, nbytes=1) and overlap(scan=Y - 4095)
    assert overlap(info=SC + 4088) and overlap(info=CR + 248)
    assert overlap(ri=1, offs=INFO) and overlap(ri=1, offs=WS + 16) and overlap(ri=1, ws=OFFS + 16)
    assert overlap(st=INFO) and overlap(ri=1, st=OFFS + 16) and overlap(st=WS + 16) and overlap(ws=ST)
    assert overlap(ws=INFO) and overlap(ws=Y + 1008) and overlap(st=SC + 4080)
    # just clear of each other
    for kw in (dict(cb=Y + 1024), dict(cr=CB + 256), dict(scan=Y + 1024, nbytes=1), dict(scan=Y - 4096),
               dict(info=SC + 4096), dict(ri=1, offs=WS + 32), dict(ws=OFFS + 16), dict(ri=1, ws=OFFS + 32),
               dict(scan=Y, nbytes=0), dict(offs=None, ws=OFFS), dict(st=None, ws=ST), dict(ws=ST + 16),
               dict(ri=1, st=OFFS + 32), dict(st=WS + 32), dict(st=SC + 4096)):
        assert not overlap(**kw), kw


def test_unscan_symbols_are_declared(hp):
    text = open(os.path.join(ROOT, "include", "hpdct.h")).read()
    for name in ("hpdct_decode_scan", "hpdct_decode_workspace_bytes", "hpdct_jpeg_parse"):
        assert name in hp.C_SYMBOLS and name + "(" in text
        getattr(hp.load_library(), name)
    assert "hpdct_decode_info" in text and "hpdct_jpeg_layout" in text


def test_unscan_wrapper_checks(hp):
    """The Python wrappers judge the buffers before the library is reached."""
    import torch as t
    from test_host_validation import FakeDev
    scan = FakeDev((100,), t.uint8)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.decode_scan(t.zeros(10, dtype=t.uint8), height=16, width=32)
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.decode_scan(FakeDev((100,), t.int8), height=16, width=32)
    with pytest.raises(hp.HpdctError, match="components"):
        hp.decode_scan(scan, height=16, width=32, components=2)
    with pytest.raises(hp.HpdctError, match="multiples of 16"):
        hp.decode_scan(scan, height=24, width=32, components=3)
    with pytest.raises(hp.HpdctError, match="multiples of 8"):
        hp.decode_scan(scan, height=24, width=36, components=3, subsampling="444")
    with pytest.raises(hp.HpdctError, match="restart_interval"):
        hp.decode_scan(scan, height=16, width=32, restart_interval=65536)
    with pytest.raises(ValueError):
        hp.decode_scan(scan, height=16, width=32, components=3, subsampling="422")
    y, c = FakeDev((2, 4, 64), t.int16), FakeDev((1, 2, 64), t.int16)
    info, ws = FakeDev((2,), t.int64), FakeDev((64,), t.uint8)
    with pytest.raises(hp.HpdctError, match="out holds"):
        hp.decode_scan(scan, height=16, width=32, components=3, out=(y,))
    with pytest.raises(hp.HpdctError, match="both"):
        hp.bind_decode_scan(scan, None, y, c, None, info, None, ws)
    with pytest.raises(hp.HpdctError, match="cb blocks holds"):
        hp.bind_decode_scan(scan, None, y, c, c, info, None, ws, subsampling="444")
    with pytest.raises(hp.HpdctError, match="y blocks holds"):
        hp.bind_decode_scan(scan, None, c, None, None, info, None, ws, height=16, width=32)
    with pytest.raises(hp.HpdctError, match="info"):
        hp.bind_decode_scan(scan, None, y, c, c, FakeDev((1,), t.int64), None, ws)
    with pytest.raises(hp.HpdctError, match="offsets holds"):
        hp.bind_decode_scan(scan, FakeDev((2,), t.int64), y, c, c, info, None, ws, restart_interval=1)
    with pytest.raises(hp.HpdctError, match="status holds"):
        hp.bind_decode_scan(scan, None, y, c, c, info, FakeDev((1,), t.int64), ws, restart_interval=1)
    with pytest.raises(hp.HpdctError, match="workspace holds"):
        hp.bind_decode_scan(scan, None, y, c, c, info, None, FakeDev((31,), t.uint8))
    with pytest.raises(hp.HpdctError, match="status dtype"):
        hp.bind_decode_scan(scan, None, y, c, c, info, FakeDev((2,), t.int32), ws)
    with pytest.raises(ValueError):
        hp.bind_decode_scan(scan, None, y, c, c, info, None, ws, order="diagonal")
    # a grey file under another table than the library's is refused before any device work
    q = np.full((8, 8), 9, np.float32)
    data = hp.jpeg_header(8, 8, components=1, q_luma=q) + b"\x00\xff\xd9"
    with pytest.raises(hp.HpdctError, match="set_quant_table"):
        hp.jpeg_decode(data)


def test_unscan_policy_rows(tmp_path):
    """tests/tools/policy_unscan_check.cpp: the decoder's launches as hpdct_policy.hpp chooses them."""
    host_programs.policy_check("policy_unscan_check", tmp_path)


# ---------------------------------------------------------------------------
# the refusals, the parser and the walker under ASan + UBSan
# ---------------------------------------------------------------------------
def test_unscan_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/tools/asan_unscan_check.cpp, its own main) with the C ABI's host sources (tests/tools/asan.mk's HOST) compiled by g++
    under tests/tools/asan.mk's ASan + UBSan flags: hpdct_decode_scan's refusals, hpdct_jpeg_parse on every
    truncation and corruption of a file, and unscan::walk_interval -- the function the decode kernel wraps -- over
    the whole corpus (grey and colour) and the built scans of tests/unscan_built.py, each at the eight addresses
    mod 8, compared with the restatement's results (the file written here, next to the program).  CPU only:
    nothing is launched, nothing is loaded into Python."""
    import unscan_built
    cases, results = unscan_corpus.cases_and_expected()
    built = unscan_built.corpus_cases()
    unscan_corpus.write_file(str(tmp_path / "unscan_corpus.bin"), list(cases) + built,
                             list(results) + [unscan_corpus.expected(c) for c in built])
    host_programs.sanitised_check("asan_unscan_check", tmp_path, "hpdct_unscan.o")
