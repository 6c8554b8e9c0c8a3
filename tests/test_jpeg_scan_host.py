"""Baseline-JPEG entropy coding, the CPU side (no GPU, no kernel runs):

- hpdct_huffman_table against the Annex K.3 literals of tests/jpeg_scan.py;
- the plain-Python restatement of the coding (jpeg_scan.encode), which the GPU
  tests compare the kernels with byte for byte, checked here: a round trip of the
  decoder-input catalogue through an independent table-walking decoder, and
  Pillow (libjpeg-turbo) as the outside decoder of hpdct_jpeg_header + encode +
  EOI;
- hpdct_encode_scan and hpdct_jpeg_header validate every argument before any
  device work (the pointers here are never dereferenced), once more in a
  stand-alone program under ASan + UBSan; the policy rows of the launches.
"""
import ctypes
import io
import os

import numpy as np
import pytest

import decoder_blocks
import host_programs
import jpeg_scan as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S444, S420 = 0, 1


# ---------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_huffman_tables_are_annex_k(hp, kind):
    bits, vals = hp.huffman_table(kind)
    want_bits, want_vals = J.TABLES[kind]
    assert bits.tolist() == want_bits and vals.tolist() == want_vals
    assert len(vals) == (12 if kind in (0, 2) else 162) == sum(want_bits) and len(set(vals.tolist())) == len(vals)
    # a full prefix code: the codes fill the code space up to the one all-ones word Annex C keeps free
    codes = J.codes_of(J.TABLES[kind])
    longest = max(ln for _, ln in codes.values())
    assert sum(2 ** (longest - ln) for _, ln in codes.values()) == 2 ** longest - 1
    words = sorted(format(c, "0%db" % ln) for c, ln in codes.values())
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))
    assert "1" * longest not in words
    name = {v: k for k, v in hp.HUFFMAN_TABLES.items()}[kind]
    assert hp.huffman_table(name)[1].tolist() == want_vals
    with pytest.raises(ValueError):
        hp.huffman_table(4)
    n = ctypes.c_int(-1)
    hp.load_library().hpdct_huffman_table(7, None, None, ctypes.addressof(n))
    assert n.value == 0
    hp.load_library().hpdct_huffman_table(kind, None, None, None)        # every output may be NULL


# ---------------------------------------------------------------------------
# the restatement: the catalogue through an independent decoder
# ---------------------------------------------------------------------------
def clipped_catalogue(oracle):
    """The first 381 catalogue blocks clipped to +-1023, zig-zag order, as the tiles of a 24 x 1016 frame."""
    cat, _ = decoder_blocks.catalogue(oracle.default_transform())
    return np.clip(cat[:decoder_blocks.FIRST], -1023, 1023)[:, J.ZIGZAG].reshape(3, 127, 64)


@pytest.mark.parametrize("ri", [0, 1, 5, 127])
def test_catalogue_round_trip(oracle, ri):
    x = clipped_catalogue(oracle)
    data, offsets = J.encode([x], "grey", ri)
    back, = J.decode(data, "grey", [(3, 127)], ri)
    assert np.array_equal(back, x)
    intervals = 1 if ri == 0 else -(-381 // ri)
    assert len(offsets) == intervals + 1 and offsets[0] == 0 and offsets[-1] == len(data)
    assert all(a < b for a, b in zip(offsets, offsets[1:]))
    for i in range(1, intervals):
        assert data[offsets[i] - 2:offsets[i]] == bytes([0xff, 0xd0 + ((i - 1) & 7)])
    assert J.out_of_range([x], "grey", ri) == 0
    # the input keeps exercising the hard paths
    assert data.count(b"\xff\x00") >= 1000
    flat = x.reshape(-1, 64).astype(np.int64)
    zrl = 0
    for blk in flat:
        nz = np.flatnonzero(blk[1:])
        zrl += int((np.diff(np.concatenate(([-1], nz))) - 1).__floordiv__(16).sum())
    assert zrl >= 100
    assert int((flat[:, 63] != 0).sum()) >= 50
    assert int(np.abs(flat[:, 1:]).max()).bit_length() == 10
    if ri == 0:
        assert int(np.abs(np.diff(np.concatenate(([0], flat[:, 0])))).max()).bit_length() == 11
    assert (flat == 0).all(axis=1).any()


def test_out_of_range_counts_what_baseline_cannot_code(oracle):
    cat, _ = decoder_blocks.catalogue(oracle.default_transform())
    raw = cat[:decoder_blocks.FIRST][:, J.ZIGZAG].reshape(3, 127, 64)
    with pytest.raises(ValueError):
        J.encode([raw], "grey", 0)
    n = J.out_of_range([raw], "grey", 0)
    assert n >= int((np.abs(raw[..., 1:].astype(np.int64)) > 1023).sum()) > 0
    one = np.zeros((1, 2, 64), np.int16)
    one[0, 0, 0], one[0, 1, 0], one[0, 1, 5] = 1024, -1024, -1024
    assert J.out_of_range([one], "grey", 0) == 2            # the difference -2048 and the AC value
    assert J.out_of_range([one], "grey", 1) == 1            # the predictor is 0 again: only the AC value


# ---------------------------------------------------------------------------
# Pillow as the outside decoder of hpdct_jpeg_header + encode + EOI
# ---------------------------------------------------------------------------
def _pillow(data, ycbcr=False):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    if ycbcr:
        im.draft("YCbCr", im.size)
        assert im.mode == "YCbCr"
    return np.asarray(im).astype(np.int64)


def _dc_pixels(dc, q00):
    return np.clip((dc.astype(np.int64) * q00 + 4) // 8 + 128, 0, 255)


def _dc_values(n, q00, seed):
    """n DC values with every pixel value reachable under q00, one step beyond both clamp edges included."""
    lo, hi = -(-(-128 * 8 - 4) // q00), (127 * 8 + 4) // q00            # pixel 0 and pixel 255
    edge = [lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, 0, 1, -1]
    edge += [max(-1023, lo - 1 - 8 // q00), min(1023, hi + 1 + 8 // q00)]
    rnd = np.random.default_rng(seed).integers(max(-1023, lo - 2), min(1023, hi + 2) + 1, n)
    vals = np.where(np.arange(n) % 3 == 0, np.resize(edge, n), rnd)
    return np.clip(vals, -1023, 1023).astype(np.int16)


@pytest.mark.parametrize("ri", [0, 1, 3, 37])
@pytest.mark.parametrize("q00", [16, 3, 1])
def test_pillow_decodes_grey_dc_blocks_exactly(hp, q00, ri):
    pytest.importorskip("PIL")
    blocks = np.zeros((3, 127, 64), np.int16)
    blocks[..., 0] = _dc_values(381, q00, 7 + q00).reshape(3, 127)
    want = _dc_pixels(blocks[..., 0], q00)
    assert want.min() == 0 and want.max() == 255
    q = np.full(64, 7, np.float32)
    q[0] = q00
    data, _ = J.encode([blocks], "grey", ri)
    got = _pillow(hp.jpeg_header(24, 1016, components=1, q_luma=q, restart_interval=ri) + data + b"\xff\xd9")
    assert got.shape == (24, 1016)
    assert np.array_equal(got, np.kron(want, np.ones((8, 8), np.int64)))


@pytest.mark.parametrize("ri", [0, 1, 3, 7])
@pytest.mark.parametrize("sampling", ["444", "420"])
def test_pillow_decodes_colour_dc_blocks_exactly(hp, sampling, ri):
    pytest.importorskip("PIL")
    f = 2 if sampling == "420" else 1
    my, mx = 4, 5                                                          # 20 MCUs: the marker index wraps at ri 1
    rng = np.random.default_rng(11)
    comps = [np.zeros((f * my, f * mx, 64), np.int16), np.zeros((my, mx, 64), np.int16),
             np.zeros((my, mx, 64), np.int16)]
    q00 = (16, 17, 17)                                                     # the library's and Annex K's chroma DC
    for c, q in zip(comps, q00):
        c[..., 0] = rng.integers(-1100 // q, 1100 // q, c.shape[:2])
    data, _ = J.encode(comps, sampling, ri)
    h, w = 8 * f * my, 8 * f * mx
    got = _pillow(hp.jpeg_header(h, w, components=3, subsampling=sampling, restart_interval=ri) + data + b"\xff\xd9",
                  ycbcr=True)
    assert got.shape == (h, w, 3)
    assert np.array_equal(got[..., 0], np.kron(_dc_pixels(comps[0][..., 0], 16), np.ones((8, 8), np.int64)))
    for c in (1, 2):
        want = np.kron(_dc_pixels(comps[c][..., 0], 17), np.ones((8 * f, 8 * f), np.int64))
        if sampling == "444":
            assert np.array_equal(got[..., c], want)
        else:
            # fancy upsampling mixes neighbouring blocks at an MCU's border: pixels 2..13 have all their
            # neighbours in one block
            inner = np.zeros((h, w), bool)
            for r in range(my):
                for col in range(mx):
                    inner[16 * r + 2:16 * r + 14, 16 * col + 2:16 * col + 14] = True
            assert np.array_equal(got[..., c][inner], want[inner])


def test_pillow_decodes_a_general_frame_within_the_idct_accuracy(hp, oracle):
    """A 24 x 1016 grey frame coded with the exact DCT and the default table: Pillow's pixels lie within 1.0 of the
    float64 exact-IDCT reconstruction (libjpeg's integer IDCT accuracy; an error of one quantisation step in a
    low-frequency coefficient moves pixels by more)."""
    pytest.importorskip("PIL")
    img = oracle.rand_u8(24 * 1016, 42).reshape(24, 1016).astype(np.float64)
    q = hp.default_quant_table().reshape(64).astype(np.float64)
    tiles = img.reshape(3, 8, 127, 8).transpose(0, 2, 1, 3) - 128.0
    coef = np.rint(J.fdct(tiles).reshape(3, 127, 64) / q).astype(np.int16)
    blocks = np.ascontiguousarray(coef[..., J.ZIGZAG])
    assert np.abs(blocks[..., 1:]).max() > 8                              # AC throughout, not a DC frame
    data, _ = J.encode([blocks], "grey", 127)
    got = _pillow(hp.jpeg_header(24, 1016, components=1, restart_interval=127) + data + b"\xff\xd9")
    want = np.clip(J.plane(J.idct(blocks, q)), 0.0, 255.0)
    err = float(np.abs(got - want).max())
    print("max |Pillow - float64 IDCT| = %.3f" % err)
    assert err <= 1.0


def test_header_layout(hp):
    """The segments in order, the TRUE size in SOF0, zig-zag DQT, two or four DHT tables, DRI only when asked."""
    q = np.arange(1, 65, dtype=np.float32)

    def segments(data):
        assert data[:2] == b"\xff\xd8"
        out, i = [], 2
        while i < len(data):
            assert data[i] == 0xff
            n = (data[i + 2] << 8) | data[i + 3]
            out.append((data[i + 1], data[i + 4:i + 2 + n]))
            i += 2 + n
        assert i == len(data)
        return out

    segs = segments(hp.jpeg_header(45, 77, components=3, subsampling="420", q_luma=q, restart_interval=5))
    assert [m for m, _ in segs] == [0xe0, 0xdb, 0xc0, 0xc4, 0xdd, 0xda]
    assert segs[0][1][:5] == b"JFIF\0"
    dqt = segs[1][1]
    assert dqt[0] == 0 and list(dqt[1:65]) == [int(q[z]) for z in J.ZIGZAG] and dqt[65] == 1
    assert list(dqt[66:]) == [int(hp.default_chroma_quant_table().reshape(64)[z]) for z in J.ZIGZAG]
    assert segs[2][1] == bytes([8, 0, 45, 0, 77, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    dht, p = segs[3][1], 0
    for ident, kind in ((0x00, 0), (0x10, 1), (0x01, 2), (0x11, 3)):
        bits, vals = J.TABLES[kind]
        assert dht[p] == ident and list(dht[p + 1:p + 17]) == bits and list(dht[p + 17:p + 17 + len(vals)]) == vals
        p += 17 + len(vals)
    assert p == len(dht)
    assert segs[4][1] == bytes([0, 5])
    assert segs[5][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    segs = segments(hp.jpeg_header(8, 65535, components=1))
    assert [m for m, _ in segs] == [0xe0, 0xdb, 0xc0, 0xc4, 0xda]
    assert len(segs[1][1]) == 65 and list(segs[1][1][1:]) == [int(hp.default_quant_table().reshape(64)[z])
                                                             for z in J.ZIGZAG]
    assert segs[2][1] == bytes([8, 0, 8, 0xff, 0xff, 1, 1, 0x11, 0])
    assert len(segs[3][1]) == 2 * 17 + 12 + 162
    assert segs[4][1] == bytes([1, 1, 0x00, 0, 63, 0])
    segs = segments(hp.jpeg_header(16, 16, components=3, subsampling="444"))
    assert segs[2][1][6:] == bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])


# ---------------------------------------------------------------------------
# argument validation (fake pointers, never dereferenced)
# ---------------------------------------------------------------------------
Y, CB, CR, SCAN, INFO, OFFS, WS = 1 << 30, 1 << 31, 1 << 32, 1 << 33, 1 << 34, 1 << 35, 1 << 36


def _p(x):
    return None if x is None else ctypes.c_void_p(x)


def _enc(L, y=Y, cb=CB, cr=CR, h=16, w=32, sub=S420, ri=0, flags=0, scan=SCAN, cap=4096, info=INFO, offs=OFFS,
         ws=WS, wsb=1 << 20):
    return L.hpdct_encode_scan(_p(y), _p(cb), _p(cr), h, w, sub, ri, flags, _p(scan), cap, _p(info), _p(offs), _p(ws),
                               wsb, None)


def test_encode_scan_arguments_rejected(hp):
    L = hp.load_library()
    err = L.hpdct_last_error_string

    def passes_every_check(**kw):
        """The call gets as far as the workspace size, the last thing judged."""
        return _enc(L, wsb=0, **kw) == 1 and b"workspace too small" in err()

    assert passes_every_check()
    assert passes_every_check(cb=None, cr=None, h=8, w=8, sub=77)          # grey: sub is not read
    assert passes_every_check(offs=None)
    assert passes_every_check(scan=SCAN + 1, cap=0)                        # the scan has no alignment rule
    for name in ("y", "scan", "info", "ws"):
        assert _enc(L, **{name: None}) == 1 and b"null" in err()
    assert _enc(L, cb=None) == 1 and b"null" in err()
    assert _enc(L, cr=None) == 1 and b"null" in err()
    for h, w, sub in ((0, 32, S420), (16, -16, S420), (24, 32, S420), (16, 40, S420), (12, 32, S444), (8, 20, S444)):
        assert _enc(L, h=h, w=w, sub=sub) == 1 and b"multiples of" in err()
    assert _enc(L, cb=None, cr=None, h=8, w=12) == 1 and b"multiples of 8" in err()
    assert passes_every_check(h=24, w=40, sub=S444) and passes_every_check(cb=None, cr=None, h=24, w=1016)
    assert _enc(L, h=1 << 23, w=1 << 23) == 1 and b"too large" in err()
    for sub in (2, -1):
        assert _enc(L, sub=sub) == 1 and b"subsampling" in err()
    for ri in (-1, 65536, 1 << 40):
        assert _enc(L, ri=ri) == 1 and b"restart_interval" in err()
    assert passes_every_check(ri=65535) and passes_every_check(ri=1)
    assert _enc(L, flags=0x80) == 2 and _enc(L, flags=hp.BLOCKS_NATURAL | 0x2) == 2
    assert passes_every_check(flags=hp.BLOCKS_NATURAL)
    assert _enc(L, cap=-1) == 1 and b"capacity" in err()
    for name, base in (("y", Y), ("cb", CB), ("cr", CR), ("ws", WS), ("offs", OFFS)):
        assert _enc(L, **{name: base + 8}) == 1 and b"aligned" in err()
    assert _enc(L, info=INFO + 4) == 1 and b"aligned" in err()
    assert passes_every_check(info=INFO + 8)
    # the workspace: 16 x 32 4:2:0 is 2 MCUs; one interval needs 16 bytes, two need 32
    assert hp.load_library().hpdct_scan_workspace_bytes(16, 32, 3, S420, 0) == 16
    assert hp.load_library().hpdct_scan_workspace_bytes(16, 32, 3, S420, 1) == 32
    assert _enc(L, wsb=15) == 1 and b"workspace too small" in err()
    assert _enc(L, ri=1, wsb=31) == 1 and b"workspace too small" in err()
    assert _enc(L, wsb=-5) == 1


def test_encode_scan_overlaps_rejected(hp):
    L = hp.load_library()
    err = L.hpdct_last_error_string

    def overlap(**kw):
        """Whether the sweep refuses the call; a call it lets through ends at the workspace size, judged last."""
        st = _enc(L, wsb=0, **kw)
        assert st == 1 and (b"overlap" in err() or b"workspace too small" in err()), (st, err())
        return b"overlap" in err()

    # 16 x 32 4:2:0: y 1024 bytes, cb and cr 256 each, info 16, offsets (ri 1: 2 intervals) 24, workspace 32
    assert overlap(cb=Y + 1008) and overlap(cr=CB + 240) and overlap(cr=Y)
    assert overlap(scan=Y + 1023, cap=1) and overlap(scan=Y - 4095)
    assert overlap(info=SCAN + 4088) and overlap(info=CR + 248)
    assert overlap(ri=1, offs=INFO) and overlap(ri=1, offs=WS + 16) and overlap(ri=1, ws=OFFS + 16)
    assert overlap(ws=INFO) and overlap(ws=Y + 1008)
    # just clear of each other
    for kw in (dict(cb=Y + 1024), dict(cr=CB + 256), dict(scan=Y + 1024, cap=1), dict(scan=Y - 4096),
               dict(info=SCAN + 4096), dict(ri=1, offs=WS + 32), dict(ws=OFFS + 16), dict(ri=1, ws=OFFS + 32),
               dict(scan=Y, cap=0), dict(offs=None, ws=OFFS)):
        assert not overlap(**kw)


def test_scan_bound_and_workspace(hp):
    assert hp.scan_bound(1, 1) == 419 and hp.scan_bound(0, 0) == 0
    assert hp.scan_bound(381, 3) == 415 * 381 + 12
    # alternating +-1023 blocks, about the longest a block gets (some 270 bytes), are within it
    for first in (1023, -1023):
        blk = np.tile(np.array([first, -first], np.int16), 32).reshape(1, 1, 64)
        data, _ = J.encode([blk], "grey", 0)
        assert 260 <= len(data) <= hp.scan_bound(1, 1)
    L = hp.load_library()
    assert L.hpdct_scan_bound(-1, 1) == -1 and L.hpdct_scan_bound(1, -1) == -1
    assert L.hpdct_scan_bound(1 << 62, 1) == -1
    with pytest.raises(hp.HpdctError):
        hp.scan_bound(-1, 0)
    ws = L.hpdct_scan_workspace_bytes
    assert ws(24, 1016, 1, 0, 127) == 48 and ws(24, 1016, 1, 99, 0) == 16 and ws(24, 1016, 1, 0, 1) == 4576
    assert ws(8192, 8192, 1, 0, 1024) == 16 * 768          # 12 bytes per interval, at most 16
    assert ws(24, 1016, 2, 0, 0) == -1 and ws(24, 1016, 3, 5, 0) == -1 and ws(24, 1016, 3, S420, 0) == -1
    assert ws(24, 1016, 1, 0, 65536) == -1
    # never more than the block arrays
    for h, w, comp, sub, ri in ((8, 8, 1, 0, 1), (16, 16, 3, S420, 1), (8, 8, 3, S444, 1), (24, 1016, 1, 0, 1)):
        assert ws(h, w, comp, sub, ri) <= 2 * h * w


def test_jpeg_header_arguments_rejected(hp):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    buf = np.zeros(1024, np.uint8)
    n = ctypes.c_int64(-1)

    def hdr(out=buf.ctypes.data, cap=1024, nb=ctypes.addressof(n), h=45, w=77, comp=3, sub=S420, ql=None, qc=None,
            ri=0):
        t = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)     # noqa: E731
        return L.hpdct_jpeg_header(_p(out), cap, _p(nb), h, w, comp, sub, t(ql), t(qc), ri)

    assert hdr() == 0 and n.value > 600 and bytes(buf[:2]) == b"\xff\xd8"
    full = n.value
    assert hdr(out=None) == 1 and hdr(nb=None) == 1 and b"null" in err()
    n.value = -1
    assert hdr(cap=full - 1) == 1 and n.value == full and b"too small" in err()
    assert hdr(cap=full) == 0 and hdr(cap=-1) == 1
    for h, w in ((0, 77), (45, 0), (-1, 77), (65536, 77), (45, 65536)):
        assert hdr(h=h, w=w) == 1 and b"65535" in err()
    assert hdr(h=65535, w=65535) == 0 and hdr(h=1, w=1) == 0
    assert hdr(comp=2) == 1 and hdr(comp=0) == 1 and hdr(comp=4) == 1
    assert hdr(sub=2) == 1 and b"subsampling" in err()
    assert hdr(comp=1, sub=2) == 0                                         # one component: sub is not read
    assert hdr(ri=-1) == 1 and hdr(ri=65536) == 1 and hdr(ri=65535) == 0
    good = np.full(64, 9, np.float32)
    for bad_value in (0.0, 256.0, 0.5, 16.5, -3.0, np.nan, np.inf):
        bad = good.copy()
        bad[17] = bad_value
        assert hdr(ql=bad) == 3 and b"luma" in err()
        assert hdr(qc=bad) == 3 and b"chroma" in err()
        assert hdr(comp=1, qc=bad) == 0                                    # one component: no chroma table
    edge = good.copy()
    edge[0], edge[63] = 1.0, 255.0
    assert hdr(ql=edge, qc=edge) == 0
    # the library table, when it is not a JPEG table
    hp.set_quant_table(np.full(64, 0.25, np.float32))
    try:
        assert hdr() == 3 and b"luma" in err()
        assert hdr(ql=good) == 0
    finally:
        hp.set_quant_table(None)
    with pytest.raises(hp.HpdctError) as e:
        hp.jpeg_header(65536, 8, components=1)
    assert e.value.status == 1


def test_scan_symbols_are_declared(hp):
    text = open(os.path.join(ROOT, "include", "hpdct.h")).read()
    for name in ("hpdct_encode_scan", "hpdct_scan_bound", "hpdct_scan_workspace_bytes", "hpdct_jpeg_header",
                 "hpdct_huffman_table"):
        assert name in hp.C_SYMBOLS and name + "(" in text
        getattr(hp.load_library(), name)
    assert ctypes.sizeof(ctypes.c_uint64) + 2 * ctypes.sizeof(ctypes.c_uint32) == 16     # hpdct_scan_info


def test_scan_wrapper_checks(hp):
    """The Python wrappers judge the buffers before the library is reached."""
    import torch as t
    from test_host_validation import FakeDev
    y, c = FakeDev((2, 4, 64), t.int16), FakeDev((1, 2, 64), t.int16)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.encode_scan(t.zeros((2, 4, 64), dtype=t.int16))
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.encode_scan(FakeDev((2, 4, 64), t.int8))
    with pytest.raises(hp.HpdctError, match="both"):
        hp.encode_scan(y, c, None)
    with pytest.raises(hp.HpdctError, match="multiples of 16"):
        hp.encode_scan(FakeDev((3, 4, 64), t.int16), c, c)
    with pytest.raises(hp.HpdctError, match="cb blocks holds"):
        hp.encode_scan(y, c, c, subsampling="444")
    with pytest.raises(hp.HpdctError, match="restart_interval"):
        hp.encode_scan(y, restart_interval=65536)
    with pytest.raises(hp.HpdctError, match="height and width"):
        hp.encode_scan(FakeDev((512,), t.int16))
    with pytest.raises(ValueError):
        hp.encode_scan(y, c, c, subsampling="422")
    with pytest.raises(ValueError):
        hp.bind_scan(y, None, None, None, None, None, None, order="diagonal")


def test_scan_policy_rows(tmp_path):
    """tests/tools/policy_scan_check.cpp: the coder's launches as hpdct_policy.hpp chooses them."""
    host_programs.policy_check("policy_scan_check", tmp_path)


# ---------------------------------------------------------------------------
# the same validation paths and the header writer under ASan + UBSan
# ---------------------------------------------------------------------------
def test_scan_validation_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/tools/asan_scan_check.cpp, its own main) drives hpdct_encode_scan's refusals
    and hpdct_jpeg_header with the C ABI's host sources (tests/tools/asan.mk's HOST) compiled by g++ under tests/tools/asan.mk's ASan + UBSan flags and the
    library's kernel objects linked as they are.  CPU only: nothing is launched, nothing is loaded into Python."""
    host_programs.sanitised_check("asan_scan_check", tmp_path, "hpdct_scan.o")
