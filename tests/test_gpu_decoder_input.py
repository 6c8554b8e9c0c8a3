"""The inverse kernels on decoder input the forward never makes: the block
catalogue of tests/decoder_blocks.py (all-zero, DC-only and single-coefficient
blocks, int16 values up to +-32767, blocks that drive most pixels far outside
0..255), non-finite fp32 coefficients, and finite tables so large that the
dequantised coefficient or a partial sum overflows.

Every comparison is exact: fp32 bit for bit (NaN-aware), uint8 and RGB with
array_equal.  References: oracle.idct / oracle.to_u8 on the plane holding
(float)block for the grey paths, test_gpu_rgb.ref_inverse for the colour paths.

Frames: 64x1024 holds the whole catalogue (1024 tiles, whole LDS-staged sets),
24x1016 its first 381 entries (sets straddling tile rows, a ragged last set).
Tables: the default, "x0.37" (not integers) and "signed" (x0.37 with the sign
flipped at odd positions: negative entries are legal and make -0 operands).

Huge tables.  The integer-input inverses skip the zero entries of the built-in
T, which is exact only while every operand and partial sum is finite; the
library keeps that to tables with max|Q| * qmax * c^2 < FLT_MAX (c the largest
column abs-sum of T, qmax 32768 for int16 blocks and 128 for int8) and runs
the full chain beyond it.  (a) one entry of 2e34: q * Q is infinite, the
reference gives NaN (0 * inf) and Inf; (b) a uniform 2e33: a pass overflows
while q * Q stays finite; (c) a uniform table just below the criterion: all
finite, the skipping kernels.  The int8 cases scale the tables by 256.
"""
import numpy as np
import pytest

import decoder_blocks as D
from test_gpu_parity import to_dev, to_host
from test_gpu_rgb import CHROMA_K, ref_inverse, rgb_preclamp
from test_gpu_rgb_frame import assert_only_the_frame_written, frame_buffer
from test_gpu_roundtrip import nan_aware_bits_equal

pytestmark = pytest.mark.gpu

FRAMES = [(64, 1024), (24, 1016)]
FRAME_IDS = ["%dx%d" % f for f in FRAMES]
TABLES = ["default", "x0.37", "signed"]
ORDERS = ["zigzag", "natural"]
FLT_MAX = float(np.finfo(np.float32).max)


def grey_table(oracle, name):
    q = oracle.default_quant().astype(np.float32)
    if name == "default":
        return q
    t = (q * np.float32(0.37)).astype(np.float32)
    if name == "x0.37":
        return t
    if name == "signed":
        t.reshape(-1)[1::2] *= np.float32(-1)
        return t
    raise KeyError(name)


def colour_tables(oracle, name):
    """(luma, chroma) as the reference sees them, and as the call is given them."""
    if name == "default":
        return (oracle.default_quant().astype(np.float32), CHROMA_K), (None, None)
    t = [(q * np.float32(0.37)).astype(np.float32) for q in (oracle.default_quant(), CHROMA_K)]
    if name == "signed":
        for q in t:
            q.reshape(-1)[1::2] *= np.float32(-1)
    return tuple(t), tuple(t)


def differing(a, b):
    """Number of fp32 values that differ (two NaNs are equal)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


@pytest.fixture(scope="module")
def zz(hp):
    return hp.zigzag_order().astype(np.int64)


@pytest.fixture(scope="module")
def T(oracle):
    return oracle.default_transform()


@pytest.fixture()
def use_table(hp):
    """Sets the library's table for one test and restores the default after it."""
    yield hp.set_quant_table
    hp.set_quant_table(None)


@pytest.fixture()
def use_mapping(hp):
    yield hp.set_mapping
    hp.set_mapping("auto")


_cache = {}


def grey_case(oracle, T, frame, table, int8=False):
    """(natural-order blocks, reference fp32 pixels, reference uint8 pixels) of a frame; computed once, read-only."""
    key = ("grey", frame, table, int8)
    if key not in _cache:
        h, w = frame
        blocks = D.take(T, (h // 8) * (w // 8))
        if int8:
            blocks = np.clip(blocks, -128, 127)
        rec = oracle.idct(D.plane_of(blocks, h, w), Q=grey_table(oracle, table))
        out = (blocks, rec, oracle.to_u8(rec))
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def check_inverse_blocks(hp, dev, zz, frame, blocks, rec, rec8, what):
    import torch
    h, w = frame
    for order in ORDERS:
        b = to_dev(D.in_order(blocks, zz, order).reshape(h // 8, w // 8, 64), dev)
        got32 = to_host(hp.inverse_blocks(b, order=order))
        got8 = to_host(hp.inverse_blocks(b, out_dtype=torch.uint8, order=order))
        print("inverse_blocks %s %s: %d fp32 pixels and %d uint8 pixels of %d differ" %
              (what, order, differing(got32, rec), int((got8 != rec8).sum()), rec.size))
        assert got32.shape == frame and nan_aware_bits_equal(got32, rec), order
        assert np.array_equal(got8, rec8), order


def check_inverse_int8(hp, dev, frame, blocks, rec, rec8, what):
    import torch
    h, w = frame
    assert blocks.min() >= -128 and blocks.max() <= 127
    coef = to_dev(D.plane_of(blocks, h, w).astype(np.int8), dev)
    got32 = to_host(hp.inverse(coef, out_dtype=torch.float32))
    got8 = to_host(hp.inverse(coef, out_dtype=torch.uint8))
    print("inverse int8 %s: %d fp32 pixels and %d uint8 pixels of %d differ" %
          (what, differing(got32, rec), int((got8 != rec8).sum()), rec.size))
    assert nan_aware_bits_equal(got32, rec)
    assert np.array_equal(got8, rec8)


# ------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("mapping", ["auto", "octet"])
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("frame", FRAMES, ids=FRAME_IDS)
def test_inverse_blocks_on_the_catalogue(hp, oracle, dev, zz, T, use_table, use_mapping, frame, table, mapping):
    blocks, rec, rec8 = grey_case(oracle, T, frame, table)
    use_table(None if table == "default" else grey_table(oracle, table))
    use_mapping(mapping)
    check_inverse_blocks(hp, dev, zz, frame, blocks, rec, rec8, "%s %s %s" % (frame, table, mapping))


@pytest.mark.parametrize("mapping", ["tile", "octet"])
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("frame", FRAMES, ids=FRAME_IDS)
def test_inverse_int8_on_the_clipped_catalogue(hp, oracle, dev, T, use_table, use_mapping, frame, table, mapping):
    """The catalogue clipped to int8: the zero, dc, basis and dense classes survive with values +-127 / -128."""
    blocks, rec, rec8 = grey_case(oracle, T, frame, table, int8=True)
    assert blocks.min() == -128 and blocks.max() == 127
    use_table(None if table == "default" else grey_table(oracle, table))
    use_mapping(mapping)
    check_inverse_int8(hp, dev, frame, blocks, rec, rec8, "%s %s %s" % (frame, table, mapping))


# ------------------------------------------------ non-finite fp32 coefficients
@pytest.mark.parametrize("mapping", ["tile", "octet", "duo"])
def test_inverse_nonfinite_fp32_coefficients(hp, oracle, dev, use_mapping, mapping):
    """+inf, -inf, NaN, +-3e38 and a subnormal among noise coefficients: fp32 out bit for bit, and the uint8
    clamp (convertToUnsignedChar: NaN -> 0, +inf -> 255, -inf -> 0, 4.3e9 -> 255)."""
    import torch
    assert oracle.to_u8(np.array([np.nan, np.inf, -np.inf, 4.3e9], np.float32)).tolist() == [0, 255, 0, 255]
    coef = np.round(np.random.default_rng(1).uniform(-30, 30, (16, 32))).astype(np.float32)
    coef[1, 2] = np.inf
    coef[9, 20] = np.nan
    coef[12, 5] = -np.inf
    coef[3, 30] = 3.0e38
    coef[11, 27] = -3.0e38
    coef[5, 17] = 1e-42  # subnormal
    rec = oracle.idct(coef)
    rec8 = oracle.to_u8(rec)
    assert np.isnan(rec).any() and (rec == np.inf).any() and (rec == -np.inf).any() and np.isfinite(rec).any()
    use_mapping(mapping)
    x = to_dev(coef, dev)
    got32 = to_host(hp.inverse(x))
    got8 = to_host(hp.inverse(x, out_dtype=torch.uint8))
    print("inverse non-finite %s: %d fp32 and %d uint8 pixels differ" %
          (mapping, differing(got32, rec), int((got8 != rec8).sum())))
    assert nan_aware_bits_equal(got32, rec)
    assert np.array_equal(got8, rec8)


# ---------------------------------------------------------------------- colour
# (subsampling, padded height, padded width) -> the three natural-order block lists
OFFSETS = (0, 341, 683)


def colour_blocks(T, sub, hp_, wp_):
    ny = (hp_ // 8) * (wp_ // 8)
    nc = ny // 4 if sub == "420" else ny
    return [D.take(T, n, off) for n, off in zip((ny, nc, nc), OFFSETS)]


def colour_case(oracle, T, sub, hp_, wp_, table):
    """(block lists, reference RGB of the padded frame), computed once, read-only; the reference is checked
    to exercise the clamps before the GPU is asked."""
    key = ("rgb", sub, hp_, wp_, table)
    if key not in _cache:
        blocks = colour_blocks(T, sub, hp_, wp_)
        ch, cw = (hp_ // 2, wp_ // 2) if sub == "420" else (hp_, wp_)
        coefs = [D.plane_of(b, h, w) for b, (h, w) in zip(blocks, ((hp_, wp_), (ch, cw), (ch, cw)))]
        (ql, qc), _ = colour_tables(oracle, table)
        planes = [oracle.to_u8(oracle.idct(np.array(c), Q=q)) for c, q in zip(coefs, (ql, qc, qc))]
        for p, name in zip(planes, ("Y", "Cb", "Cr")):
            assert (p == 0).any() and (p == 255).any() and ((p > 0) & (p < 255)).any(), name
        for c, name in zip(rgb_preclamp(*planes, sub), "RGB"):
            assert c.max() > 255 and c.min() < 0, name
        want = ref_inverse(oracle, coefs, sub, ql, qc)
        want.setflags(write=False)
        _cache[key] = (blocks, want)
    return _cache[key]


def device_blocks(dev, zz, blocks, sub, hp_, wp_, order):
    ch, cw = (hp_ // 2, wp_ // 2) if sub == "420" else (hp_, wp_)
    return [to_dev(D.in_order(b, zz, order).reshape(h // 8, w // 8, 64), dev)
            for b, (h, w) in zip(blocks, ((hp_, wp_), (ch, cw), (ch, cw)))]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("sub,h,w", [("444", 64, 512), ("420", 128, 1024)], ids=["444-64x512", "420-128x1024"])
def test_inverse_rgb_blocks_on_the_catalogue(hp, oracle, dev, zz, T, sub, h, w, table, order):
    blocks, want = colour_case(oracle, T, sub, h, w, table)
    _, (ql, qc) = colour_tables(oracle, table)
    y, cb, cr = device_blocks(dev, zz, blocks, sub, h, w, order)
    got = to_host(hp.inverse_rgb_blocks(y, cb, cr, subsampling=sub, q_luma=ql, q_chroma=qc, order=order))
    print("inverse_rgb_blocks %s %dx%d %s %s: %d bytes differ" % (sub, h, w, table, order, int((got != want).sum())))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("sub,h,w", [("444", 13, 515), ("420", 25, 1033)], ids=["444-13x515", "420-25x1033"])
def test_inverse_rgb_frame_on_the_catalogue(hp, oracle, dev, zz, T, sub, h, w, table, order):
    side = 16 if sub == "420" else 8
    hp_, wp_ = -(-h // side) * side, -(-w // side) * side
    blocks, want = colour_case(oracle, T, sub, hp_, wp_, table)
    _, (ql, qc) = colour_tables(oracle, table)
    y, cb, cr = device_blocks(dev, zz, blocks, sub, hp_, wp_, order)
    buf, out = frame_buffer(dev, h, w, 3 * w)
    hp.inverse_rgb_frame(y, cb, cr, height=h, width=w, subsampling=sub, q_luma=ql, q_chroma=qc, order=order, out=out)
    assert_only_the_frame_written(buf, h, w, 3 * w, 0, want[:h, :w])


# ---------------------------------------------------------- huge finite tables
def skip_limit(T, qmax):
    """The largest fp32 q with q * qmax * c^2 (and the library's rounding margin) below FLT_MAX: a uniform
    table of it is the last one the zero-skipping kernels take."""
    c = float(np.abs(np.asarray(T, np.float64)).sum(axis=0).max())
    q = np.float32(FLT_MAX / (qmax * c * c * (1.0 + 1e-5)))
    while float(q) * qmax * c * c * (1.0 + 1e-5) >= FLT_MAX:
        q = np.nextafter(q, np.float32(0))
    return q


def huge_case(oracle, T, kind, qmax):
    """(frame, natural-order blocks, table, reference fp32, reference uint8) of a huge-table case for
    coefficients up to qmax; the reference is checked for what the case is about."""
    key = ("huge", kind, qmax)
    if key not in _cache:
        scale = np.float32(32768 // qmax)
        if kind == "a":
            table = oracle.default_quant().astype(np.float32)
            table[0, 1] = np.float32(2e34) * scale
        elif kind == "b":
            table = np.full((8, 8), np.float32(2e33) * scale, np.float32)
        else:
            table = np.full((8, 8), skip_limit(T, qmax), np.float32)
        assert np.isfinite(table).all()
        if kind == "b":
            frame, blocks = (8, 16), D.of_classes(T, {"worst-sign"})
        else:
            frame, blocks = (24, 1056), D.of_classes(T, {"dc", "basis", "worst-sign"})
        assert len(blocks) == (frame[0] // 8) * (frame[1] // 8)
        blocks = np.clip(blocks, -qmax, qmax - 1)
        assert np.abs(blocks.astype(np.int64)).max() >= qmax - 1
        plane = D.plane_of(blocks, *frame)
        rec = oracle.idct(plane, Q=table)
        with np.errstate(over="ignore"):
            d = plane.reshape(frame[0] // 8, 8, frame[1] // 8, 8) * table[None, :, None, :]
        if kind == "a":
            assert np.isinf(d).any() and np.isnan(rec).any() and np.isinf(rec).any()
        elif kind == "b":
            assert np.isfinite(d).all() and not np.isfinite(rec).all()
        else:
            assert np.isfinite(rec).all()
        _cache[key] = (frame, blocks, table, rec, oracle.to_u8(rec))
    return _cache[key]


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_huge_table_inverse_blocks(hp, oracle, dev, zz, T, use_table, kind):
    frame, blocks, table, rec, rec8 = huge_case(oracle, T, kind, 32768)
    use_table(table)
    check_inverse_blocks(hp, dev, zz, frame, blocks, rec, rec8, "huge table (%s)" % kind)


@pytest.mark.parametrize("mapping", ["tile", "octet"])
@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_huge_table_inverse_int8(hp, oracle, dev, T, use_table, use_mapping, kind, mapping):
    frame, blocks, table, rec, rec8 = huge_case(oracle, T, kind, 128)
    use_table(table)
    use_mapping(mapping)
    check_inverse_int8(hp, dev, frame, blocks, rec, rec8, "huge table (%s) %s" % (kind, mapping))


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_huge_table_inverse_rgb_blocks(hp, oracle, dev, zz, T, kind):
    """4:4:4 with the huge table for luma and chroma; Cb and Cr take the case's blocks from other offsets."""
    (h, w), blocks, table, _, _ = huge_case(oracle, T, kind, 32768)
    n = len(blocks)
    comps = [blocks[(np.arange(n) + off) % n] for off in (0, n // 3, 2 * n // 3 + 1)]
    coefs = [D.plane_of(b, h, w) for b in comps]
    want = ref_inverse(oracle, coefs, "444", table, table)
    for order in ORDERS:
        y, cb, cr = device_blocks(dev, zz, comps, "444", h, w, order)
        got = to_host(hp.inverse_rgb_blocks(y, cb, cr, subsampling="444", q_luma=table, q_chroma=table, order=order))
        print("inverse_rgb_blocks huge table (%s) %s: %d bytes of %d differ" %
              (kind, order, int((got != want).sum()), want.size))
        assert np.array_equal(got, want), order
