"""Colour frames on the GPU (hpdct_forward_rgb_blocks / hpdct_inverse_rgb_blocks):
exact equality with the host reference everywhere, no tolerance.

Reference: the integer formulas of include/hpdct.h in numpy int64 (conversion,
the 2x2 chroma average, the inverse conversion with flooring shifts) around
oracle.fdct(plane, Q=table) / oracle.idct / oracle.to_u8 per component,
regrouped into blocks as test_gpu_blocks._to_blocks does.

Shapes.  4:4:4 (one lane per 8x8 pixel tile, 64 per wave): the six of
test_gpu_blocks.py.  4:2:0 (one lane per 16x16 MCU, 64 per wave):
  16x16      1 MCU: one live lane
  16x1040    65: a whole set plus a one-MCU ragged set
  32x528     33 per row: a set spanning two MCU rows (chroma staged, Y direct)
  48x2032    381: sets straddling MCU rows and a ragged last one
  128x1024   512: 8 whole sets in one MCU row each: the 16 KiB staged Y stores
  256x2048   2048: several workgroups

The rounding pattern of test_conversion_extremes: a strict two-colour
checkerboard puts two pixels of each colour in every 2x2 quad, so its quad sums
2 (a + b) are always even and can never be 1 or 3 mod 4.  The pattern here
holds 0..4 pixels of the second colour per quad (filled in checkerboard
order), with colours whose Cb and Cr differ by an odd amount, and the test
asserts on the reference that the quad sums reach 1, 2 and 3 mod 4.
"""
import numpy as np
import pytest

from test_gpu_blocks import _to_blocks
from test_gpu_parity import to_dev, to_host

pytestmark = pytest.mark.gpu

SHAPES = {"444": [(8, 8), (8, 520), (16, 264), (24, 1016), (64, 512), (512, 1024)],
          "420": [(16, 16), (16, 1040), (32, 528), (48, 2032), (128, 1024), (256, 2048)]}
CASES = [(s, shape) for s in ("444", "420") for shape in SHAPES[s]]
CASE_IDS = ["%s-%dx%d" % (s, h, w) for s, (h, w) in CASES]
TABLES = ["default", "q75", "x0.37"]
ORDERS = ["zigzag", "natural"]

CHROMA_K = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                     24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32,
                    np.float32).reshape(8, 8)


def _tables(oracle, name):
    """(luma, chroma) as the reference sees them, and as the call is given them."""
    ql, qc = oracle.default_quant().astype(np.float32), CHROMA_K
    if name == "default":
        return (ql, qc), (None, None)                       # JPEG forms for Y, 3-op quotient for chroma
    if name == "q75":                                       # libjpeg quality 75: integers (3-op quotient for both)
        t = tuple(np.maximum(np.floor((q * 50 + 50) / 100), 1).astype(np.float32) for q in (ql, qc))
        return t, t
    if name == "x0.37":                                     # not integers: IEEE division
        t = tuple((q * np.float32(0.37)).astype(np.float32) for q in (ql, qc))
        return t, t
    raise KeyError(name)


def ycc_of(rgb):
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def quad_sums(p):
    return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]


def planes_of(rgb, sub):
    """The three uint8 component planes the transform sees."""
    y, cb, cr = ycc_of(rgb)
    if sub == "420":
        cb, cr = (quad_sums(cb) + 2) >> 2, (quad_sums(cr) + 2) >> 2
    for p in (y, cb, cr):
        assert p.min() >= 0 and p.max() <= 255
    return tuple(p.astype(np.uint8) for p in (y, cb, cr))


def rgb_preclamp(y, cb, cr, sub):
    """uint8 component planes -> the int64 R, G, B before the clamp."""
    y, cb, cr = (p.astype(np.int64) for p in (y, cb, cr))
    if sub == "420":
        cb, cr = (np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in (cb, cr))
    cb, cr = cb - 128, cr - 128
    return (y + ((91881 * cr + 32768) >> 16),
            y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
            y + ((116130 * cb + 32768) >> 16))


def rgb_of(y, cb, cr, sub):
    return np.stack([np.clip(c, 0, 255) for c in rgb_preclamp(y, cb, cr, sub)], axis=-1).astype(np.uint8)


def ref_forward(oracle, rgb, sub, ql, qc):
    """The quantised fp32 planes (Y, Cb, Cr) of an (H, W, 3) frame."""
    y, cb, cr = planes_of(rgb, sub)
    return oracle.fdct(y, Q=ql), oracle.fdct(cb, Q=qc), oracle.fdct(cr, Q=qc)


def ref_inverse(oracle, coefs, sub, ql, qc):
    y, cb, cr = (oracle.to_u8(oracle.idct(np.array(c), Q=q)) for c, q in zip(coefs, (ql, qc, qc)))
    return rgb_of(y, cb, cr, sub)


def blocks_of(coefs, zz, order, shape3=False):
    out = []
    for c in coefs:
        b = np.ascontiguousarray(_to_blocks(c, zz, order).astype(np.int16))
        out.append(b.reshape(c.shape[0] // 8, c.shape[1] // 8, 64) if shape3 else b)
    return out


_cache = {}


def _case(oracle, sub, shape, table):
    """(rgb, reference coefficient planes, reference RGB of their inverse), computed once and never written to."""
    key = (sub, shape, table)
    if key not in _cache:
        h, w = shape
        rgb = oracle.rand_u8(3 * h * w, 42).reshape(h, w, 3)
        (ql, qc), _ = _tables(oracle, table)
        coefs = ref_forward(oracle, rgb, sub, ql, qc)
        _cache[key] = (rgb, coefs, ref_inverse(oracle, coefs, sub, ql, qc))
    return _cache[key]


@pytest.fixture(scope="module")
def zz(hp):
    return hp.zigzag_order().astype(np.int64)


def _differ(got, want):
    return sum(int((to_host(g).reshape(-1) != w.reshape(-1)).sum()) for g, w in zip(got, want))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("sub,shape", CASES, ids=CASE_IDS)
def test_forward_matches_reference(hp, oracle, dev, zz, sub, shape, table, order):
    import torch
    rgb, coefs, _ = _case(oracle, sub, shape, table)
    want = blocks_of(coefs, zz, order)
    _, (ql, qc) = _tables(oracle, table)
    got = hp.forward_rgb_blocks(to_dev(rgb, dev), subsampling=sub, q_luma=ql, q_chroma=qc, order=order)
    ch, cw = (shape[0] // 2, shape[1] // 2) if sub == "420" else shape
    assert all(g.dtype == torch.int16 for g in got)
    assert [tuple(g.shape) for g in got] == [(shape[0] // 8, shape[1] // 8, 64)] + [(ch // 8, cw // 8, 64)] * 2
    print("forward_rgb %s %s %s %s: %d values differ" % (sub, shape, table, order, _differ(got, want)))
    for g, w, name in zip(got, want, "y cb cr".split()):
        assert np.array_equal(to_host(g).reshape(-1, 64), w), name


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("sub,shape", CASES, ids=CASE_IDS)
def test_inverse_matches_reference(hp, oracle, dev, zz, sub, shape, table, order):
    import torch
    _, coefs, want = _case(oracle, sub, shape, table)
    _, (ql, qc) = _tables(oracle, table)
    y, cb, cr = (to_dev(b, dev) for b in blocks_of(coefs, zz, order, shape3=True))
    got = hp.inverse_rgb_blocks(y, cb, cr, subsampling=sub, q_luma=ql, q_chroma=qc, order=order)
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape + (3,)
    got = to_host(got)
    print("inverse_rgb %s %s %s %s: %d bytes differ" % (sub, shape, table, order, int((got != want).sum())))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("sub,shape", [("444", (24, 1016)), ("420", (48, 2032))], ids=["444", "420"])
def test_y_equals_the_plane_path(hp, oracle, dev, sub, shape, table):
    """d_y is hpdct_forward_blocks of the Y plane under set_quant_table(luma), and each array goes straight
    into hpdct_inverse_blocks."""
    import torch
    rgb, coefs, _ = _case(oracle, sub, shape, table)
    (ql, qc), (pl, pc) = _tables(oracle, table)
    y, cb, cr = hp.forward_rgb_blocks(to_dev(rgb, dev), subsampling=sub, q_luma=pl, q_chroma=pc)
    yp, cbp, crp = planes_of(rgb, sub)
    hp.set_quant_table(ql)
    try:
        assert np.array_equal(to_host(y), to_host(hp.forward_blocks(to_dev(yp, dev))))
        back = to_host(hp.inverse_blocks(y, out_dtype=torch.uint8))
        assert np.array_equal(back, oracle.to_u8(oracle.idct(np.array(coefs[0]), Q=ql)))
        hp.set_quant_table(qc)
        assert np.array_equal(to_host(cb), to_host(hp.forward_blocks(to_dev(cbp, dev))))
        assert np.array_equal(to_host(cr), to_host(hp.forward_blocks(to_dev(crp, dev))))
    finally:
        hp.set_quant_table(None)


def _corner_image():
    img = np.zeros((16, 128, 3), np.uint8)
    for k in range(8):
        img[:, 16 * k:16 * k + 16] = [255 * (k & 1), 255 * ((k >> 1) & 1), 255 * ((k >> 2) & 1)]
    return img


def _rounding_image():
    """Two colours; quad q of a row of quads holds q % 5 pixels of the second one, placed in checkerboard
    order (the two diagonal cells first)."""
    # (Y, Cb, Cr) = (141, 161, 99) and (140, 160, 98): a quad with k pixels of b sums to 4 a - k
    a, b = np.array([100, 150, 200], np.uint8), np.array([98, 150, 196], np.uint8)
    img = np.empty((32, 160, 3), np.uint8)
    img[:] = a
    cells = [(0, 0), (1, 1), (0, 1), (1, 0)]
    for qy in range(16):
        for qx in range(80):
            for dy, dx in cells[:(qx + qy) % 5]:
                img[2 * qy + dy, 2 * qx + dx] = b
    return img


@pytest.mark.parametrize("sub", ["444", "420"])
def test_conversion_extremes(hp, oracle, dev, zz, sub):
    corners, rounding = _corner_image(), _rounding_image()
    _, cb, cr = ycc_of(corners)
    for p in (cb, cr):
        assert p.min() == 0 and p.max() == 255                  # the formulas' whole range, no clamp
    _, cb, cr = ycc_of(rounding)
    for p in (cb, cr):
        assert {1, 2, 3} <= set((quad_sums(p) % 4).reshape(-1).tolist())   # the + 2 >> 2 rounding at work
    (ql, qc), _ = _tables(oracle, "default")
    ones = np.ones((8, 8), np.float32)
    for img in (corners, rounding):
        for tl, tc in ((None, None), (ones, ones)):             # the all-ones tables keep every unit of the values
            coefs = ref_forward(oracle, img, sub, ql if tl is None else tl, qc if tc is None else tc)
            want = blocks_of(coefs, zz, "zigzag")
            got = hp.forward_rgb_blocks(to_dev(img, dev), subsampling=sub, q_luma=tl, q_chroma=tc)
            for g, w, name in zip(got, want, "y cb cr".split()):
                assert np.array_equal(to_host(g).reshape(-1, 64), w), name


@pytest.mark.parametrize("sub", ["444", "420"])
def test_inverse_gamut(hp, oracle, dev, zz, sub):
    """Flat component planes whose RGB leaves the cube on every side: the clamp, not a wrap."""
    colours = [(250, 5, 250), (5, 5, 5), (250, 5, 5), (5, 250, 250), (250, 250, 128)]
    y = np.concatenate([np.full((16, 16), c[0], np.uint8) for c in colours], axis=1)
    n = 8 if sub == "420" else 16
    cb = np.concatenate([np.full((n, n), c[1], np.uint8) for c in colours], axis=1)
    cr = np.concatenate([np.full((n, n), c[2], np.uint8) for c in colours], axis=1)
    (ql, qc), _ = _tables(oracle, "default")
    coefs = (oracle.fdct(y, Q=ql), oracle.fdct(cb, Q=qc), oracle.fdct(cr, Q=qc))
    planes = [oracle.to_u8(oracle.idct(np.array(c), Q=q)) for c, q in zip(coefs, (ql, qc, qc))]
    for c, name in zip(rgb_preclamp(*planes, sub), "RGB"):
        assert c.max() > 255 and c.min() < 0, name               # on the reference, before the clamp
    want = rgb_of(*planes, sub)
    for order in ORDERS:
        b = [to_dev(x, dev) for x in blocks_of(coefs, zz, order, shape3=True)]
        got = to_host(hp.inverse_rgb_blocks(*b, subsampling=sub, order=order))
        assert np.array_equal(got, want), order


@pytest.mark.parametrize("sub,shape", [("444", (64, 512)), ("420", (128, 1024))], ids=["444", "420"])
def test_two_tables_on_two_streams(hp, oracle, dev, zz, sub, shape):
    """The tables travel with each call: two forwards with different pairs on two streams at once."""
    import torch
    x = to_dev(_case(oracle, sub, shape, "default")[0], dev)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    names = ["q75", "x0.37"]
    got = []
    for s, name in zip(streams, names):
        _, (ql, qc) = _tables(oracle, name)
        got.append(hp.forward_rgb_blocks(x, subsampling=sub, q_luma=ql, q_chroma=qc, stream=s))
    for s in streams:
        s.synchronize()
    for g3, name in zip(got, names):
        want = blocks_of(_case(oracle, sub, shape, name)[1], zz, "zigzag")
        for g, w, comp in zip(g3, want, "y cb cr".split()):
            assert np.array_equal(to_host(g).reshape(-1, 64), w), (name, comp)


@pytest.mark.parametrize("sub,shape", [("444", (8, 520)), ("444", (64, 512)), ("420", (16, 1040)),
                                       ("420", (48, 2032)), ("420", (128, 1024))],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_memory_beyond_the_buffers_is_untouched(hp, oracle, dev, zz, sub, shape):
    import torch
    h, w = shape
    rgb, coefs, back = _case(oracle, sub, shape, "default")
    want = blocks_of(coefs, zz, "zigzag")
    pad = 64 * 64
    out = tuple(torch.full((b.size + pad,), -21846, dtype=torch.int16, device=dev) for b in want)  # 0xaaaa
    hp.forward_rgb_blocks(to_dev(rgb, dev), subsampling=sub, out=out)
    for o, b, name in zip(out, want, "y cb cr".split()):
        got = to_host(o)
        assert np.array_equal(got[:b.size].reshape(-1, 64), b), name
        assert (got[b.size:] == -21846).all(), name
    px = torch.full((h + 8, w, 3), 0xa5, dtype=torch.uint8, device=dev)
    b = [to_dev(x, dev) for x in want]
    hp.inverse_rgb_blocks(*b, subsampling=sub, out=px, height=h, width=w)
    got = to_host(px)
    assert np.array_equal(got[:h], back)
    assert (got[h:] == 0xa5).all()


@pytest.mark.parametrize("sub,shape", [("444", (16, 264)), ("420", (32, 528))], ids=["444", "420"])
def test_stacked_frames(hp, oracle, dev, sub, shape):
    """A (2, H, W, 3) stack is the (2H, W, 3) image: each frame's blocks contiguous in all three arrays."""
    h, w = shape
    frames = oracle.rand_u8(2 * 3 * h * w, 9).reshape(2, h, w, 3)
    x = to_dev(frames, dev)
    whole = [to_host(t) for t in hp.forward_rgb_blocks(x, subsampling=sub)]
    singles = [[to_host(t) for t in hp.forward_rgb_blocks(x[f], subsampling=sub)] for f in range(2)]
    for c in range(3):
        assert whole[c].shape[0] == 2 * singles[0][c].shape[0]
        assert np.array_equal(whole[c], np.concatenate([singles[0][c], singles[1][c]], axis=0))


@pytest.mark.parametrize("sub,shape", [("444", (64, 512)), ("420", (128, 1024))], ids=["444", "420"])
def test_mapping_does_not_affect_colour(hp, oracle, dev, zz, sub, shape):
    rgb, coefs, back = _case(oracle, sub, shape, "default")
    want = blocks_of(coefs, zz, "zigzag", shape3=True)
    hp.set_mapping("octet")
    try:
        got = [to_host(t) for t in hp.forward_rgb_blocks(to_dev(rgb, dev), subsampling=sub)]
        rec = to_host(hp.inverse_rgb_blocks(*[to_dev(b, dev) for b in want], subsampling=sub))
    finally:
        hp.set_mapping("auto")
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.array_equal(rec, back)


@pytest.mark.parametrize("sub,shape", [("444", (24, 1016)), ("420", (48, 2032))], ids=["444", "420"])
def test_library_table_is_the_luma_default_only(hp, oracle, dev, zz, sub, shape):
    """hpdct_set_quant_table(x) changes d_y when q_luma is NULL and leaves d_cb, d_cr alone."""
    rgb, coefs, _ = _case(oracle, sub, shape, "default")
    x = to_dev(rgb, dev)
    base = [to_host(t) for t in hp.forward_rgb_blocks(x, subsampling=sub)]
    (ql75, _), _ = _tables(oracle, "q75")
    hp.set_quant_table(ql75)
    try:
        got = [to_host(t) for t in hp.forward_rgb_blocks(x, subsampling=sub)]
        rec = to_host(hp.inverse_rgb_blocks(*[to_dev(g, dev) for g in got], subsampling=sub))
    finally:
        hp.set_quant_table(None)
    y75 = oracle.fdct(planes_of(rgb, sub)[0], Q=ql75)
    assert np.array_equal(got[0].reshape(-1, 64), _to_blocks(y75, zz, "zigzag").astype(np.int16))
    assert not np.array_equal(got[0], base[0])
    assert np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2])
    # the inverse reads the library table the same way
    assert np.array_equal(rec, ref_inverse(oracle, (y75, coefs[1], coefs[2]), sub, ql75, CHROMA_K))


def test_byte_offsets_past_4_gib(hp, oracle, dev, zz):
    """A 32 x 89,478,496 4:2:0 frame: 8.6e9 bytes of RGB and 5.7e9 bytes of Y blocks, so every byte offset of
    the second MCU row is past 2^32.  Checked on the first and last 65 MCUs of both MCU rows (tiles are
    independent, so a crop's reference is the crop of the reference); 5,592,406 MCUs per row, so sets straddle."""
    import torch
    h, w, crop = 32, 16 * 5592406, 1040
    assert 3 * h * w > 2 ** 33 and (h * w * 2) > 2 ** 32
    rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    hp.fill_hash_u8(rgb, seed=11)
    y, cb, cr = hp.forward_rgb_blocks(rgb, subsampling="420")
    back = hp.inverse_rgb_blocks(y, cb, cr, subsampling="420")
    (ql, qc), _ = _tables(oracle, "default")
    for x0 in (0, w - crop):
        part = to_host(rgb[:, x0:x0 + crop]).copy()
        coefs = ref_forward(oracle, part, "420", ql, qc)
        want = blocks_of(coefs, zz, "zigzag", shape3=True)
        got = (y[:, x0 // 8:(x0 + crop) // 8], cb[:, x0 // 16:(x0 + crop) // 16], cr[:, x0 // 16:(x0 + crop) // 16])
        for g, wb, name in zip(got, want, "y cb cr".split()):
            assert np.array_equal(to_host(g), wb), (x0, name)
        assert np.array_equal(to_host(back[:, x0:x0 + crop]), ref_inverse(oracle, coefs, "420", ql, qc)), x0
