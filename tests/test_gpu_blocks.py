"""JPEG-style int16 coefficient blocks on the GPU (hpdct_forward_blocks /
hpdct_inverse_blocks): exact equality with the CPU oracle everywhere, no
tolerance.

Reference: the oracle's quantised plane, regrouped per tile, reordered and cast
to int16 (the values are integers; the oracle's -0.0 becomes 0).  The inverse is
checked on the reference blocks against oracle.idct of that plane, bit for bit.

Shapes (the smallest that reach each path of the kernels):
  8x8       one live lane
  8x520     65 tiles: a whole 64-tile set plus a one-tile ragged set
  16x264    33 tiles per row: a set spanning two tile rows on the pixel side
  24x1016   381 tiles: sets straddling tile rows and a ragged last set
  64x512    8 whole sets: the LDS-staged block stores
  512x1024  128 waves, many workgroups
"""
import numpy as np
import pytest

from test_gpu_parity import _hardest_tiles, bits_equal, to_dev, to_host

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (8, 520), (16, 264), (24, 1016), (64, 512), (512, 1024)]
TABLES = ["default", "q75", "x0.37"]
ORDERS = ["zigzag", "natural"]


def _table(oracle, name):
    q = oracle.default_quant().astype(np.float32)
    if name == "default":
        return None                                             # the JPEG forms (qmode 2)
    if name == "q75":
        return np.floor((q * 50 + 50) / 100).astype(np.float32)  # libjpeg quality 75: integers, DC 8 (qmode 1)
    if name == "x0.37":
        return (q * np.float32(0.37)).astype(np.float32)         # not integers: IEEE division
    if name == "ones":
        return np.ones((8, 8), np.float32)
    raise KeyError(name)


def _to_blocks(plane, zz, order):
    """The spatial plane's tiles as (ntiles, 64) in row-major tile order."""
    h, w = plane.shape
    b = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    return b[:, zz] if order == "zigzag" else b


_cache = {}


def _case(oracle, shape, table):
    """(image, quantised fp32 plane) of a shape under a table, computed once."""
    key = (shape, table)
    if key not in _cache:
        h, w = shape
        img = oracle.rand_u8(h * w, 42).reshape(h, w)
        _cache[key] = (img, oracle.fdct(img, Q=_table(oracle, table)))  # shared: never written to
    return _cache[key]


@pytest.fixture(scope="module")
def zz(hp):
    return hp.zigzag_order().astype(np.int64)


@pytest.fixture()
def use_table(hp, oracle):
    """Sets the library's table for one test and restores the default after it."""
    def set_(name):
        hp.set_quant_table(_table(oracle, name))
    yield set_
    hp.set_quant_table(None)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_forward_blocks_match_oracle(hp, oracle, dev, zz, use_table, shape, table, order):
    import torch
    img, ref = _case(oracle, shape, table)
    want = _to_blocks(ref, zz, order).astype(np.int16)
    use_table(table)
    x = to_dev(img, dev)
    if table == "q75":
        # the int8 wire format refuses this ordinary table; the int16 blocks take it
        with pytest.raises(hp.HpdctError) as e:
            hp.forward(x, out_dtype=torch.int8)
        assert e.value.status == 3
    got = hp.forward_blocks(x, order=order)
    assert got.dtype == torch.int16 and tuple(got.shape) == (shape[0] // 8, shape[1] // 8, 64)
    got = to_host(got).reshape(-1, 64)
    bad = int((got != want).sum())
    print("forward_blocks %s %s %s: %d of %d values differ" % (shape, table, order, bad, want.size))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_inverse_blocks_match_oracle(hp, oracle, dev, zz, use_table, shape, table, order):
    import torch
    _, ref = _case(oracle, shape, table)
    blocks = np.ascontiguousarray(_to_blocks(ref, zz, order).astype(np.int16))
    rec = oracle.idct(np.array(ref), Q=_table(oracle, table))
    use_table(table)
    b = to_dev(blocks.reshape(shape[0] // 8, shape[1] // 8, 64), dev)
    got32 = to_host(hp.inverse_blocks(b, order=order))
    assert got32.shape == shape and got32.dtype == np.float32
    print("inverse_blocks %s %s %s: %d fp32 pixels differ" %
          (shape, table, order, int((got32.view(np.uint32) != rec.view(np.uint32)).sum())))
    assert bits_equal(got32, rec)
    got8 = to_host(hp.inverse_blocks(b, out_dtype=torch.uint8, order=order))
    assert got8.dtype == np.uint8 and np.array_equal(got8, oracle.to_u8(rec))
    # a flat block buffer with the shape passed in
    flat = to_host(hp.inverse_blocks(b.reshape(-1), order=order, height=shape[0], width=shape[1]))
    assert bits_equal(flat, rec)


def test_extremes_beyond_int8(hp, oracle, dev, zz, use_table):
    """A flat 0 tile, a flat 255 tile and a per-pixel 0/255 checkerboard under
    an all-ones table: quotients of -1024 and 1016 survive in int16."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (24, 24), dtype=np.uint8)
    img[0:8, 0:8] = 0
    img[0:8, 8:16] = 255
    yy, xx = np.mgrid[0:8, 0:8]
    img[8:16, 16:24] = np.where((yy + xx) % 2 == 0, 0, 255)
    ref = oracle.fdct(img, Q=_table(oracle, "ones"))
    assert ref.min() == -1024 and 1016 in ref        # beyond int8: what the oracle gives
    use_table("ones")
    for order in ORDERS:
        want = _to_blocks(ref, zz, order).astype(np.int16)
        got = to_host(hp.forward_blocks(to_dev(img, dev), order=order)).reshape(-1, 64)
        assert np.array_equal(got, want), order
        assert got.min() == -1024 and (got == 1016).any()
        back = to_host(hp.inverse_blocks(to_dev(want.reshape(3, 3, 64), dev), order=order))
        assert bits_equal(back, oracle.idct(ref, Q=_table(oracle, "ones")))


@pytest.fixture(scope="module")
def hardest(oracle):
    img = _hardest_tiles(oracle)
    return img, oracle.fdct(img)


def test_hardest_tiles(hp, oracle, dev, zz, hardest):
    """The tiles nearest a rounding boundary of the default table at every
    position, and each position's extreme tiles: the quantiser forms behind the
    int16 convert are those of the fp32 forward."""
    img, ref = hardest
    x = to_dev(img, dev)
    for order in ORDERS:
        want = _to_blocks(ref, zz, order).astype(np.int16)
        got = to_host(hp.forward_blocks(x, order=order)).reshape(-1, 64)
        print("hardest tiles %s: %d of %d values differ" % (order, int((got != want).sum()), want.size))
        assert np.array_equal(got, want), order


def test_round_trip_equals_the_plane_path(hp, oracle, dev):
    import torch
    img, _ = _case(oracle, (24, 1016), "default")
    x = to_dev(img, dev)
    coef = hp.forward(x)
    for order in ORDERS:
        b = hp.forward_blocks(x, order=order)
        assert bits_equal(to_host(hp.inverse_blocks(b, order=order)), to_host(hp.inverse(coef)))
        assert np.array_equal(to_host(hp.inverse_blocks(b, out_dtype=torch.uint8, order=order)),
                              to_host(hp.inverse(coef, out_dtype=torch.uint8)))


def test_natural_order_is_the_zigzag_unscrambled(hp, oracle, dev, zz):
    img, _ = _case(oracle, (24, 1016), "default")
    x = to_dev(img, dev)
    nat = to_host(hp.forward_blocks(x, order="natural"))
    zig = to_host(hp.forward_blocks(x, order="zigzag"))
    assert np.array_equal(nat[:, :, zz], zig)


def test_stacked_frames(hp, oracle, dev):
    """A (3, 16, 264) stack is the (48, 264) image: each frame's blocks contiguous."""
    frames = oracle.rand_u8(3 * 16 * 264, 9).reshape(3, 16, 264)
    x = to_dev(frames, dev)
    whole = to_host(hp.forward_blocks(x))
    assert whole.shape == (6, 33, 64)
    singles = [to_host(hp.forward_blocks(x[f])) for f in range(3)]
    assert all(s.shape == (2, 33, 64) for s in singles)
    assert np.array_equal(whole, np.concatenate(singles, axis=0))


@pytest.mark.parametrize("shape", [(8, 520), (24, 1016), (64, 512)], ids=lambda s: "%dx%d" % s)
def test_memory_beyond_the_frame_is_untouched(hp, oracle, dev, zz, shape):
    import torch
    h, w = shape
    img, ref = _case(oracle, shape, "default")
    want = _to_blocks(ref, zz, "zigzag").astype(np.int16)
    n, pad = h * w, 64 * 64
    out = torch.full((n + pad,), -21846, dtype=torch.int16, device=dev)  # 0xaaaa
    hp.forward_blocks(to_dev(img, dev), out=out)
    got = to_host(out)
    assert np.array_equal(got[:n].reshape(-1, 64), want)
    assert (got[n:] == -21846).all()
    # the inverse's pixel buffer has 8 more rows than the frame
    b = to_dev(want, dev)
    for dt, sentinel in ((torch.float32, -7.5), (torch.uint8, 0xa5)):
        px = torch.full((h + 8, w), sentinel, dtype=dt, device=dev)
        hp.inverse_blocks(b, out=px, height=h, width=w)
        got = to_host(px)
        assert (got[h:] == sentinel).all(), dt
        assert np.array_equal(got[:h], to_host(hp.inverse_blocks(b, out_dtype=dt, height=h, width=w))), dt


def test_mapping_does_not_affect_blocks(hp, oracle, dev, zz):
    img, ref = _case(oracle, (64, 512), "default")
    want = _to_blocks(ref, zz, "zigzag").astype(np.int16)
    rec = oracle.idct(np.array(ref))
    x = to_dev(img, dev)
    hp.set_mapping("octet")
    try:
        got = to_host(hp.forward_blocks(x)).reshape(-1, 64)
        back = to_host(hp.inverse_blocks(to_dev(want.reshape(8, 64, 64), dev)))
    finally:
        hp.set_mapping("auto")
    assert np.array_equal(got, want)
    assert bits_equal(back, rec)
