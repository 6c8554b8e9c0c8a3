"""GPU tests of the entropy coder (hpdct_encode_scan): byte for byte against
the plain-Python restatement of the coding in tests/jpeg_scan.py (which
tests/test_jpeg_scan_host.py checks against an independent decoder and Pillow),
no tolerance: the scan bytes, hpdct_scan_info and every interval offset.
"""
import numpy as np
import pytest

import decoder_blocks
import jpeg_scan as J

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xA5

_memo = {}


def _expected(key, components, sampling, ri):
    """jpeg_scan.encode, computed once per input and interval."""
    k = (key, sampling, ri)
    if k not in _memo:
        _memo[k] = J.encode(components, sampling, ri)
    return _memo[k]


def _natural(zz_blocks):
    nat = np.zeros_like(zz_blocks)
    nat[..., J.ZIGZAG] = zz_blocks
    return nat


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_scan(hp, dev, key, components, sampling, ri, order="zigzag"):
    """One call through encode_scan against the restatement: bytes, info, offsets."""
    want, want_offs = _expected(key, components, sampling, ri)
    arrays = [_dev(c if order == "zigzag" else _natural(c), dev) for c in components]
    h, w = 8 * components[0].shape[0], 8 * components[0].shape[1]
    sub = "444" if sampling == "grey" else sampling
    scan, info, offs = hp.encode_scan(*arrays, height=h, width=w, subsampling=sub, restart_interval=ri, order=order)
    assert info == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
    got = scan.cpu().numpy().tobytes()
    if got != want:
        first = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else -1
        raise AssertionError("scan differs: %d bytes against %d, first difference at %d" % (len(got), len(want), first))
    assert offs.cpu().numpy().tolist() == want_offs
    blocks = sum(c.shape[0] * c.shape[1] for c in components)
    assert len(want) <= hp.scan_bound(blocks, len(want_offs) - 1)


# ---------------------------------------------------------------------------
# grey
# ---------------------------------------------------------------------------
GREY_SHAPES = [(8, 8), (8, 520), (24, 1016), (64, 512)]
INTERVALS = [0, 1, 5, 64, 127, 65535]


def _q75(oracle):
    return np.floor((oracle.default_quant().reshape(8, 8) * 50 + 50) / 100).astype(np.float32)


def _forward_blocks(hp, oracle, dev, shape, table):
    """forward_blocks of the rand_u8 frame under the default or the quality-75 table, on the host, zig-zag."""
    k = ("fwd", shape, table)
    if k not in _memo:
        h, w = shape
        img = oracle.rand_u8(h * w, 42).reshape(h, w)
        hp.set_quant_table(_q75(oracle) if table == "q75" else None)
        try:
            _memo[k] = hp.forward_blocks(_dev(img, dev)).cpu().numpy()
            nat = hp.forward_blocks(_dev(img, dev), order="natural").cpu().numpy()
        finally:
            hp.set_quant_table(None)
        assert np.array_equal(_natural(_memo[k]), nat)
    return _memo[k]


@pytest.mark.parametrize("ri", INTERVALS)
@pytest.mark.parametrize("shape", GREY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_grey_forward_blocks(hp, oracle, dev, shape, ri):
    for table in ("default", "q75"):
        blocks = _forward_blocks(hp, oracle, dev, shape, table)
        for order in ("zigzag", "natural"):
            _check_scan(hp, dev, ("fwd", shape, table), [blocks], "grey", ri, order)


def _catalogue(oracle, clip=True):
    cat, _ = decoder_blocks.catalogue(oracle.default_transform())
    x = cat[:decoder_blocks.FIRST]
    if clip:
        x = np.clip(x, -1023, 1023)
    return np.ascontiguousarray(x[:, J.ZIGZAG].reshape(3, 127, 64))


@pytest.mark.parametrize("order", ["zigzag", "natural"])
@pytest.mark.parametrize("ri", INTERVALS)
def test_grey_catalogue(hp, oracle, dev, ri, order):
    """The clipped catalogue in a 24 x 1016 frame: dense +-1023 blocks (the longest codes, 0xFF runs), ZRL runs,
    blocks without EOB, the all-zero block."""
    _check_scan(hp, dev, "catalogue", [_catalogue(oracle)], "grey", ri, order)


# ---------------------------------------------------------------------------
# colour
# ---------------------------------------------------------------------------
COLOUR_SHAPES = {"420": [(16, 16), (16, 176), (48, 80)], "444": [(8, 8), (8, 176), (24, 40)]}


def _colour_catalogue(oracle, sampling, shape):
    """Clipped catalogue blocks, taken cyclically, as the three arrays of a frame."""
    h, w = shape
    f = 2 if sampling == "420" else 1
    T = oracle.default_transform()
    sizes = [(h // 8, w // 8), (h // 8 // f, w // 8 // f), (h // 8 // f, w // 8 // f)]
    out, offset = [], 0
    for ty, tx in sizes:
        b = np.clip(decoder_blocks.take(T, ty * tx, offset), -1023, 1023)[:, J.ZIGZAG]
        out.append(np.ascontiguousarray(b.reshape(ty, tx, 64)))
        offset += ty * tx
    return out


@pytest.mark.parametrize("ri", [0, 1, 3, "row"])
@pytest.mark.parametrize("sampling,shape", [(s, sh) for s in ("420", "444") for sh in COLOUR_SHAPES[s]],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_colour_catalogue(hp, oracle, dev, sampling, shape, ri):
    if ri == "row":
        ri = shape[1] // (16 if sampling == "420" else 8)
    comps = _colour_catalogue(oracle, sampling, shape)
    for order in ("zigzag", "natural"):
        _check_scan(hp, dev, ("colour", shape), comps, sampling, ri, order)


def _rgb_frame(oracle):
    return oracle.rand_u8(45 * 77 * 3, 21).reshape(45, 77, 3)


@pytest.mark.parametrize("ri", [0, 1, 3, "row"])
@pytest.mark.parametrize("sampling", ["420", "444"])
def test_colour_forward_rgb_frame(hp, oracle, dev, sampling, ri):
    """What forward_rgb_frame writes for a 45 x 77 frame (padded to 48 x 80), coded as it lies on the device."""
    rgb = _dev(_rgb_frame(oracle), dev)
    y, cb, cr = hp.forward_rgb_frame(rgb, subsampling=sampling)
    comps = [t.cpu().numpy() for t in (y, cb, cr)]
    if ri == "row":
        ri = 80 // (16 if sampling == "420" else 8)
    want, want_offs = J.encode(comps, sampling, ri)
    scan, info, offs = hp.encode_scan(y, cb, cr, height=48, width=80, subsampling=sampling, restart_interval=ri)
    assert info == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
    assert scan.cpu().numpy().tobytes() == want
    assert offs.cpu().numpy().tolist() == want_offs


# ---------------------------------------------------------------------------
# capacity, range, graph capture
# ---------------------------------------------------------------------------
def _buffers(hp, dev, blocks_dev, h, w, ri, capacity, cb=None, cr=None, sub="444"):
    import torch
    nmcu = (h // 8) * (w // 8) if cb is None or sub == "444" else (h // 16) * (w // 16)
    intervals = 1 if ri == 0 else -(-nmcu // ri)
    buf = torch.full((capacity + GUARD,), FILL, dtype=torch.uint8, device=dev)
    info = torch.full((2,), -1, dtype=torch.int64, device=dev)
    offs = torch.full((intervals + 1,), -1, dtype=torch.int64, device=dev)
    comps = 1 if cb is None else 3
    ws = torch.empty(hp.load_library().hpdct_scan_workspace_bytes(h, w, comps, hp.SUBSAMPLINGS[sub], ri),
                     dtype=torch.uint8, device=dev)
    call = hp.bind_scan(blocks_dev, cb, cr, buf, info, offs, ws, height=h, width=w, subsampling=sub,
                        restart_interval=ri, capacity=capacity)
    return call, buf, info, offs, ws


@pytest.mark.parametrize("ri", [0, 5, 127])
def test_capacity_is_respected(hp, oracle, dev, ri):
    x = _catalogue(oracle)
    want, want_offs = _expected("catalogue", [x], "grey", ri)
    xd = _dev(x, dev)
    # one byte short: truncated, the size it needs, nothing past the capacity
    call, buf, info, offs, _ = _buffers(hp, dev, xd, 24, 1016, ri, len(want) - 1)
    call()
    assert hp.scan_info(info) == {"bytes": len(want), "truncated": 1, "out_of_range": 0}
    assert bool((buf[len(want) - 1:] == FILL).all())
    assert offs.cpu().numpy().tolist() == want_offs
    # exactly enough: the scan, and the guard untouched
    call, buf, info, offs, _ = _buffers(hp, dev, xd, 24, 1016, ri, len(want))
    call()
    assert hp.scan_info(info) == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
    assert buf[:len(want)].cpu().numpy().tobytes() == want
    assert bool((buf[len(want):] == FILL).all())
    assert offs.cpu().numpy().tolist() == want_offs


def test_capacity_with_out_given(hp, oracle, dev):
    """encode_scan(out=...): a buffer that is too small comes back empty with the size needed."""
    import torch
    x = _catalogue(oracle)
    want, _ = _expected("catalogue", [x], "grey", 127)
    small = torch.full((len(want) - 1,), FILL, dtype=torch.uint8, device=dev)
    scan, info, _ = hp.encode_scan(_dev(x, dev), restart_interval=127, out=small)
    assert scan.numel() == 0 and info["truncated"] == 1 and info["bytes"] == len(want)
    fits = torch.full((len(want) + 100,), FILL, dtype=torch.uint8, device=dev)
    scan, info, _ = hp.encode_scan(_dev(x, dev), restart_interval=127, out=fits)
    assert scan.cpu().numpy().tobytes() == want and scan.data_ptr() == fits.data_ptr()
    assert bool((fits[len(want):] == FILL).all())


@pytest.mark.parametrize("capacity", ["bound", 1000])
@pytest.mark.parametrize("ri", [0, 5, 127])
def test_out_of_range_is_counted_and_safe(hp, oracle, dev, ri, capacity):
    """The unclipped catalogue (+-32767): the count of the restatement, a length within the bound, and no
    byte at or past the capacity, whether the scan fits it or not."""
    raw = _catalogue(oracle, clip=False)
    intervals = 1 if ri == 0 else -(-381 // ri)
    bound = hp.scan_bound(381, intervals)
    cap = bound if capacity == "bound" else capacity
    call, buf, info, offs, _ = _buffers(hp, dev, _dev(raw, dev), 24, 1016, ri, cap)
    call()
    res = hp.scan_info(info)
    assert res["out_of_range"] == J.out_of_range([raw], "grey", ri) > 0
    assert 0 < res["bytes"] <= bound
    assert res["truncated"] == int(res["bytes"] > cap)
    assert bool((buf[cap:] == FILL).all())
    o = offs.cpu().numpy()
    assert o[0] == 0 and o[-1] == res["bytes"] and bool((np.diff(o) > 0).all())


def test_graph_capture_and_replay(hp, oracle, dev):
    """One bind_scan launch captured in a graph (three kernels, one chain, no allocation) and replayed twice."""
    import torch
    x = _catalogue(oracle)
    want, want_offs = _expected("catalogue", [x], "grey", 127)
    xd = _dev(x, dev)
    call, buf, info, offs, ws = _buffers(hp, dev, xd, 24, 1016, 127, len(want))
    call()                                          # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            hp.bind_scan(xd, None, None, buf, info, offs, ws, height=24, width=1016, restart_interval=127,
                         capacity=len(want))()
    torch.cuda.synchronize()
    for _ in range(2):
        buf.fill_(FILL)
        info.fill_(-1)
        offs.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert hp.scan_info(info) == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
        assert buf[:len(want)].cpu().numpy().tobytes() == want
        assert bool((buf[len(want):] == FILL).all())
        assert offs.cpu().numpy().tolist() == want_offs


# ---------------------------------------------------------------------------
# the whole file
# ---------------------------------------------------------------------------
def test_jpeg_encode_grey(hp, oracle, dev):
    img = oracle.rand_u8(64 * 512, 42).reshape(64, 512)
    x = _dev(img, dev)
    blocks = hp.forward_blocks(x).cpu().numpy()
    got = hp.jpeg_encode(x)
    scan, _ = J.encode([blocks], "grey", 64)                               # one MCU row per interval
    assert got == hp.jpeg_header(64, 512, components=1, restart_interval=64) + scan + b"\xff\xd9"
    scan, _ = J.encode([blocks], "grey", 0)
    assert hp.jpeg_encode(x, restart_interval=0) == hp.jpeg_header(64, 512, components=1) + scan + b"\xff\xd9"


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_jpeg_encode_rgb(hp, oracle, dev, sampling):
    rgb = _dev(_rgb_frame(oracle), dev)
    comps = [t.cpu().numpy() for t in hp.forward_rgb_frame(rgb, subsampling=sampling)]
    ri = 80 // (16 if sampling == "420" else 8)
    scan, _ = J.encode(comps, sampling, ri)
    got = hp.jpeg_encode(rgb, subsampling=sampling)
    assert got == hp.jpeg_header(45, 77, components=3, subsampling=sampling, restart_interval=ri) + scan + b"\xff\xd9"
    # the file opens in an outside decoder, where there is one, at its true size
    try:
        from PIL import Image
    except ImportError:
        return
    import io
    im = Image.open(io.BytesIO(got))
    assert im.size == (77, 45) and np.asarray(im).shape == (45, 77, 3)
