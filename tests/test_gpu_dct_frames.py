"""The exact DCT on the frame and JPEG path (HPDCT_FRAME_DCT, transform="dct") on the GPU: exact equality with
the oracle everywhere; the only tolerances are against Pillow's own decoder and are derived below.

Reference, with Td = hp.dct_transform():
  forward  blocks_of(oracle.fdct(padded(frame), T=Td, Q=q)): the unflagged contract with the matrix replaced;
  inverse  oracle.to_u8(oracle.idct(c, T=Td, Q=q, shift=False) + np.float32(128.5)), cropped: every term of the
           chains, then one fp32 add, clamp and truncate (round half up);
  colour   test_gpu_rgb.planes_of / rgb_of around the two expressions, per component plane.
Every forward test also asserts that its reference differs from the T=None one, so a kernel that ignores the flag
cannot pass (but for the 1x1 frames: one pixel replicated is a constant tile, DC only, and row 0 of the two matrices
is the same).

Shapes are the ones of test_gpu_grey_frame.py and test_gpu_rgb_frame.py (each docstring says which mechanism a
shape reaches).  Inverse inputs: the forward's coefficients; under "q75" also seeded random int16 in [-1023, 1023]
(DC in [-2047, 2047]), decoder input the forward never makes; "huge" (one table entry of 2e34) on one shape, where
q * Q is infinite and the reference gives NaN and Inf.

Against Pillow (test 5 and 6): Pillow's pixels lie within 1.0 of the float64 IDCT (test_jpeg_unscan_host.py
asserts it) and ours are that IDCT's rounding up to fp32 error, so a grey pixel differs by at most 1; a 4:4:4
pixel by at most 3: +-1 per component through the conversion's largest gain, 1.772, plus its rounding.  The 4:2:0
difference is Pillow's smooth chroma upsampling, which the library does not do: printed, not asserted.
"""
import io
import os

import numpy as np
import pytest

import jpeg_scan as J
import jpeg_unscan as U
from test_gpu_grey_frame import (assert_only_the_frame_written, blocks_on_device, frame_buffer, frame_on_device,
                                 padded, table_of)
from test_gpu_parity import to_dev, to_host
from test_gpu_rgb import TABLES, _tables, blocks_of, planes_of, rgb_of
import test_gpu_rgb_frame as RF

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORDERS = ["zigzag", "natural"]
# (height, width, pitch - width, base offset)
GREY_SHAPES = [(1, 1, 0, 0), (7, 9, 0, 0), (13, 515, 0, 0), (13, 515, 5, 0), (17, 512, 0, 0), (24, 1016, 40, 0),
               (24, 1016, 0, 3)]
GREY_ALL_TABLES = {(13, 515, 0, 0), (17, 512, 0, 0)}
GREY_CASES = [(s, t) for s in GREY_SHAPES for t in (TABLES if s in GREY_ALL_TABLES else TABLES[:1])]
GREY_IDS = ["%dx%d+%d@%d-%s" % (s + (t,)) for s, t in GREY_CASES]
# the inverse's extra inputs: (shape, table, input kind)
INV_CASES = ([(s, t, "forward") for s, t in GREY_CASES] +
             [(s, "q75", "random") for s in sorted(GREY_ALL_TABLES)] + [((13, 515, 0, 0), "huge", "huge")])
INV_IDS = ["%dx%d+%d@%d-%s-%s" % (s + (t, k)) for s, t, k in INV_CASES]
RGB_ALL_TABLES = {("444", 13, 515, 0), ("420", 18, 1030, 0)}
RGB_CASES = [(s, t) for s in RF.SHAPES for t in (TABLES if s in RGB_ALL_TABLES else TABLES[:1])]
RGB_IDS = ["%s-%dx%d+%d-%s" % (s + (t,)) for s, t in RGB_CASES]


@pytest.fixture(scope="module")
def zz(hp):
    return hp.zigzag_order().astype(np.int64)


@pytest.fixture(scope="module")
def Td(hp):
    return hp.dct_transform()


def inverse_plane(oracle, Td, coefs, q):
    """The inverse contract for one component plane of coefficients: uint8 pixels of the padded plane."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = oracle.idct(np.array(coefs, np.float32), T=Td, Q=q, shift=False)
        return oracle.to_u8(r + np.float32(128.5))


_cache = {}


def grey_case(oracle, Td, h, w, table, kind="forward"):
    """(frame, reference coefficients of the padded frame, the inverse's input plane, reference pixels of its
    inverse cropped to the frame), computed once and never written to."""
    key = ("grey", h, w, table, kind)
    if key not in _cache:
        frame = oracle.rand_u8(h * w, 42).reshape(h, w)
        q, _ = table_of(oracle, table)
        coefs = oracle.fdct(padded(frame), T=Td, Q=q)
        # (one pixel replicated is a constant tile: DC only, and the two matrices share row 0)
        assert (h, w) == (1, 1) or not np.array_equal(coefs, oracle.fdct(padded(frame), Q=q)), "a blind case"
        inp = coefs
        if kind == "random":
            rng = np.random.default_rng(1234 + h * w)
            inp = rng.integers(-1023, 1024, coefs.shape).astype(np.float32)
            inp[0::8, 0::8] = rng.integers(-2047, 2048, inp[0::8, 0::8].shape)
        elif kind == "huge":
            inp = coefs.copy()
            inp[0::8, 1::16] = 30000.0
            inp[0::8, 9::16] = -32768.0
        back = inverse_plane(oracle, Td, inp, q)[:h, :w]
        if kind == "huge":
            with np.errstate(over="ignore", invalid="ignore"):
                assert not np.isfinite(oracle.idct(np.array(inp), T=Td, Q=q, shift=False)).all()
        for a in (frame, coefs, inp, back):
            a.setflags(write=False)
        _cache[key] = (frame, coefs, inp, back)
    return _cache[key]


def rgb_case(oracle, Td, sub, h, w, table):
    """(rgb, reference coefficient planes of the padded frame, reference RGB of their inverse cropped)."""
    key = ("rgb", sub, h, w, table)
    if key not in _cache:
        rgb = oracle.rand_u8(3 * h * w, 42).reshape(h, w, 3)
        (ql, qc), _ = _tables(oracle, table)
        planes = planes_of(RF.padded(rgb, sub), sub)
        coefs = tuple(oracle.fdct(p, T=Td, Q=q) for p, q in zip(planes, (ql, qc, qc)))
        assert (h, w) == (1, 1) or not np.array_equal(coefs[0], oracle.fdct(planes[0], Q=ql)), "a blind case"
        back = rgb_of(*(inverse_plane(oracle, Td, c, q) for c, q in zip(coefs, (ql, qc, qc))), sub)[:h, :w]
        for a in (rgb, back) + coefs:
            a.setflags(write=False)
        _cache[key] = (rgb, coefs, back)
    return _cache[key]


# ---------------------------------------------------------------------------
# 1, 2: grey frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape,table", GREY_CASES, ids=GREY_IDS)
def test_grey_forward_matches_reference(hp, oracle, dev, zz, Td, shape, table, order):
    import torch
    h, w, extra, offset = shape
    frame, coefs, _, _ = grey_case(oracle, Td, h, w, table)
    x = frame_on_device(dev, frame, w + extra, offset)
    assert x.data_ptr() % 8 == offset
    want = blocks_of([coefs], zz, order)[0]
    out = torch.full((want.size + 64 * 64,), -21846, dtype=torch.int16, device=dev)  # 0xaaaa behind the blocks
    got = hp.forward_grey_frame(x, q=table_of(oracle, table)[1], order=order, out=out, transform="dct")
    assert got is out
    host = to_host(out)
    print("grey forward %s %s %s: %d values differ" % (shape, table, order,
                                                       int((host[:want.size].reshape(-1, 64) != want).sum())))
    assert np.array_equal(host[:want.size].reshape(-1, 64), want)
    assert (host[want.size:] == -21846).all()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape,table,kind", INV_CASES, ids=INV_IDS)
def test_grey_inverse_matches_reference(hp, oracle, dev, zz, Td, shape, table, kind, order):
    h, w, extra, offset = shape
    _, _, inp, want = grey_case(oracle, Td, h, w, table, kind)
    b = blocks_on_device(dev, zz, inp, order)
    buf, out = frame_buffer(dev, h, w, w + extra, offset)
    got = hp.inverse_grey_frame(b, height=h, width=w, q=table_of(oracle, table)[1], order=order, out=out,
                                transform="dct")
    assert got is out
    assert_only_the_frame_written(buf, h, w, w + extra, offset, want)


# ---------------------------------------------------------------------------
# 3: colour frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape,table", RGB_CASES, ids=RGB_IDS)
def test_rgb_forward_matches_reference(hp, oracle, dev, zz, Td, shape, table, order):
    sub, h, w, extra = shape
    rgb, coefs, _ = rgb_case(oracle, Td, sub, h, w, table)
    _, (ql, qc) = _tables(oracle, table)
    x = RF.frame_on_device(dev, rgb, 3 * w + extra)
    got = hp.forward_rgb_frame(x, subsampling=sub, q_luma=ql, q_chroma=qc, order=order, transform="dct")
    assert [tuple(g.shape) for g in got] == RF.block_shapes(h, w, sub)
    RF.assert_blocks(got, blocks_of(coefs, zz, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape,table", RGB_CASES, ids=RGB_IDS)
def test_rgb_inverse_matches_reference(hp, oracle, dev, zz, Td, shape, table, order):
    sub, h, w, extra = shape
    _, coefs, want = rgb_case(oracle, Td, sub, h, w, table)
    _, (ql, qc) = _tables(oracle, table)
    y, cb, cr = (to_dev(b, dev) for b in blocks_of(coefs, zz, order, shape3=True))
    buf, out = RF.frame_buffer(dev, h, w, 3 * w + extra)
    got = hp.inverse_rgb_frame(y, cb, cr, height=h, width=w, subsampling=sub, q_luma=ql, q_chroma=qc, order=order,
                               out=out, transform="dct")
    assert got is out
    RF.assert_only_the_frame_written(buf, h, w, 3 * w + extra, 0, want)


# ---------------------------------------------------------------------------
# 4: the two transforms at once
# ---------------------------------------------------------------------------
def test_two_transforms_on_two_streams_at_once(hp, oracle, dev, zz, Td):
    """The same frame forward and the same blocks inverse, without the flag on one stream and with it on the
    other, interleaved: each result equals its own reference (the transform travels with the launch)."""
    import torch
    import test_gpu_grey_frame as GF
    h, w = 13, 515
    names = ("hpappr", "dct")
    frame, coefs_d, _, back_d = grey_case(oracle, Td, h, w, "q75")
    _, coefs_h, _, _ = GF._case(oracle, h, w, "q75")
    qref, q = table_of(oracle, "q75")
    # both inverses read the DCT forward's blocks: each transform gives them its own pixels
    back_h = oracle.to_u8(oracle.idct(np.array(coefs_d), Q=qref))[:h, :w]
    assert not np.array_equal(back_h, back_d)
    streams = [torch.cuda.Stream(device=dev) for _ in names]
    x = frame_on_device(dev, frame, 520)
    fwd_out = [torch.zeros((2, 65, 64), dtype=torch.int16, device=dev) for _ in names]
    inv_in = blocks_on_device(dev, zz, coefs_d, "zigzag")
    inv_buf = [frame_buffer(dev, h, w, 520) for _ in names]
    torch.cuda.synchronize()
    fwd = [hp.bind_grey_frame("fwd", x, o, q=q, stream=s, transform=t) for o, s, t in zip(fwd_out, streams, names)]
    inv = [hp.bind_grey_frame("inv", b[1], inv_in, q=q, stream=s, transform=t)
           for b, s, t in zip(inv_buf, streams, names)]
    for _ in range(4):
        for k in (0, 1):
            fwd[k]()
            inv[1 - k]()
    torch.cuda.synchronize()
    for k, (c, back) in enumerate(((coefs_h, back_h), (coefs_d, back_d))):
        assert np.array_equal(to_host(fwd_out[k]).reshape(-1, 64), blocks_of([c], zz, "zigzag")[0]), names[k]
        assert_only_the_frame_written(inv_buf[k][0], h, w, 520, 0, back)


# ---------------------------------------------------------------------------
# 5, 6: files
# ---------------------------------------------------------------------------
def coef_plane(blocks):
    """(ty, tx, 64) zig-zag int16 blocks -> the (8 ty, 8 tx) fp32 coefficient plane."""
    nat = np.zeros(blocks.shape, np.float32)
    nat[..., J.ZIGZAG] = blocks
    return np.ascontiguousarray(J.plane(nat.reshape(blocks.shape[:2] + (8, 8))))


@pytest.mark.parametrize("name,bound", [("pillow_grey_rows.jpg", 1), ("pillow_444_norestart.jpg", 3),
                                        ("pillow_420_blocks3.jpg", None)])
def test_pillow_files_decode_to_pillows_pixels(hp, oracle, dev, Td, name, bound):
    Image = pytest.importorskip("PIL.Image")
    from test_jpeg_unscan_host import fixture_layout
    data, lay, sampling, shapes, scan, _ = fixture_layout(hp, name)
    h, w = lay["height"], lay["width"]
    blocks, status, _, errors = U.decode(scan, sampling, shapes, lay["restart_interval"])
    assert not status.any() and errors == 0
    qs = [lay["q_luma"]] + [lay["q_chroma"]] * (lay["components"] - 1)
    planes = [inverse_plane(oracle, Td, coef_plane(b), q) for b, q in zip(blocks, qs)]
    want = planes[0][:h, :w] if lay["components"] == 1 else rgb_of(*planes, lay["subsampling"])[:h, :w]
    got = to_host(hp.jpeg_decode(data, device=dev, transform="dct", quant="file"))
    assert np.array_equal(got, want)                    # the CPU restatement, exactly
    with Image.open(io.BytesIO(data)) as im:
        px = np.asarray(im).astype(np.int64)
    err = int(np.abs(got.astype(np.int64) - px).max())
    old = int(np.abs(to_host(hp.jpeg_decode(data, device=dev, quant="file")).astype(np.int64) - px).max())
    print("%s: max |ours - Pillow| = %d with the DCT, %d with HpApprDCT" % (name, err, old))
    if bound is not None:
        assert err <= bound


def test_jpeg_encode_with_the_dct_is_what_pillow_expects(hp, oracle, dev, Td):
    Image = pytest.importorskip("PIL.Image")
    h, w = 24, 1016
    frame = oracle.rand_u8(h * w, 21).reshape(h, w)
    x = to_dev(frame, dev)

    def pillow(data):
        with Image.open(io.BytesIO(data)) as im:
            assert im.size == (w, h) and im.mode == "L"
            return np.asarray(im).astype(np.int64)

    data = hp.jpeg_encode(x, transform="dct")
    ours = to_host(hp.jpeg_decode(data, device=dev, transform="dct")).astype(np.int64)
    err = int(np.abs(ours - pillow(data)).max())
    data0 = hp.jpeg_encode(x)
    err0 = int(np.abs(to_host(hp.jpeg_decode(data0, device=dev)).astype(np.int64) - pillow(data0)).max())
    print("24x1016 noise: max |ours - Pillow| = %d with the DCT, %d with HpApprDCT" % (err, err0))
    assert err <= 1
    assert err0 > 1
    # an all-ones table: through the file to exactly the CPU restatement
    ones = np.ones((8, 8), np.float32)
    data1 = hp.jpeg_encode(x, q_luma=ones, transform="dct")
    got = to_host(hp.jpeg_decode(data1, device=dev, transform="dct", quant="file"))
    want = inverse_plane(oracle, Td, oracle.fdct(padded(frame), T=Td, Q=ones), ones)[:h, :w]
    assert np.array_equal(got, want)
    print("all-ones table: max |round trip - frame| = %d" % int(np.abs(got.astype(np.int64) - frame).max()))
