"""Colour frames of any size and row pitch on the GPU (hpdct_forward_rgb_frame /
hpdct_inverse_rgb_frame): exact equality with the host reference, no tolerance.

Reference: the frame edge-padded to whole units with
np.pad(rgb, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge"), then test_gpu_rgb's
ref_forward / ref_inverse / blocks_of; the inverse cropped to [:H, :W].

Shapes, the smallest at which each mechanism can fail (pitch in bytes; dense
when not given):
  444  1x1              one pixel replicated over a whole tile; one live lane
  444  7x9              partial rows; one whole and one 1-pixel tile column
  444  13x515           2 x 65 units: edge lanes in the middle of whole (staged) sets, a ragged last
                        set, dense pitch 1545 (odd)
  444  17x512           a whole staged set made only of bottom-edge units (1 live row)
  444  24x1016 +40, +1  whole units: the unclipped instantiation with a pitch; then the unaligned
                        path on the same data
  420  1x1, 15x17       odd height and width: quads straddling both edges
  420  18x1030          width mod 16 = 6: the MCU's second Y tile column is all padding; 65 MCUs a row
  420  40x1032          width mod 16 = 8: exactly one Y tile column; height mod 16 = 8
  420  25x1033          width mod 16 = 9, odd height
  420  33x1024          64 MCUs a row: whole sets on the 16 KiB staged Y path whose last MCU row has
                        one live pixel row
  420  128x1024 +64     whole MCUs with a pitch
Every frame lives in a sentinel-filled buffer larger than its extent, so every
inverse also checks the pitch padding and the bytes after the last row.
"""
import numpy as np
import pytest

from test_gpu_parity import to_dev, to_host
from test_gpu_rgb import TABLES, _tables, blocks_of, ref_forward, ref_inverse

pytestmark = pytest.mark.gpu

# (subsampling, height, width, pitch - 3 * width)
SHAPES = [("444", 1, 1, 0), ("444", 7, 9, 0), ("444", 13, 515, 0), ("444", 17, 512, 0),
          ("444", 24, 1016, 40), ("444", 24, 1016, 1),
          ("420", 1, 1, 0), ("420", 15, 17, 0), ("420", 18, 1030, 0), ("420", 40, 1032, 0),
          ("420", 25, 1033, 0), ("420", 33, 1024, 0), ("420", 128, 1024, 64)]
# the three table pairs on the two mid-size shapes of each subsampling, the default pair elsewhere
ALL_TABLES = {("444", 13, 515, 0), ("444", 17, 512, 0), ("420", 18, 1030, 0), ("420", 25, 1033, 0)}
CASES = [(s, t) for s in SHAPES for t in (TABLES if s in ALL_TABLES else TABLES[:1])]
CASE_IDS = ["%s-%dx%d+%d-%s" % (s + (t,)) for s, t in CASES]
ORDERS = ["zigzag", "natural"]
SENTINEL = 0xa5
SLACK = 4096          # sentinel bytes kept behind every frame's extent


def padded(rgb, sub):
    side = 16 if sub == "420" else 8
    h, w = rgb.shape[:2]
    hp, wp = -(-h // side) * side, -(-w // side) * side
    return np.pad(rgb, ((0, hp - h), (0, wp - w), (0, 0)), mode="edge")


_cache = {}


def _case(oracle, sub, h, w, table):
    """(rgb, reference coefficient planes of the padded frame, reference RGB of their inverse cropped to the
    frame), computed once and never written to."""
    key = (sub, h, w, table)
    if key not in _cache:
        rgb = oracle.rand_u8(3 * h * w, 42).reshape(h, w, 3)
        (ql, qc), _ = _tables(oracle, table)
        coefs = ref_forward(oracle, padded(rgb, sub), sub, ql, qc)
        back = ref_inverse(oracle, coefs, sub, ql, qc)[:h, :w]
        for a in (rgb, back) + tuple(coefs):
            a.setflags(write=False)
        _cache[key] = (rgb, coefs, back)
    return _cache[key]


@pytest.fixture(scope="module")
def zz(hp):
    return hp.zigzag_order().astype(np.int64)


def frame_buffer(dev, h, w, pitch, offset=0):
    """A sentinel-filled byte buffer and the (h, w, 3) view of it that starts `offset` bytes in with rows
    `pitch` bytes apart."""
    import torch
    buf = torch.full((offset + (h - 1) * pitch + 3 * w + SLACK,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf.as_strided((h, w, 3), (pitch, 3, 1), offset)


def frame_on_device(dev, rgb, pitch, offset=0):
    import torch
    h, w = rgb.shape[:2]
    buf, view = frame_buffer(dev, h, w, pitch, offset)
    view.copy_(torch.from_numpy(np.array(rgb)).to(dev))      # a writable copy: the reference stays read-only
    return view


def assert_only_the_frame_written(buf, h, w, pitch, offset, want):
    """The frame's bytes equal `want`; every other byte of the buffer keeps the sentinel."""
    got = to_host(buf)
    live = np.zeros(got.shape, bool)
    for r in range(h):
        live[offset + r * pitch: offset + r * pitch + 3 * w] = True
    assert np.array_equal(got[live].reshape(h, w, 3), want)
    assert (got[~live] == SENTINEL).all(), "%d bytes outside the frame were written" % int((got[~live] != SENTINEL).sum())


def assert_blocks(got, want):
    for g, w, name in zip(got, want, "y cb cr".split()):
        assert np.array_equal(to_host(g).reshape(-1, 64), w.reshape(-1, 64)), name


def block_shapes(h, w, sub):
    side = 16 if sub == "420" else 8
    hp, wp = -(-h // side) * side, -(-w // side) * side
    ch, cw = (hp // 2, wp // 2) if sub == "420" else (hp, wp)
    return [(hp // 8, wp // 8, 64)] + [(ch // 8, cw // 8, 64)] * 2


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape,table", CASES, ids=CASE_IDS)
def test_forward_frame_matches_reference(hp, oracle, dev, zz, shape, table, order):
    import torch
    sub, h, w, extra = shape
    rgb, coefs, _ = _case(oracle, sub, h, w, table)
    _, (ql, qc) = _tables(oracle, table)
    x = frame_on_device(dev, rgb, 3 * w + extra)
    got = hp.forward_rgb_frame(x, subsampling=sub, q_luma=ql, q_chroma=qc, order=order)
    assert all(g.dtype == torch.int16 for g in got)
    assert [tuple(g.shape) for g in got] == block_shapes(h, w, sub)
    assert hp.rgb_frame_geometry(h, w, sub)[2:] == (got[0].numel() // 64, got[1].numel() // 64)
    assert_blocks(got, blocks_of(coefs, zz, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape,table", CASES, ids=CASE_IDS)
def test_inverse_frame_matches_reference(hp, oracle, dev, zz, shape, table, order):
    sub, h, w, extra = shape
    _, coefs, want = _case(oracle, sub, h, w, table)
    _, (ql, qc) = _tables(oracle, table)
    y, cb, cr = (to_dev(b, dev) for b in blocks_of(coefs, zz, order, shape3=True))
    buf, out = frame_buffer(dev, h, w, 3 * w + extra)
    got = hp.inverse_rgb_frame(y, cb, cr, height=h, width=w, subsampling=sub, q_luma=ql, q_chroma=qc, order=order,
                               out=out)
    assert got is out
    assert_only_the_frame_written(buf, h, w, 3 * w + extra, 0, want)


@pytest.mark.parametrize("offset", [1, 4])
@pytest.mark.parametrize("sub,h,w", [("444", 13, 515), ("420", 18, 1030)], ids=["444-13x515", "420-18x1030"])
def test_base_offset(hp, oracle, dev, zz, sub, h, w, offset):
    """The frame starts 1 and 4 bytes into a larger allocation: no 8-byte load or store is legal."""
    rgb, coefs, want = _case(oracle, sub, h, w, "default")
    x = frame_on_device(dev, rgb, 3 * w, offset)
    assert x.data_ptr() % 8 == offset
    assert_blocks(hp.forward_rgb_frame(x, subsampling=sub), blocks_of(coefs, zz, "zigzag"))
    buf, out = frame_buffer(dev, h, w, 3 * w, offset)
    b = [to_dev(t, dev) for t in blocks_of(coefs, zz, "zigzag", shape3=True)]
    hp.inverse_rgb_frame(*b, height=h, width=w, subsampling=sub, out=out)
    assert_only_the_frame_written(buf, h, w, 3 * w, offset, want)


@pytest.mark.parametrize("sub,h,w", [("444", 13, 515), ("420", 25, 1033)], ids=["444-13x515", "420-25x1033"])
def test_view_agrees_with_blocks_of_the_padded_frame(hp, oracle, dev, sub, h, w):
    """On the device alone: forward_rgb_frame of an H x W view of a larger frame equals forward_rgb_blocks
    of the explicitly edge-padded copy, and inverse_rgb_frame equals the crop of inverse_rgb_blocks."""
    import torch
    side = 16 if sub == "420" else 8
    hp_, wp_ = -(-h // side) * side, -(-w // side) * side
    bw = -(-(w + 24) // 8) * 8                      # a pitch of 3 bw bytes and a view 24 bytes into its rows:
    big = to_dev(oracle.rand_u8(3 * (h + 5) * bw, 7).reshape(h + 5, bw, 3), dev)
    view = big[3:3 + h, 8:8 + w]                    # 8-byte aligned, so only the edge units leave the 8-byte loads
    assert not view.is_contiguous() and view.data_ptr() % 8 == 0 and view.stride(0) % 8 == 0
    rows = torch.clamp(torch.arange(hp_, device=dev), max=h - 1)
    cols = torch.clamp(torch.arange(wp_, device=dev), max=w - 1)
    pad = view[rows][:, cols].contiguous()
    got = hp.forward_rgb_frame(view, subsampling=sub)
    want = hp.forward_rgb_blocks(pad, subsampling=sub)
    for g, wnt, name in zip(got, want, "y cb cr".split()):
        assert torch.equal(g, wnt), name
    back = hp.inverse_rgb_frame(*got, height=h, width=w, subsampling=sub)
    assert torch.equal(back, hp.inverse_rgb_blocks(*want, subsampling=sub)[:h, :w])


@pytest.mark.parametrize("sub,h,w", [("444", 64, 512), ("420", 128, 1024)], ids=["444", "420"])
def test_dense_aligned_shape_equals_the_existing_calls(hp, oracle, dev, sub, h, w):
    import torch
    x = to_dev(oracle.rand_u8(3 * h * w, 3).reshape(h, w, 3), dev)
    for order in ORDERS:
        got = hp.forward_rgb_frame(x, subsampling=sub, order=order)
        want = hp.forward_rgb_blocks(x, subsampling=sub, order=order)
        for g, wnt in zip(got, want):
            assert g.shape == wnt.shape and torch.equal(g, wnt)
        back = hp.inverse_rgb_frame(*got, height=h, width=w, subsampling=sub, order=order)
        assert torch.equal(back, hp.inverse_rgb_blocks(*want, subsampling=sub, order=order))


@pytest.mark.parametrize("sub,h,w", [("444", 13, 515), ("444", 17, 512), ("420", 18, 1030), ("420", 33, 1024)],
                         ids=["444-13x515", "444-17x512", "420-18x1030", "420-33x1024"])
def test_forward_writes_its_block_arrays_only(hp, oracle, dev, zz, sub, h, w):
    import torch
    rgb, coefs, _ = _case(oracle, sub, h, w, "default")
    want = blocks_of(coefs, zz, "zigzag")
    pad = 64 * 64
    out = tuple(torch.full((b.size + pad,), -21846, dtype=torch.int16, device=dev) for b in want)  # 0xaaaa
    hp.forward_rgb_frame(frame_on_device(dev, rgb, 3 * w), subsampling=sub, out=out)
    for o, b, name in zip(out, want, "y cb cr".split()):
        got = to_host(o)
        assert np.array_equal(got[:b.size].reshape(-1, 64), b), name
        assert (got[b.size:] == -21846).all(), name


@pytest.mark.parametrize("sub,h,w", [("444", 7, 9), ("420", 15, 17), ("420", 25, 1033)],
                         ids=["444-7x9", "420-15x17", "420-25x1033"])
def test_round_trip(hp, oracle, dev, sub, h, w):
    """inverse(forward(x)) is the reference's own round trip."""
    rgb, _, want = _case(oracle, sub, h, w, "default")
    blocks = hp.forward_rgb_frame(frame_on_device(dev, rgb, 3 * w), subsampling=sub)
    got = hp.inverse_rgb_frame(*blocks, height=h, width=w, subsampling=sub)
    assert tuple(got.shape) == (h, w, 3)
    assert np.array_equal(to_host(got), want)
