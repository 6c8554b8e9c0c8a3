"""Grey frames of any size, row pitch and quant table on the GPU
(hpdct_forward_grey_frame / hpdct_inverse_grey_frame) and the grey JPEG path
built on them: exact equality everywhere, no tolerance.

Reference: forward oracle.fdct(np.pad(frame, ((0, Hp - H), (0, Wp - W)), mode="edge"), Q=q), regrouped into
blocks by test_gpu_rgb.blocks_of; inverse oracle.to_u8(oracle.idct(coefs, Q=q))[:H, :W].

Shapes (height x width, pitch - width, base offset), the smallest at which each mechanism can fail:
  1x1               one pixel replicated over a tile; one live lane
  7x9               partial rows; one whole and one 1-pixel tile column; odd pitch
  13x515            2 x 65 tiles, odd pitch: every tile by bytes; a ragged last set; edge lanes in the middle of
                    whole staged sets
  13x515 +5         the same data with pitch 520: interior tiles on 8-byte loads, edge lanes diverging in a wave
  17x512            a whole staged set made only of bottom-edge tiles with one live row
  24x1016 +40, +1   whole tiles with an aligned pitch (no edge code), then the unaligned path on the same data
  24x1016 base 3    aligned pitch, unaligned base
  16x512            q=None equals forward_blocks / inverse_blocks(out_dtype=uint8) bit for bit
  9x16 +2^29-8      pitch 2^29 + 8: row 8 starts past 4 GiB, the 64-bit row offset (no sentinel scan)
Tables: test_gpu_rgb's three (the JPEG forms, the 3-op quotient, IEEE division) and "huge", the default table with
one entry of 2e34, which fails skip_zero_exact: the full-chain inverse.  For that table the inverse's input holds
large coefficients at the huge entry, so q * Q is infinite and the reference gives NaN and Inf.  All four on the
two mid-size shapes, the default elsewhere.  Every frame lives in a sentinel-filled buffer larger than its extent,
so every inverse also checks the pitch padding and the bytes after the last row.
"""
import io
import os

import numpy as np
import pytest

from test_gpu_parity import to_dev, to_host
from test_gpu_rgb import TABLES, _tables, blocks_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (height, width, pitch - width, base offset)
SHAPES = [(1, 1, 0, 0), (7, 9, 0, 0), (13, 515, 0, 0), (13, 515, 5, 0), (17, 512, 0, 0), (24, 1016, 40, 0),
          (24, 1016, 1, 0), (24, 1016, 0, 3)]
ALL_TABLES = {(13, 515, 0, 0), (17, 512, 0, 0)}
GREY_TABLES = TABLES + ["huge"]
CASES = [(s, t) for s in SHAPES for t in (GREY_TABLES if s in ALL_TABLES else GREY_TABLES[:1])]
CASE_IDS = ["%dx%d+%d@%d-%s" % (s + (t,)) for s, t in CASES]
ORDERS = ["zigzag", "natural"]
SENTINEL = 0xa5
SLACK = 4096          # sentinel bytes kept behind every frame's extent
BIG_PITCH = (1 << 29) + 8


def table_of(oracle, name):
    """The table as the reference sees it, and as the call is given it (None: the library's)."""
    if name == "huge":
        q = oracle.default_quant().astype(np.float32).copy()
        q[0, 1] = np.float32(2e34)
        return q, q
    ref, call = _tables(oracle, name)
    return ref[0], call[0]


def padded(frame):
    h, w = frame.shape
    return np.pad(frame, ((0, -h % 8), (0, -w % 8)), mode="edge")


_cache = {}


def _case(oracle, h, w, table):
    """(frame, reference coefficient plane of the padded frame, the inverse's input plane, reference pixels of its
    inverse cropped to the frame), computed once and never written to."""
    key = (h, w, table)
    if key not in _cache:
        frame = oracle.rand_u8(h * w, 42).reshape(h, w)
        q, _ = table_of(oracle, table)
        coefs = oracle.fdct(padded(frame), Q=q)
        inp = coefs
        if table == "huge":
            # the forward leaves zeros at the huge entry; the decoder-side input has large values there
            inp = coefs.copy()
            inp[0::8, 1::16] = 30000.0
            inp[0::8, 9::16] = -32768.0
            with np.errstate(over="ignore"):
                assert np.isinf(inp[0::8, 1::8] * q[0, 1]).all()
        rec = oracle.idct(np.array(inp), Q=q)
        if table == "huge":
            assert not np.isfinite(rec).all()
        back = oracle.to_u8(rec)[:h, :w]
        for a in (frame, coefs, inp, back):
            a.setflags(write=False)
        _cache[key] = (frame, coefs, inp, back)
    return _cache[key]


@pytest.fixture(scope="module")
def zz(hp):
    return hp.zigzag_order().astype(np.int64)


def frame_buffer(dev, h, w, pitch, offset=0):
    """A sentinel-filled byte buffer and the (h, w) view of it that starts `offset` bytes in with rows `pitch`
    bytes apart."""
    import torch
    buf = torch.full((offset + (h - 1) * pitch + w + SLACK,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf.as_strided((h, w), (pitch, 1), offset)


def frame_on_device(dev, frame, pitch, offset=0):
    import torch
    h, w = frame.shape
    _, view = frame_buffer(dev, h, w, pitch, offset)
    view.copy_(torch.from_numpy(np.array(frame)).to(dev))      # a writable copy: the reference stays read-only
    return view


def assert_only_the_frame_written(buf, h, w, pitch, offset, want):
    """The frame's bytes equal `want`; every other byte of the buffer keeps the sentinel."""
    got = to_host(buf)
    live = np.zeros(got.shape, bool)
    for r in range(h):
        live[offset + r * pitch: offset + r * pitch + w] = True
    assert np.array_equal(got[live].reshape(h, w), want)
    assert (got[~live] == SENTINEL).all(), "%d bytes outside the frame were written" % int((got[~live] != SENTINEL).sum())


def blocks_on_device(dev, zz, plane, order):
    return to_dev(blocks_of([plane], zz, order, shape3=True)[0], dev)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape,table", CASES, ids=CASE_IDS)
def test_forward_frame_matches_reference(hp, oracle, dev, zz, shape, table, order):
    import torch
    h, w, extra, offset = shape
    frame, coefs, _, _ = _case(oracle, h, w, table)
    x = frame_on_device(dev, frame, w + extra, offset)
    assert x.data_ptr() % 8 == offset
    want = blocks_of([coefs], zz, order)[0]
    # a sentinel behind the blocks: the forward writes its block array only
    out = torch.full((want.size + 64 * 64,), -21846, dtype=torch.int16, device=dev)  # 0xaaaa
    got = hp.forward_grey_frame(x, q=table_of(oracle, table)[1], order=order, out=out)
    assert got is out
    assert hp.grey_frame_geometry(h, w) == (coefs.shape[0], coefs.shape[1], want.shape[0])
    host = to_host(out)
    assert np.array_equal(host[:want.size].reshape(-1, 64), want)
    assert (host[want.size:] == -21846).all()
    fresh = hp.forward_grey_frame(x, q=table_of(oracle, table)[1], order=order)
    assert fresh.dtype == torch.int16 and tuple(fresh.shape) == (coefs.shape[0] // 8, coefs.shape[1] // 8, 64)
    assert torch.equal(fresh.reshape(-1), out[:want.size])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape,table", CASES, ids=CASE_IDS)
def test_inverse_frame_matches_reference(hp, oracle, dev, zz, shape, table, order):
    h, w, extra, offset = shape
    _, _, inp, want = _case(oracle, h, w, table)
    b = blocks_on_device(dev, zz, inp, order)
    buf, out = frame_buffer(dev, h, w, w + extra, offset)
    got = hp.inverse_grey_frame(b, height=h, width=w, q=table_of(oracle, table)[1], order=order, out=out)
    assert got is out
    assert_only_the_frame_written(buf, h, w, w + extra, offset, want)


def test_dense_whole_frame_equals_the_blocks_calls(hp, oracle, dev):
    """16x512 dense with q=None: bit for bit hp.forward_blocks / hp.inverse_blocks(out_dtype=uint8)."""
    import torch
    x = to_dev(oracle.rand_u8(16 * 512, 3).reshape(16, 512), dev)
    for order in ORDERS:
        got = hp.forward_grey_frame(x, order=order)
        want = hp.forward_blocks(x, order=order)
        assert got.shape == want.shape and torch.equal(got, want)
        back = hp.inverse_grey_frame(got, height=16, width=512, order=order)
        assert back.dtype == torch.uint8 and torch.equal(back, hp.inverse_blocks(want, out_dtype=torch.uint8, order=order))


def test_rows_past_4gib(hp, oracle, dev, zz):
    """9x16 with a pitch of 2^29 + 8 bytes: row 8, the second tile row, starts past 4 GiB."""
    import torch
    h, w = 9, 16
    frame, coefs, inp, want = _case(oracle, h, w, "default")
    buf = torch.empty(((h - 1) * BIG_PITCH + w,), dtype=torch.uint8, device=dev)      # uninitialised
    view = buf.as_strided((h, w), (BIG_PITCH, 1), 0)
    assert (h - 1) * BIG_PITCH >= 1 << 32
    view.copy_(to_dev(np.array(frame), dev))
    got = hp.forward_grey_frame(view)
    assert np.array_equal(to_host(got).reshape(-1, 64), blocks_of([coefs], zz, "zigzag")[0])
    view.fill_(SENTINEL)
    hp.inverse_grey_frame(blocks_on_device(dev, zz, inp, "zigzag"), height=h, width=w, out=view)
    assert np.array_equal(to_host(view.contiguous()), want)
    del buf, view


def test_two_tables_on_two_streams_at_once(hp, oracle, dev, zz):
    """Two bound forwards and two bound inverses with different tables, interleaved on two streams: each result
    equals its own reference (the table travels with the launch, not in process-wide state)."""
    import torch
    h, w = 13, 515
    names = ("q75", "x0.37")
    cases = [_case(oracle, h, w, n) for n in names]
    qs = [table_of(oracle, n)[1] for n in names]
    streams = [torch.cuda.Stream(device=dev) for _ in names]
    x = frame_on_device(dev, cases[0][0], 520)
    fwd_out = [torch.zeros((2, 65, 64), dtype=torch.int16, device=dev) for _ in names]
    inv_in = [blocks_on_device(dev, zz, c[2], "zigzag") for c in cases]
    inv_buf = [frame_buffer(dev, h, w, 520) for _ in names]
    torch.cuda.synchronize()
    fwd = [hp.bind_grey_frame("fwd", x, o, q=q, stream=s) for o, q, s in zip(fwd_out, qs, streams)]
    inv = [hp.bind_grey_frame("inv", b[1], i, q=q, stream=s) for b, i, q, s in zip(inv_buf, inv_in, qs, streams)]
    assert all(c.tables[0] is not None for c in fwd + inv)      # the host table lives as long as the callable
    for _ in range(4):
        for k in (0, 1):
            fwd[k]()
            inv[1 - k]()
    torch.cuda.synchronize()
    for k in (0, 1):
        assert np.array_equal(to_host(fwd_out[k]).reshape(-1, 64), blocks_of([cases[k][1]], zz, "zigzag")[0]), names[k]
        assert_only_the_frame_written(inv_buf[k][0], h, w, 520, 0, cases[k][3])


def test_no_global_state(hp, oracle, dev, zz):
    """The calls leave get_quant_table() and forward_blocks alone, and q=None follows set_quant_table."""
    import torch
    h, w = 7, 9
    fixed = to_dev(oracle.rand_u8(16 * 64, 5).reshape(16, 64), dev)
    before_q, before_b = hp.get_quant_table().copy(), hp.forward_blocks(fixed).clone()
    q75, call75 = table_of(oracle, "q75")
    frame, _, _, _ = _case(oracle, h, w, "q75")
    x = frame_on_device(dev, frame, w)
    got75 = hp.forward_grey_frame(x, q=call75)
    hp.inverse_grey_frame(got75, height=h, width=w, q=call75)
    torch.cuda.synchronize()
    assert np.array_equal(hp.get_quant_table(), before_q)
    assert torch.equal(hp.forward_blocks(fixed), before_b)
    default = hp.forward_grey_frame(x)
    assert not torch.equal(default, got75)
    hp.set_quant_table(q75)
    try:
        assert torch.equal(hp.forward_grey_frame(x), got75)                    # q=None: the library table now
        assert torch.equal(hp.inverse_grey_frame(got75, height=h, width=w),
                           hp.inverse_grey_frame(got75, height=h, width=w, q=call75))
        assert torch.equal(hp.forward_grey_frame(x, q=oracle.default_quant()), default)  # a per-call table wins
    finally:
        hp.set_quant_table(None)
    assert torch.equal(hp.forward_grey_frame(x), default)


def test_range_table_refused_and_nothing_written(hp, oracle, dev):
    import torch
    tiny = np.full((8, 8), 1.0 / 64.0, np.float32)
    x = frame_on_device(dev, _case(oracle, 7, 9, "default")[0], 9)
    out = torch.full((1, 2, 64), -21846, dtype=torch.int16, device=dev)
    with pytest.raises(hp.HpdctError) as e:
        hp.forward_grey_frame(x, q=tiny, out=out)
    assert e.value.status == 3
    buf, px = frame_buffer(dev, 7, 9, 9)
    with pytest.raises(hp.HpdctError) as e:
        hp.inverse_grey_frame(out, height=7, width=9, q=tiny, out=px)
    assert e.value.status == 3
    torch.cuda.synchronize()
    assert bool((out == -21846).all()) and bool((buf == SENTINEL).all())


# ---------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["serial", "split"])
@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimised"])
@pytest.mark.parametrize("table", ["default", "q75"])
def test_jpeg_round_trip_of_a_ragged_grey_frame(hp, oracle, dev, table, optimize, method):
    """jpeg_decode(jpeg_encode(x, q_luma=q), quant="file") for a 43x61 frame is the library's own inverse of its
    own forward under q; the header carries the true size and q; Pillow opens the file at 43x61."""
    import torch
    h, w = 43, 61
    qref, q = table_of(oracle, table)
    x = frame_on_device(dev, oracle.rand_u8(h * w, 11).reshape(h, w), w)
    data = hp.jpeg_encode(x, q_luma=q, optimize=optimize)
    lay = hp.jpeg_parse_tables(data)
    assert (lay["height"], lay["width"], lay["components"]) == (h, w, 1)
    assert np.array_equal(lay["q_luma"].reshape(-1), qref.reshape(-1))
    want = hp.inverse_grey_frame(hp.forward_grey_frame(x, q=q), height=h, width=w, q=q)
    got = hp.jpeg_decode(data, device=dev, method=method, quant="file")
    assert tuple(got.shape) == (h, w) and got.dtype == torch.uint8 and torch.equal(got, want)
    if table != "default":
        with pytest.raises(hp.HpdctError, match="set_quant_table"):
            hp.jpeg_decode(data, device=dev, method=method)                    # the default mode still refuses


@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimised"])
def test_pillow_opens_the_ragged_grey_file(hp, oracle, dev, optimize):
    Image = pytest.importorskip("PIL.Image")
    x = to_dev(oracle.rand_u8(43 * 61, 11).reshape(43, 61), dev)
    data = hp.jpeg_encode(x, q_luma=table_of(oracle, "q75")[1], optimize=optimize)
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        assert im.size == (61, 43) and im.mode == "L"


def test_jpeg_encode_of_a_strided_view(hp, oracle, dev):
    """A 43x61 view of a larger frame gives the file of its dense copy."""
    big = to_dev(oracle.rand_u8(50 * 80, 12).reshape(50, 80), dev)
    view = big[3:46, 8:69]
    assert not view.is_contiguous()
    assert hp.jpeg_encode(view) == hp.jpeg_encode(view.contiguous())


@pytest.mark.parametrize("name", ["pillow_grey_rows.jpg", "pillow_opt_grey_rows.jpg"])
def test_pillow_grey_files_under_their_own_table(hp, dev, name):
    """With the library table at its default, quant="file" gives the 43x61 pixels of today's route
    (set_quant_table(file's table), jpeg_decode, reset); the default call still raises."""
    import torch
    data = open(os.path.join(GOLDEN, name), "rb").read()
    lay = hp.jpeg_parse_tables(data)
    assert np.array_equal(hp.get_quant_table(), hp.default_quant_table())
    assert not np.array_equal(lay["q_luma"], hp.default_quant_table())
    got = hp.jpeg_decode(data, device=dev, quant="file")
    assert tuple(got.shape) == (43, 61) and got.dtype == torch.uint8 and got.is_contiguous()
    assert np.array_equal(hp.get_quant_table(), hp.default_quant_table())
    with pytest.raises(hp.HpdctError, match="set_quant_table"):
        hp.jpeg_decode(data, device=dev)
    hp.set_quant_table(lay["q_luma"])
    try:
        want = hp.jpeg_decode(data, device=dev).clone()
    finally:
        hp.set_quant_table(None)
    assert torch.equal(got, want)
    for method in ("serial", "split"):
        assert torch.equal(hp.jpeg_decode(data, device=dev, method=method, quant="file"), want)


def test_damaged_grey_scan_is_reported_under_quant_file(hp, oracle, dev):
    import jpeg_unscan as U
    x = to_dev(oracle.rand_u8(43 * 61, 13).reshape(43, 61), dev)
    data = hp.jpeg_encode(x, q_luma=table_of(oracle, "q75")[1])
    lay = hp.jpeg_parse(data)
    scan = data[lay["scan_offset"]:lay["scan_offset"] + lay["scan_bytes"]]
    at = lay["scan_offset"] + U.markers(scan)[-1]       # the last restart marker, cut out: an interval goes missing
    with pytest.raises(hp.HpdctError, match="damaged restart intervals"):
        hp.jpeg_decode(data[:at] + data[at + 2:], device=dev, quant="file")
    with pytest.raises(ValueError):
        hp.jpeg_decode(data, device=dev, quant="other")
