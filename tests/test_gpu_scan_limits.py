"""GPU tests of the entropy coder (hpdct_encode_scan) at the limits its buffers
and loops allow, with the inputs of tests/scan_limits.py (which
tests/test_scan_limits_host.py proves extreme on the CPU): steps that fill the
wave's bit buffer and take every stuffing pass, encode_scan's second attempt,
more intervals than the offsets kernel has threads, more intervals than the
coding launches have workgroups, side streams and reused buffers.  Byte for
byte against tests/jpeg_scan.py, no tolerance: the scan, hpdct_scan_info as a
whole and every interval offset.
"""
import time

import numpy as np
import pytest

import jpeg_scan as J
import scan_limits as S

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xA5


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)               # a copy: the inputs are read-only


def _frame(components, sampling):
    """(height, width, subsampling) of encode_scan for the components of a frame."""
    return 8 * components[0].shape[0], 8 * components[0].shape[1], "444" if sampling == "grey" else sampling


def _arrays(components, dev, order="zigzag"):
    arrays = [_dev(c if order == "zigzag" else S.natural(c), dev) for c in components]
    return arrays + [None] * (3 - len(arrays))


def _same_bytes(got, want):
    if got != want:
        first = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else -1
        raise AssertionError("scan differs: %d bytes against %d, first difference at %d" % (len(got), len(want), first))


def _check_scan(hp, dev, key, components, sampling, ri, order="zigzag", **kw):
    """One call through encode_scan (no out: its own buffers) against the restatement: bytes, info, offsets."""
    want, want_offs = S.expected(key, components, sampling, ri)
    y, cb, cr = _arrays(components, dev, order)
    h, w, sub = _frame(components, sampling)
    scan, info, offs = hp.encode_scan(y, cb, cr, height=h, width=w, subsampling=sub, restart_interval=ri, order=order,
                                      **kw)
    assert info == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
    _same_bytes(scan.cpu().numpy().tobytes(), want)
    assert offs.cpu().numpy().tolist() == want_offs
    return scan


class _Buffers:
    """The buffers of one bind_scan launch: the scan with a guard behind its capacity, everything pre-filled."""

    def __init__(self, hp, dev, components, sampling, ri, capacity, fill=FILL, offsets=True):
        import torch
        self.hp, self.capacity, self.fill = hp, capacity, fill
        self.h, self.w, self.sub = _frame(components, sampling)
        self.intervals = S.intervals_of(sampling, (self.h, self.w), ri)
        self.buf = torch.full((capacity + GUARD,), fill, dtype=torch.uint8, device=dev)
        self.info = torch.full((2,), -1, dtype=torch.int64, device=dev)
        self.offs = torch.full((self.intervals + 1,), -1, dtype=torch.int64, device=dev) if offsets else None
        n = hp.load_library().hpdct_scan_workspace_bytes(self.h, self.w, len(components), hp.SUBSAMPLINGS[self.sub], ri)
        self.ws = torch.full((n,), fill, dtype=torch.uint8, device=dev)

    def call(self, components, dev, ri, order="zigzag", stream=None, capacity=None):
        self.inputs = y, cb, cr = _arrays(components, dev, order)       # bind_scan keeps pointers only
        return self.hp.bind_scan(y, cb, cr, self.buf, self.info, self.offs, self.ws, height=self.h, width=self.w,
                                 subsampling=self.sub, restart_interval=ri, order=order,
                                 capacity=self.capacity if capacity is None else capacity, stream=stream)

    def guard_untouched(self, start=None):
        return bool((self.buf[self.capacity if start is None else start:] == self.fill).all())


# ---------------------------------------------------------------------------
# 1. saturated steps: the bit buffer full, every stuffing pass, encode_scan's second attempt
# ---------------------------------------------------------------------------
SAT_IDS = ["%s-%dx%d" % (s, h, w) for s, (h, w) in S.SATURATED_SHAPES]


@pytest.mark.parametrize("order", ["zigzag", "natural"])
@pytest.mark.parametrize("ri", [0, 1, "uneven"])
@pytest.mark.parametrize("ac", S.SATURATED_AC)
@pytest.mark.parametrize("sampling,shape", S.SATURATED_SHAPES, ids=SAT_IDS)
def test_saturated_steps(hp, dev, sampling, shape, ac, ri, order):
    """Blocks of 1656 and 1658 bits, 64 to a step: up to 3318 of the bit buffer's 3322 words, 52 passes of 256
    bytes.  Every one is larger than encode_scan's first buffer, so each result is its second attempt's."""
    if ri == "uneven":
        ri = S.UNEVEN_INTERVAL[sampling]
    comps = S.saturated(sampling, shape, ac)
    want, _ = S.expected(("sat", shape, ac), comps, sampling, ri)
    blocks, intervals = S.blocks_of(sampling, shape), S.intervals_of(sampling, shape, ri)
    assert len(want) > 128 * blocks + 4 * intervals                        # the first attempt cannot hold it
    scan = _check_scan(hp, dev, ("sat", shape, ac), comps, sampling, ri, order)
    assert scan.numel() == scan.untyped_storage().nbytes() == len(want)   # the retry's buffer: the exact size


@pytest.mark.parametrize("ri", [0, 50])
@pytest.mark.parametrize("ac", ["neg", "pos"])
def test_saturated_exact_capacity(hp, dev, ac, ri):
    """bind_scan with exactly the bytes the scan needs: all of them written, the guard behind them untouched; one
    byte less: nothing written at all."""
    shape = (8, 1088)
    comps = S.saturated("grey", shape, ac)
    want, want_offs = S.expected(("sat", shape, ac), comps, "grey", ri)
    b = _Buffers(hp, dev, comps, "grey", ri, len(want))
    b.call(comps, dev, ri)()
    assert hp.scan_info(b.info) == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
    _same_bytes(b.buf[:len(want)].cpu().numpy().tobytes(), want)
    assert b.guard_untouched()
    assert b.offs.cpu().numpy().tolist() == want_offs
    b = _Buffers(hp, dev, comps, "grey", ri, len(want) - 1)
    b.call(comps, dev, ri)()
    assert hp.scan_info(b.info) == {"bytes": len(want), "truncated": 1, "out_of_range": 0}
    assert b.guard_untouched(0)
    assert b.offs.cpu().numpy().tolist() == want_offs


def _check_unspecified_bytes(hp, dev, comps, sampling, ri, order="zigzag"):
    """A frame baseline cannot code: include/hpdct.h leaves its bytes open, so what is checked is the count, the
    size, the offsets, the guard, and that two runs into buffers filled with different values agree on every byte
    below `bytes` (each is written, and measure and emit agree)."""
    h, w, _ = _frame(comps, sampling)
    blocks, intervals = S.blocks_of(sampling, (h, w)), S.intervals_of(sampling, (h, w), ri)
    bound = hp.scan_bound(blocks, intervals)
    runs = []
    for fill in (FILL, 0x3C):
        b = _Buffers(hp, dev, comps, sampling, ri, bound, fill=fill)
        b.call(comps, dev, ri, order)()
        res = hp.scan_info(b.info)
        assert res["out_of_range"] == J.out_of_range(comps, sampling, ri) > 0
        assert 0 < res["bytes"] <= bound and res["truncated"] == 0
        o = b.offs.cpu().numpy()
        assert o[0] == 0 and o[-1] == res["bytes"] and bool((np.diff(o) > 0).all())
        assert b.guard_untouched()
        runs.append((res, o, b.buf[:res["bytes"]].clone()))
    import torch
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("order", ["zigzag", "natural"])
@pytest.mark.parametrize("ri", [0, 1])
@pytest.mark.parametrize("sampling,shape", S.SATURATED_SHAPES, ids=SAT_IDS)
def test_saturated_out_of_range(hp, dev, sampling, shape, ri, order):
    """Every coefficient 32767 or -32768: each is counted and coded with the largest category."""
    _check_unspecified_bytes(hp, dev, S.saturated_out_of_range(sampling, shape), sampling, ri, order)


# ---------------------------------------------------------------------------
# 2. more intervals than the offsets kernel has threads
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.MANY_GREY)
def test_many_intervals_grey(hp, dev, n):
    """8 x 8n at restart_interval 1: n intervals, 1, 1, 2, 3 and 3 per thread of the offsets kernel; at 2500 thread
    833 owns one interval and the threads after it none."""
    for order in ("zigzag", "natural"):
        _check_scan(hp, dev, ("sparse", n), S.sparse_grey(n), "grey", 1, order)


def test_many_intervals_420(hp, dev):
    """16 x 35200 at restart_interval 2: 1100 intervals of 12 blocks (the last two threads' chunk is partly empty)."""
    for order in ("zigzag", "natural"):
        _check_scan(hp, dev, "sparse420", S.sparse_420(), "420", 2, order)


def test_many_intervals_one_byte_short(hp, dev):
    comps = S.sparse_grey(2500)
    want, want_offs = S.expected(("sparse", 2500), comps, "grey", 1)
    b = _Buffers(hp, dev, comps, "grey", 1, len(want) - 1)
    b.call(comps, dev, 1)()
    assert hp.scan_info(b.info) == {"bytes": len(want), "truncated": 1, "out_of_range": 0}
    assert b.offs.cpu().numpy().tolist() == want_offs
    assert b.guard_untouched(0)                                            # nothing is written


def test_many_intervals_out_of_range_is_summed(hp, dev):
    """The same mask with values in +-32767: the count is a sum over every chunk and thread of the offsets kernel."""
    _check_unspecified_bytes(hp, dev, S.sparse_grey(2500, clip=False), "grey", 1)


def test_many_intervals_without_offsets(hp, dev):
    comps = S.sparse_grey(2500)
    want, _ = S.expected(("sparse", 2500), comps, "grey", 1)
    b = _Buffers(hp, dev, comps, "grey", 1, len(want), offsets=False)
    b.call(comps, dev, 1)()
    assert hp.scan_info(b.info) == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
    _same_bytes(b.buf[:len(want)].cpu().numpy().tobytes(), want)
    assert b.guard_untouched()


# ---------------------------------------------------------------------------
# 3. more intervals than the coding launches have workgroups
# ---------------------------------------------------------------------------
def test_more_intervals_than_workgroups(hp, oracle, dev):
    """8200 x 8200 grey at restart_interval 1: 1,050,625 intervals on 2^20 workgroups, so waves 0..2048 code a
    second interval (b + 2^20) after their first, with the LDS their first left behind.  Block i is
    clipped-catalogue block i % 381; the expected scan (59,323,860 bytes) is assembled from the 381 blocks' own
    scans, which tests/test_scan_limits_host.py checks against jpeg_scan.encode.  tests/tools/policy_scan_check.cpp
    pins the 2^20.  Measured on an MI355X: the encode_scan call takes 0.024 s, the whole test 0.17 s."""
    import torch
    g = S.GridCap(oracle.default_transform())
    assert g.N > S.MAX_WGS
    idx = torch.arange(g.N, device=dev) % len(g.per)
    y = _dev(g.blocks, dev)[idx].reshape(g.TILES, g.TILES, 64)             # built on the device
    want, want_offs = _dev(g.scan(g.N), dev), _dev(g.offsets(g.N), dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scan, info, offs = hp.encode_scan(y, restart_interval=1)
    torch.cuda.synchronize()
    print("encode_scan of %d intervals: %.3f s" % (g.N, time.perf_counter() - t0))
    assert info == {"bytes": 59323860, "truncated": 0, "out_of_range": 0}
    if not torch.equal(offs, want_offs):
        raise AssertionError("offsets differ first at interval %d" % int((offs != want_offs).nonzero()[0]))
    if not torch.equal(scan, want):
        byte = int((scan != want).nonzero()[0])
        iv = int(torch.searchsorted(want_offs, torch.tensor([byte], device=dev), right=True)[0]) - 1
        raise AssertionError("scan differs first at byte %d, in interval %d (wave %d's turn %d)" %
                             (byte, iv, iv % S.MAX_WGS, iv // S.MAX_WGS))


# ---------------------------------------------------------------------------
# 4. streams and reuse
# ---------------------------------------------------------------------------
def test_side_stream(hp, dev):
    import torch
    side = torch.cuda.Stream(device=dev)
    comps = S.sparse_grey(2500)
    arrays = _arrays(comps, dev)
    side.wait_stream(torch.cuda.current_stream())
    want, want_offs = S.expected(("sparse", 2500), comps, "grey", 1)
    scan, info, offs = hp.encode_scan(arrays[0], restart_interval=1, stream=side)
    assert info == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
    _same_bytes(scan.cpu().numpy().tobytes(), want)
    assert offs.cpu().numpy().tolist() == want_offs


def test_two_scans_in_flight(hp, dev):
    """Two different frames on two streams with buffers of their own, both launched before either is waited for."""
    import torch
    jobs = [(("sparse", 2500), S.sparse_grey(2500), "grey", 1), ("sparse420", S.sparse_420(), "420", 2)]
    torch.cuda.synchronize()
    runs = []
    for key, comps, sampling, ri in jobs:
        want, want_offs = S.expected(key, comps, sampling, ri)
        stream = torch.cuda.Stream(device=dev)
        b = _Buffers(hp, dev, comps, sampling, ri, len(want))
        runs.append((b, b.call(comps, dev, ri, stream=stream), stream, want, want_offs))
    torch.cuda.synchronize()                                               # the inputs and fills are in place
    for _, call, _, _, _ in runs:
        call()
    for _, _, stream, _, _ in runs:
        stream.synchronize()
    for b, _, _, want, want_offs in runs:
        assert hp.scan_info(b.info) == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
        _same_bytes(b.buf[:len(want)].cpu().numpy().tobytes(), want)
        assert b.guard_untouched()
        assert b.offs.cpu().numpy().tolist() == want_offs


def test_buffers_reused_by_a_smaller_call(hp, dev):
    """One workspace, info and offsets allocation, not cleared in between: 2500 intervals, then an 8 x 24 frame at
    interval 0 (3 blocks, 1 interval), whose result owes nothing to what the first call left."""
    big = S.sparse_grey(2500)
    want, want_offs = S.expected(("sparse", 2500), big, "grey", 1)
    b = _Buffers(hp, dev, big, "grey", 1, len(want))
    b.call(big, dev, 1)()
    assert hp.scan_info(b.info) == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
    _same_bytes(b.buf[:len(want)].cpu().numpy().tobytes(), want)
    assert b.offs.cpu().numpy().tolist() == want_offs
    small = [np.ascontiguousarray(big[0][:, 7:10])]
    want2, want_offs2 = J.encode(small, "grey", 0)
    y = _dev(small[0], dev)
    hp.bind_scan(y, None, None, b.buf, b.info, b.offs, b.ws, height=8, width=24, restart_interval=0,
                 capacity=len(want2))()
    assert hp.scan_info(b.info) == {"bytes": len(want2), "truncated": 0, "out_of_range": 0}
    _same_bytes(b.buf[:len(want2)].cpu().numpy().tobytes(), want2)
    assert b.offs[:2].cpu().numpy().tolist() == want_offs2 == [0, len(want2)]
    # beyond its own: the first call's bytes, offsets and guard as they were
    _same_bytes(b.buf[len(want2):len(want)].cpu().numpy().tobytes(), want[len(want2):])
    assert b.offs[2:].cpu().numpy().tolist() == want_offs[2:]
    assert b.guard_untouched()
