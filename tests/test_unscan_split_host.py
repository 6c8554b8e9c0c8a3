"""The split entropy decoder (hpdct_decode_scan_split), the CPU side (no GPU, no
kernel runs):

- tests/jpeg_unscan_split.py, the plain-Python restatement the GPU tests compare
  the kernels with, gives jpeg_unscan.decode's blocks and status on the corrupt
  corpus and the built scans with every interval split, and reaches each of the
  conditions that send an interval to the serial walker;
- the inputs tests/unscan_split_inputs.py builds for the GPU tests are what they
  claim to be, proved from their bytes;
- hpdct_decode_scan_split validates its arguments as hpdct_decode_scan does;
- the policy rows of the launches;
- a stand-alone program under ASan + UBSan runs the whole algorithm on the CPU
  with the kernels' own walk_segment, over the corpus and the long built scans,
  and agrees with walk_interval and with the restatement's counters.
"""
import ctypes
import struct

import numpy as np
import pytest

import host_programs
import jpeg_unscan as U
import jpeg_unscan_split as S
import unscan_built
import unscan_corpus
import unscan_split_inputs as I
from test_jpeg_unscan_host import CB, CR, INFO, OFFS, SC, ST, S420, S444, WS, Y, _p

COUNTERS = ("split_intervals", "serial_intervals", "unsettled_intervals", "rounds")


def long_cases():
    """The long built scans the stand-alone program and the GPU tests decode, with the library's geometry."""
    s, g, r = S.GEOMETRY
    return [c for c, _ in I.limits(s, g, r)] + [
        I.dense("grey", (r + 1) * g * s + 1000), I.dense("420", (r + 1) * g * s + 1000), I.half(3 * g * s),
        I.stubborn(s, g, r, True), I.stubborn(s, g, r, False), I.overlapping(s), I.whole_segment_block(s)]


def all_cases():
    """(cases, jpeg_unscan's results): the corrupt corpus, the built scans of unscan_built and the split inputs."""
    cases, results = unscan_corpus.cases_and_expected()
    more = unscan_built.corpus_cases() + I.boundaries(S.GEOMETRY[0]) + long_cases()
    return list(cases) + more, list(results) + [unscan_corpus.expected(c) for c in more]


_MEMO = []


def restated():
    """(cases, jpeg_unscan's results, the restatement's counters per case with split_min_bytes = 1), once per
    process; the restatement's blocks and status are held against jpeg_unscan's on the way."""
    if not _MEMO:
        cases, results = all_cases()
        counts = []
        for c, (want, status, found, errors) in zip(cases, results):
            got = S.decode(c["data"], c["sampling"], c["shapes"], c["ri"], c["offsets"], 1)
            assert all(np.array_equal(a, b) for a, b in zip(got[0], want)), c["name"]
            assert np.array_equal(got[1], status) and got[2:4] == (found, errors), c["name"]
            counts.append(got[4])
        _MEMO.append((cases, results, counts))
    return _MEMO[0]


def test_geometry_is_the_librarys(hp):
    assert hp.decode_split_geometry() == S.GEOMETRY
    assert hp.SPLIT_MIN_BYTES == S.DEFAULT_MIN_BYTES
    for name in ("hpdct_decode_scan_split", "hpdct_decode_split_workspace_bytes", "hpdct_decode_split_geometry"):
        assert name in hp.C_SYMBOLS
        getattr(hp.load_library(), name)


def test_restatement_equals_jpeg_unscan_and_reaches_every_condition():
    """With split_min_bytes = 1 the restatement's blocks and status are jpeg_unscan.decode's on every case (held in
    restated()), every interval that is not empty or out of range is split, and each of the serial pass's
    conditions sends at least one interval to the serial walker."""
    cases, results, counts = restated()
    assert S.REASONS and all(v > 0 for v in S.REASONS.values()), S.REASONS
    by_name = {c["name"]: k for c, k in zip(cases, counts)}
    assert by_name["clean located"] == dict(split_intervals=11, serial_intervals=0, unsettled_intervals=0, rounds=0)
    assert by_name["no bytes"]["split_intervals"] == 0 and by_name["no bytes"]["serial_intervals"] == 11
    # with the library's threshold none of the corpus' short intervals is split
    c = cases[0]
    assert S.decode(c["data"], c["sampling"], c["shapes"], c["ri"], None, 0)[4] == dict(
        split_intervals=0, serial_intervals=11, unsettled_intervals=0, rounds=0)


def test_built_inputs_are_what_they_claim():
    s, g, r = S.GEOMETRY
    cases, results, counts = restated()
    by_name = {c["name"]: (c, k) for c, k in zip(cases, counts)}
    # lengths: each target has a scan of at most that many bytes and one of more, within a block of it
    lim = I.limits(s, g, r)
    for target in (s, 2 * s, g * s, (r + 1) * g * s):
        below, above = sorted(len(c["data"]) for c, _ in lim if c["target"] == target)
        assert target - I.MAX_BLOCK_BYTES < below <= target < above <= target + I.MAX_BLOCK_BYTES
    past = [len(c["data"]) for c, _ in lim if c["target"] == r * g * s]
    assert len(past) == 1 and r * g * s < past[0] <= r * g * s + I.MAX_BLOCK_BYTES
    for c, bounded in lim:
        k = by_name[c["name"]][1]
        assert k["split_intervals"] == 1 and bounded == (len(c["data"]) <= (r + 1) * g * s)
        if bounded:                                     # the header's bound, not tuning
            assert k["serial_intervals"] == 0 and k["unsettled_intervals"] == 0
    # boundaries: every feature at every offset, and where it lies, from the bytes
    b = I.boundaries(s)
    assert {(c["feature"], c["offset"]) for c in b} == {(f, o) for f in I.FEATURES for o in range(-2, 3)}
    for c in b:
        assert I.feature_byte(c) == 2 * s + c["offset"], c["name"]
        assert by_name[c["name"]][1]["serial_intervals"] == 0
    zero_first = [c for c in b if c["feature"] == "ff00" and c["offset"] == -1][0]
    assert zero_first["data"][2 * s - 1:2 * s + 1] == b"\xff\x00"      # the 00 is a segment's first byte
    assert I._AC[0xaa][1] == 16                         # (run 10, size 10), the symbol of "code16": a 16-bit code
    # a block that covers a segment (possible while a block can be longer than a segment)
    if s <= I.MAX_BLOCK_BYTES:
        first, after = I.whole_segment_block(s)["big"]
        boundary = -(-first // s) * s
        assert first <= boundary and after > boundary + s
        assert by_name["a block that covers a segment"][1]["serial_intervals"] == 0
    # slow convergence: no EOB at all, longer than the bound; the stubborn scans settle exactly at the bound
    for name in ("dense grey", "dense 420"):
        c = by_name[name][0]
        assert len(c["data"]) > (r + 1) * g * s and all((blk[..., 1:] != 0).all() for blk in c["blocks"])
    assert by_name["half 420"][1]["rounds"] >= 1 and len(by_name["half 420"][0]["data"]) > 2 * g * s
    c, k = by_name["stubborn, settles"]
    assert -(-len(c["data"]) // (g * s)) == r + 1
    assert k == dict(split_intervals=1, serial_intervals=0, unsettled_intervals=0, rounds=r)
    c, k = by_name["stubborn, does not settle"]
    assert -(-len(c["data"]) // (g * s)) == r + 2
    assert k == dict(split_intervals=1, serial_intervals=1, unsettled_intervals=1, rounds=r)
    # overlapping offsets: more segments asked for than the budget holds
    c, k = by_name["overlapping offsets"]
    n, nbytes = len(c["offsets"]) - 1, len(c["data"])
    assert (n // 2) * -(-(nbytes - 2) // s) > -(-nbytes // s) + n
    assert 0 < k["split_intervals"] < n // 2 and k["serial_intervals"] > n // 2


# ---------------------------------------------------------------------------
# argument validation (fake pointers, never dereferenced)
# ---------------------------------------------------------------------------
def _dec(L, scan=SC, nbytes=4096, offs=OFFS, y=Y, cb=CB, cr=CR, h=16, w=32, sub=S420, ri=0, flags=0, split_min=0,
         info=INFO, st=ST, ws=WS, wsb=1 << 30):
    return L.hpdct_decode_scan_split(_p(scan), nbytes, _p(offs), _p(y), _p(cb), _p(cr), h, w, sub, ri, flags, split_min,
                                     _p(info), _p(st), _p(ws), wsb, None)


def test_decode_scan_split_arguments_rejected(hp):
    L = hp.load_library()
    err = L.hpdct_last_error_string

    def passes_every_check(**kw):
        """The call gets as far as the workspace size, the last thing judged."""
        return _dec(L, wsb=0, **kw) == 1 and b"workspace too small" in err()

    assert passes_every_check() and passes_every_check(split_min=1) and passes_every_check(split_min=1 << 62)
    assert _dec(L, split_min=-1) == 1 and b"split_min_bytes" in err()
    assert passes_every_check(cb=None, cr=None, h=8, w=8, sub=77)
    assert passes_every_check(offs=None) and passes_every_check(st=None) and passes_every_check(offs=None, st=None)
    assert passes_every_check(scan=SC + 1, nbytes=0) and passes_every_check(scan=SC + 3)
    for name in ("y", "scan", "info", "ws"):
        assert _dec(L, **{name: None}) == 1 and b"null" in err()
    assert _dec(L, cb=None) == 1 and b"null" in err()
    assert _dec(L, cr=None) == 1 and b"null" in err()
    for h, w, sub in ((0, 32, S420), (16, -16, S420), (24, 32, S420), (16, 40, S420), (12, 32, S444), (8, 20, S444)):
        assert _dec(L, h=h, w=w, sub=sub) == 1 and b"multiples of" in err()
    assert _dec(L, h=1 << 23, w=1 << 23) == 1 and b"too large" in err()
    for sub in (2, -1):
        assert _dec(L, sub=sub) == 1 and b"subsampling" in err()
    for ri in (-1, 65536, 1 << 40):
        assert _dec(L, ri=ri) == 1 and b"restart_interval" in err()
    assert _dec(L, flags=0x80) == 2 and _dec(L, flags=hp.BLOCKS_NATURAL | 0x2) == 2
    assert passes_every_check(flags=hp.BLOCKS_NATURAL)
    assert _dec(L, nbytes=-1) == 1 and b"negative" in err()
    for name, base in (("y", Y), ("cb", CB), ("cr", CR), ("ws", WS), ("offs", OFFS), ("st", ST)):
        assert _dec(L, **{name: base + 8}) == 1 and b"aligned" in err()
    assert _dec(L, info=INFO + 4) == 1 and b"aligned" in err()
    assert passes_every_check(info=INFO + 8)
    # the workspace: the serial call's, and per interval, group and segment more; one byte short is refused
    ws = L.hpdct_decode_split_workspace_bytes
    s, g, r = S.GEOMETRY
    for args in ((16, 32, 3, S420, 0, 4096), (16, 32, 3, S420, 1, 4096), (8192, 8192, 1, 0, 1024, 1 << 25)):
        need = ws(*args)
        assert need % 16 == 0 and need > L.hpdct_decode_workspace_bytes(*args)
    h, w, comps, sub, ri, nbytes = 16, 32, 3, S420, 1, 4096
    need = ws(h, w, comps, sub, ri, nbytes)
    assert ws(h, w, comps, sub, ri, nbytes + s) - need == 64                   # a segment more
    assert ws(16, 32, 2, S420, 0, 0) == -1 and ws(16, 24, 3, S420, 0, 0) == -1 and ws(16, 32, 3, 5, 0, 0) == -1
    assert ws(16, 32, 3, S420, 65536, 0) == -1 and ws(16, 32, 3, S420, 0, -1) == -1
    assert _dec(L, ri=ri, wsb=need - 1) == 1 and b"workspace too small" in err()
    assert _dec(L, wsb=-5) == 1
    with pytest.raises(hp.HpdctError):
        hp.decode_split_workspace_bytes(16, 24, components=3)
    assert hp.decode_split_workspace_bytes(16, 32, components=3, restart_interval=1, scan_bytes=4096) == need
    # overlaps: the info is 32 bytes here
    def overlap(**kw):
        st = _dec(L, wsb=0, **kw)
        assert st == 1 and (b"overlap" in err() or b"workspace too small" in err()), (st, err())
        return b"overlap" in err()
    need0 = ws(16, 32, 3, S420, 0, 4096)
    assert overlap(cb=Y + 1008) and overlap(cr=CB + 240) and overlap(scan=Y + 1023, nbytes=1)
    assert overlap(info=SC + 4088) and overlap(scan=INFO + 16) and overlap(st=INFO + 16) and overlap(ws=INFO)
    assert overlap(ri=1, offs=INFO) and overlap(ri=1, st=OFFS + 16) and overlap(st=WS + need0 - 16) and overlap(ws=ST)
    for kw in (dict(cb=Y + 1024), dict(scan=INFO + 32), dict(st=INFO + 32), dict(st=WS + need0), dict(ws=ST + 16),
               dict(info=SC + 4096)):
        assert not overlap(**kw), kw
    assert ctypes.sizeof(ctypes.c_uint32) * 8 == 32                # hpdct_decode_split_info


def test_unscan_split_wrapper_checks(hp):
    import torch as t
    from test_host_validation import FakeDev
    scan = FakeDev((100,), t.uint8)
    with pytest.raises(ValueError, match="method"):
        hp.decode_scan(scan, height=16, width=32, method="parallel")
    with pytest.raises(ValueError, match="method"):
        hp.jpeg_decode(hp.jpeg_header(8, 8, components=1) + b"\x00\xff\xd9", method="fast")
    y, c = FakeDev((2, 4, 64), t.int16), FakeDev((1, 2, 64), t.int16)
    ws = FakeDev((hp.decode_split_workspace_bytes(16, 32, components=3, scan_bytes=100),), t.uint8)
    with pytest.raises(hp.HpdctError, match="info"):
        hp.bind_decode_scan_split(scan, None, y, c, c, FakeDev((2,), t.int64), None, ws)
    with pytest.raises(hp.HpdctError, match="workspace holds"):
        hp.bind_decode_scan_split(scan, None, y, c, c, FakeDev((4,), t.int64), None, FakeDev((ws.numel() - 1,), t.uint8))
    with pytest.raises(hp.HpdctError, match="split_min_bytes"):
        hp.bind_decode_scan_split(scan, None, y, c, c, FakeDev((4,), t.int64), None, ws, split_min_bytes=-1)


def test_unscan_split_policy_rows(tmp_path):
    """tests/tools/policy_unscan_split_check.cpp: the split decoder's launches as hpdct_policy.hpp chooses them."""
    host_programs.policy_check("policy_unscan_split_check", tmp_path)


def test_unscan_split_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/tools/asan_unscan_split_check.cpp, its own main) with the C ABI's host sources (tests/tools/asan.mk's HOST) compiled by
    g++ under tests/tools/asan.mk's ASan + UBSan flags: hpdct_decode_scan_split's refusals, and the whole algorithm
    on the CPU -- lanes as loops over unsplit::walk_segment, the function the kernels call -- over the corpus, the
    built scans and the split inputs, every array of the workspace in a heap buffer of exactly its budget, each scan
    at the eight addresses mod 8, in both block orders, compared with unscan::walk_interval, with jpeg_unscan's
    results and with the restatement's four counters (the two files written here, next to the program).  CPU only:
    nothing is launched, nothing is loaded into Python."""
    cases, results, counts = restated()
    unscan_corpus.write_file(str(tmp_path / "unscan_corpus.bin"), cases, results)
    with open(str(tmp_path / "unscan_split_counts.bin"), "wb") as f:
        for k in counts:
            f.write(struct.pack("<4I", *(k[name] for name in COUNTERS)))
    host_programs.sanitised_check("asan_unscan_split_check", tmp_path, "hpdct_unscan_split.o")
