"""The corrupt-input corpus of the entropy decoder's tests (a helper: no test in
it): scans and offset tables that hpdct_decode_scan must survive and report on
exactly as tests/jpeg_unscan.py does.  The same cases go through the restatement
(test_jpeg_unscan_host.py), the shared walker on the CPU under ASan + UBSan
(tests/tools/asan_unscan_check.cpp reads the file write_file() makes) and the
kernels (test_gpu_unscan.py).

A case: dict(name, data, sampling, shapes, ri, offsets) with offsets None (the
markers are located) or a list of intervals + 1 integers in 0 .. 2^64 - 1.
"""
import struct

import numpy as np

import jpeg_scan as J
import jpeg_unscan as U

GREY_SHAPES = [(3, 7)]                                  # a 24 x 56 grey frame, 21 blocks
GREY_RI = 2                                             # 11 intervals, the last one a single block


def sparse_blocks(shape, seed, density=0.35, top=1023):
    """Random blocks in baseline's range: mostly small values, some zeros runs, a few large ones."""
    rng = np.random.default_rng(seed)
    ty, tx = shape
    b = rng.integers(-40, 41, (ty, tx, 64))
    b[rng.random((ty, tx, 64)) > density] = 0
    big = rng.random((ty, tx, 64)) < 0.02
    b[big] = rng.integers(-top, top + 1, int(big.sum()))
    b[..., 0] = rng.integers(-500, 501, (ty, tx))
    if ty * tx > 2:
        b.reshape(-1, 64)[1] = 0                        # an all-zero block
        b.reshape(-1, 64)[2, 63] = 5                    # a block without EOB
    return b.astype(np.int16)


def base_grey():
    """(blocks, scan, offsets) of the ~1 KB grey scan every flip and truncation starts from."""
    blocks = sparse_blocks(GREY_SHAPES[0], 3, density=0.5)
    data, offs = J.encode([blocks], "grey", GREY_RI)
    return blocks, data, offs


def _case(name, data, offsets=None, sampling="grey", shapes=None, ri=GREY_RI):
    return dict(name=name, data=bytes(data), sampling=sampling, shapes=shapes or GREY_SHAPES, ri=ri, offsets=offsets)


def dc_case():
    """18 blocks whose DC differences are all +2047 in one interval: the predictor passes 32767 at the 17th."""
    blocks = np.zeros((3, 6, 64), np.int64)
    w = J._Bits()
    code, length = J.codes_of(J.DC_LUMA)[11]
    eob = J.codes_of(J.AC_LUMA)[0x00]
    for _ in range(18):
        w.put(code, length)
        w.put(2047, 11)
        w.put(*eob)
    return _case("dc overflow", w.finish(), None, "grey", [(3, 6)], 0)


def build():
    _, data, offs = base_grey()
    cases = [_case("clean located", data), _case("clean offsets", data, list(offs))]
    for bit in range(8 * len(data)):
        d = bytearray(data)
        d[bit >> 3] ^= 0x80 >> (bit & 7)
        cases.append(_case("flip %d" % bit, d))
    for n in range(len(data)):
        cases.append(_case("truncated to %d" % n, data[:n]))
    # the same corruptions with the offsets given: every 7th flip, every 5th truncation (the table still
    # describes the whole scan, so its tail is out of range)
    for bit in range(0, 8 * len(data), 7):
        d = bytearray(data)
        d[bit >> 3] ^= 0x80 >> (bit & 7)
        cases.append(_case("flip %d, offsets" % bit, d, list(offs)))
    for n in range(0, len(data), 5):
        cases.append(_case("truncated to %d, offsets" % n, data[:n], list(offs)))
    # markers deleted, duplicated and renumbered
    mk = U.markers(data)
    assert len(mk) == 10
    for j in (0, 4, 9):
        p = mk[j]
        cases.append(_case("marker %d deleted" % j, data[:p] + data[p + 2:]))
        cases.append(_case("marker %d duplicated" % j, data[:p] + data[p:p + 2] + data[p:]))
        for number in (0, 3, 7):
            d = bytearray(data)
            d[p + 1] = 0xd0 + number
            cases.append(_case("marker %d renumbered %d" % (j, number), d))
    cases.append(_case("ff as last byte", data[:-1] + b"\xff"))
    cases.append(_case("ff appended", data + b"\xff"))
    cases.append(_case("marker appended", data + b"\xff\xd2"))
    cases.append(_case("zero appended", data + b"\x00"))
    cases.append(_case("no bytes", b""))
    cases.append(_case("no bytes, offsets", b"", [0] * len(offs)))
    cases.append(_case("one ff", b"\xff"))
    cases.append(_case("all ff", b"\xff" * 64))
    cases.append(_case("all zero", b"\x00" * 64))
    cases.append(_case("all markers", b"\xff\xd0" * 40))
    # offset tables
    n = len(data)
    cases.append(_case("offsets descend", data, list(offs[::-1])))
    cases.append(_case("offsets exceed bytes", data, [o + n for o in offs]))
    cases.append(_case("offsets 2^63", data, [offs[0]] + [1 << 63] * (len(offs) - 1)))
    cases.append(_case("offsets 2^64 - 1", data, [(1 << 64) - 1] * len(offs)))
    cases.append(_case("offsets all 1", data, [1] * len(offs)))
    cases.append(_case("offsets shifted by one", data, [offs[0]] + [o + 1 for o in offs[1:-1]] + [offs[-1]]))
    cases.append(_case("offsets of a wider first interval", data, [0, offs[2]] + list(offs[2:])))
    cases.append(dc_case())
    return cases


def expected(case):
    """(blocks, status, markers_found, marker_errors) by the restatement."""
    return U.decode(case["data"], case["sampling"], case["shapes"], case["ri"], case["offsets"])


_MEMO = []


def cases_and_expected():
    """(cases, results), computed once per process and shared by the tests; treat both as read-only."""
    if not _MEMO:
        cases = build()
        _MEMO.append((cases, [expected(c) for c in cases]))
    return _MEMO[0]


SAMPLING_CODE = {"grey": (1, 0), "444": (3, 0), "420": (3, 1)}


def write_file(path, cases, results):
    """The corpus and what the restatement makes of it, for asan_unscan_check.cpp (little-endian):
    uint32 count, then per case: uint32 components, sub, y tile rows, y tile columns, ri, has_offsets, intervals,
    markers_found, marker_errors, pad; uint64 bytes; the scan; has_offsets * (intervals + 1) uint64; intervals
    uint64 status; the int16 blocks of every component."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c, (blocks, status, found, errors) in zip(cases, results):
            comps, sub = SAMPLING_CODE[c["sampling"]]
            ty, tx = c["shapes"][0]
            f.write(struct.pack("<10IQ", comps, sub, ty, tx, c["ri"], int(c["offsets"] is not None), len(status),
                                found, errors, 0, len(c["data"])))
            f.write(c["data"])
            if c["offsets"] is not None:
                f.write(np.asarray(c["offsets"], np.uint64).tobytes())
            f.write(np.asarray(status, np.uint64).tobytes())
            for b in blocks:
                f.write(np.ascontiguousarray(b, np.int16).tobytes())
