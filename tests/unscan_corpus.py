"""The corrupt-input corpus of the entropy decoder's tests (a helper: no test in
it): scans and offset tables that hpdct_decode_scan must survive and report on
exactly as tests/jpeg_unscan.py does.  The same cases go through the restatement
(test_jpeg_unscan_host.py), the shared walker on the CPU under ASan + UBSan
(tests/tools/asan_unscan_check.cpp reads the file write_file() makes) and the
kernels (test_gpu_unscan.py).

A case: dict(name, data, sampling, shapes, ri, offsets) with offsets None (the
markers are located) or a list of intervals + 1 integers in 0 .. 2^64 - 1.  A
case may name the byte that follows the scan in memory ("after"): a test that
places the scan inside a larger buffer writes it there, and the result must not
depend on it.

Three bases, each with every single-bit flip and every truncation: grey, and
(COLOUR) a 4:2:0 and a 4:4:4 scan whose chroma tables, three predictors and
zero fill from the middle of an MCU a grey scan never reaches.
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


# the colour bases: 4:2:0, Y 4 x 4 and chroma 2 x 2 (4 MCUs of 6 blocks), one MCU per interval; 4:4:4, 2 x 4 per
# component (8 MCUs of 3 blocks), 3 MCUs per interval, the last interval 2
COLOUR = {"420": ([(4, 4), (2, 2), (2, 2)], 1), "444": ([(2, 4)] * 3, 3)}
# every k-th bit of the colour bases is flipped: 3 is the largest k at which MARKER, END, CODE and INDEX still fail
# at every position of the MCU in both bases (test_unscan_built_host.py asserts it); every bit is 20,392 cases
FLIP_EVERY = 3


def base_colour(sampling):
    """(components, scan, offsets) of the colour base of this sampling (1,254 and 1,295 bytes)."""
    shapes, ri = COLOUR[sampling]
    comps = [sparse_blocks(s, 50 + i, density=0.5) for i, s in enumerate(shapes)]
    data, offs = J.encode(comps, sampling, ri)
    return comps, data, offs


def _case(name, data, offsets=None, sampling="grey", shapes=None, ri=GREY_RI, after=None):
    case = dict(name=name, data=bytes(data), sampling=sampling, shapes=shapes or GREY_SHAPES, ri=ri, offsets=offsets)
    if after is not None:
        case["after"] = after
    return case


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


def _dc_scan(name, sampling, shapes, diff):
    """One interval whose DC differences are diff(component, n) for the n-th block of the component in scan
    order, every AC coefficient 0 (int64 blocks: the predictors may leave int16, which is the point)."""
    comps = [np.zeros(tuple(s) + (64,), np.int64) for s in shapes]
    pred, count = [0, 0, 0], [0, 0, 0]
    for c, r, col in J.mcu_order(sampling, shapes)[0]:
        pred[c] += diff(c, count[c])
        count[c] += 1
        comps[c][r, col, 0] = pred[c]
    data, _ = J.encode(comps, sampling, 0)
    return _case(name, data, None, sampling, shapes, 0)


def dc_colour_cases():
    """The predictor of one component alone leaves int16 at its 17th +2047 (Cb: block 16 * 3 + 1, Cr: 16 * 3 + 2
    of a 4:4:4 interval; Y: after three differences of 0 the 17th is Y block 19, position 3 of MCU 4 of a 4:2:0
    interval, block 27), the other predictors stay within 17; and clean scans in which all three reach exactly
    32767 = 16 * 2047 + 15 and exactly -32768 = -16 * 2047 - 16 in their 17th block."""
    s444, s420 = [(3, 6)] * 3, [(4, 6), (2, 3), (2, 3)]
    small = lambda n: (1, -1, 0)[n % 3]  # noqa: E731
    return [
        _dc_scan("dc overflow in cb", "444", s444, lambda c, n: 2047 if c == 1 else small(n)),
        _dc_scan("dc overflow in cr", "444", s444, lambda c, n: 2047 if c == 2 else small(n)),
        _dc_scan("dc overflow in y at position 3", "420", s420,
                 lambda c, n: (2047 if n >= 3 else 0) if c == 0 else small(n)),
        _dc_scan("dc reaches 32767", "444", s444, lambda c, n: 2047 if n < 16 else 15 if n == 16 else -3),
        _dc_scan("dc reaches -32768", "444", s444, lambda c, n: -2047 if n < 16 else -16 if n == 16 else 3),
    ]


def _flipped(data, bit):
    d = bytearray(data)
    d[bit >> 3] ^= 0x80 >> (bit & 7)
    return d


def colour_cases(sampling):
    """What build() does to the grey base, done to the colour base of this sampling."""
    shapes, ri = COLOUR[sampling]
    _, data, offs = base_colour(sampling)
    kw = dict(sampling=sampling, shapes=shapes, ri=ri)
    tag = sampling + " "
    cases = [_case(tag + "clean located", data, **kw), _case(tag + "clean offsets", data, list(offs), **kw)]
    for bit in range(0, 8 * len(data), FLIP_EVERY):
        cases.append(_case(tag + "flip %d" % bit, _flipped(data, bit), **kw))
    for n in range(len(data)):
        cases.append(_case(tag + "truncated to %d" % n, data[:n], **kw))
    for bit in range(0, 8 * len(data), 7):
        cases.append(_case(tag + "flip %d, offsets" % bit, _flipped(data, bit), list(offs), **kw))
    for n in range(0, len(data), 5):
        cases.append(_case(tag + "truncated to %d, offsets" % n, data[:n], list(offs), **kw))
    for j, p in enumerate(U.markers(data)):
        cases.append(_case(tag + "marker %d deleted" % j, data[:p] + data[p + 2:], **kw))
        cases.append(_case(tag + "marker %d duplicated" % j, data[:p] + data[p:p + 2] + data[p:], **kw))
        for number in (0, 3, 7):
            d = bytearray(data)
            d[p + 1] = 0xd0 + number
            cases.append(_case(tag + "marker %d renumbered %d" % (j, number), d, **kw))
    cases.append(_case(tag + "ff as last byte", data[:-1] + b"\xff", **kw))
    cases.append(_case(tag + "ff appended", data + b"\xff", **kw))
    cases.append(_case(tag + "marker appended", data + b"\xff\xd2", **kw))
    cases.append(_case(tag + "no bytes", b"", **kw))
    cases.append(_case(tag + "one ff", b"\xff", **kw))
    cases.append(_case(tag + "all markers", b"\xff\xd0" * 40, **kw))
    return cases


def next_byte_cases():
    """Each base with FF as its last byte and D0..D7 as the byte after the scan: FF Dn would be a marker, but its
    second byte is not the scan's.  Also with the offsets given, and the scan of a single FF."""
    cases = []
    for sampling in ("grey", "420", "444"):
        if sampling == "grey":
            (_, data, offs), kw = base_grey(), {}
        else:
            _, data, offs = base_colour(sampling)
            kw = dict(sampling=sampling, shapes=COLOUR[sampling][0], ri=COLOUR[sampling][1])
        for n in range(8):
            cases.append(_case("%s ends ff, next byte d%d" % (sampling, n), data[:-1] + b"\xff", after=0xd0 + n, **kw))
        cases.append(_case("%s ends ff, next byte d0, offsets" % sampling, data[:-1] + b"\xff", list(offs),
                           after=0xd0, **kw))
        cases.append(_case("%s one ff, next byte d5" % sampling, b"\xff", after=0xd5, **kw))
    return cases


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
    for sampling in ("420", "444"):
        cases += colour_cases(sampling)
    cases += dc_colour_cases()
    cases += next_byte_cases()
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
