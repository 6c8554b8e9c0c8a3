"""Scans built for the split entropy decoder's tests (a helper: no test in it),
in the form of tests/unscan_corpus.py's cases.  Nothing here asks the library
but for its geometry, which the callers pass in: S bytes a segment, G segments a
group, R launches between groups.  test_unscan_split_host.py proves each input
from its bytes before test_gpu_unscan_split.py uses it.

Every scan but the colour ones is grey and one interval (restart_interval 0).
"""
import functools

import numpy as np

import jpeg_scan as J
import unscan_corpus

MAX_BLOCK_BYTES = 415                                   # 63 codes of 16 bits and 10 extra bits, the DC, stuffed


def _case(name, blocks_per_component, sampling="grey", ri=0, offsets=None, data=None):
    shapes = [tuple(b.shape[:2]) for b in blocks_per_component]
    if data is None:
        data, _ = J.encode(blocks_per_component, sampling, ri)
    case = unscan_corpus._case(name, data, offsets, sampling, shapes, ri)
    case["blocks"] = blocks_per_component
    return case


@functools.lru_cache(maxsize=None)
def limits(S, G, R):
    """Grey, one interval, the first n blocks of one row of unscan_corpus.sparse_blocks: for each of S, 2 S, G S
    and (R + 1) G S bytes the longest scan of at most that many bytes and the shortest of more (each within a
    block's length of it), and the shortest scan of more than R groups.  -> [(case, whether it has at most
    R + 1 groups: the bound under which every interval settles)]; built once per process, read-only."""
    nmax = ((R + 1) * G * S + 2 * MAX_BLOCK_BYTES) // 24   # a sparse block is well above 24 bytes
    row = unscan_corpus.sparse_blocks((1, nmax), 1234)
    scans = {}

    def scan(n):
        if n not in scans:
            scans[n] = J.encode([row[:, :n]], "grey", 0)[0]
        return scans[n]

    out = []
    for target in (S, 2 * S, G * S, R * G * S, (R + 1) * G * S):
        lo, hi = 1, nmax                                # len(scan(lo)) <= target < len(scan(hi))
        assert len(scan(lo)) <= target < len(scan(hi)), (target, len(scan(hi)))
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if len(scan(mid)) <= target else (lo, mid)
        for n in ((hi,) if target == R * G * S else (lo, hi)):
            c = _case("limit %d bytes, %d blocks" % (target, n), [row[:, :n].copy()], data=scan(n))
            c["target"] = target
            out.append((c, len(c["data"]) <= (R + 1) * G * S))
    return out


# ---------------------------------------------------------------------------
# one feature at each byte offset -2 .. +2 around a segment boundary
# ---------------------------------------------------------------------------
_DC, _AC = J.codes_of(J.DC_LUMA), J.codes_of(J.AC_LUMA)


def block_bits(b):
    """The bits of a grey block whose DC difference is b[0] (no padding, no stuffing)."""
    n = _DC[J._category(b[0])][1] + J._category(b[0])
    run = 0
    for k in range(1, 64):
        if b[k] == 0:
            run += 1
            continue
        n += (run // 16) * _AC[0xf0][1]
        size = J._category(b[k])
        n += _AC[((run % 16) << 4) | size][1] + size
        run = 0
    return n + (_AC[0x00][1] if run else 0)


def _bits_of(b):
    """(the bits of the block as an integer, their number)."""
    plain = J.encode([b[None, None]], "grey", 0)[0].replace(b"\xff\x00", b"\xff")
    n = block_bits(b)
    return int.from_bytes(plain, "big") >> (8 * len(plain) - n), n


def raw_byte_of_bit(data, bit):
    """The raw byte of a stuffed scan that holds data bit `bit`."""
    plain = bytes(data).replace(b"\xff\x00", b"\xff")
    return bit // 8 + plain[:bit // 8].count(0xff)


def _filler(rng, dc=0):
    """A block of a few small coefficients, DC difference 0: 2 to 8 bytes."""
    b = np.zeros(64, np.int16)
    for k in rng.choice(np.arange(1, 20), size=int(rng.integers(2, 6)), replace=False):
        b[k] = rng.integers(1, 7) * rng.choice([-1, 1])
    return b


# the feature's block (DC differences are 0 around it: every block here has DC 0 but "dc" and "extra", which are
# followed by a block that returns to 0) and the bit of the block at which the feature starts
FEATURES = {
    "ff00": (lambda: _set({1: 1023, 2: 1023, 3: 1023, 4: 1023}), None),    # runs of 19 ones: aligned FF bytes
    "code16": (lambda: _set({11: 700}), 2),                 # after the DC's 00: (run 10, size 10), 16 bits
    "extra": (lambda: _set({0: -2047}), 9),                 # the 11 extra bits of the largest DC difference
    "dc": (lambda: _set({0: 100}), 0),
    "eob": (lambda: _set({1: 1}), 5),                       # DC 00, (0, 1) 00 and its bit, then EOB
    "zrl": (lambda: _set({40: 3}), 2),                      # DC 00, then the first of two ZRLs
    "last": (None, None),
}


def _set(values):
    b = np.zeros(64, np.int16)
    for k, v in values.items():
        b[k] = v
    return b


def feature_byte(case):
    """From the case's blocks and bytes: the raw byte at which its feature starts."""
    kind, data = case["feature"], case["data"]
    if kind == "last":
        return len(data) - 1
    if kind == "ff00":                                  # the pair at the place the case names, if there is one
        at = case["boundary"] + case["offset"]
        return at if data[at:at + 2] == b"\xff\x00" else -1
    blocks = case["blocks"][0][0]
    diffs = np.diff(np.concatenate([[0], blocks[:, 0].astype(np.int64)]))
    bit = 0
    for j in range(case["feature_block"]):
        b = blocks[j].copy()
        b[0] = diffs[j]
        bit += block_bits(b)
    return raw_byte_of_bit(data, bit + FEATURES[kind][1])


@functools.lru_cache(maxsize=None)
def boundaries(S):
    """For each feature and each offset -2 .. +2 a scan in which the feature starts at that offset from the segment
    boundary 2 S (feature_byte(case) == 2 S + offset): the first byte of a 16-bit code, of 11 extra bits, of a DC
    symbol, of an EOB and of a ZRL, the FF of an FF 00 pair (offset -1: the 00 is a segment's first
    byte) and the interval's last byte.  A shim block and fillers in front shift it there, fillers follow it.
    The longest extra bits the Annex K tables code are 11 (DC) and 10 (AC): there are no 15.  -> [case]"""
    rng = np.random.default_rng(77)
    fillers = [_filler(rng) for _ in range(S)]
    cum = np.concatenate([[0], np.cumsum([block_bits(f) for f in fillers])])
    acc = [0]
    for f in fillers:
        v, n = _bits_of(f)
        acc.append((acc[-1] << n) | v)
    shims = [_set({1: v}) for v in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)] + \
            [_set({1: v, 2: w}) for v in (1, 4, 16, 64) for w in (1, 4, 16, 64)]
    shim_bits = [_bits_of(x) for x in shims]
    out = []
    for kind, (make, _) in FEATURES.items():
        for off in range(-2, 3):
            found = None
            for n in range(len(fillers)):
                if int(cum[n]) // 8 > 2 * S + 8:
                    break
                for shim, (sv, sn) in zip(shims, shim_bits):
                    # where the block after the fillers starts, from the bits alone: only near the boundary is the
                    # scan written out and the feature looked up in its bytes
                    nbits = sn + int(cum[n])
                    stream = (((sv << int(cum[n])) | acc[n]) << (-nbits % 8)).to_bytes((nbits + 7) // 8, "big")
                    start = nbits // 8 + stream[:nbits // 8].count(0xff)
                    if not 2 * S + off - 16 <= start <= 2 * S + off:
                        continue
                    front = [shim] + fillers[:n]
                    blocks = front + ([] if kind == "last" else [make()])
                    if kind in ("dc", "extra"):
                        back = _set({0: blocks[-1][0]})      # the same DC again: difference 0 from here on
                        blocks += [back + f for f in fillers[n:n + 30]]
                        blocks[len(front)][0] = make()[0]
                    elif kind != "last":
                        blocks += fillers[n:n + 30]
                    c = _case("boundary %s %+d" % (kind, off), [np.stack(blocks)[None].astype(np.int16)])
                    c["feature"], c["offset"], c["feature_block"], c["boundary"] = kind, off, len(front), 2 * S
                    if feature_byte(c) == 2 * S + off:
                        found = c
                        break
                if found:
                    break
            assert found is not None, (kind, off)
            out.append(found)
    return out


def whole_segment_block(S):
    """A block whose bytes cover a whole segment, so that the segment completes no block: DC 0 and all 63
    coefficients 1023 (317 bytes with its stuffing), behind as many fillers as put its first bit at most 40 bytes
    before a segment boundary; fillers follow.  -> case, with "big" = (the raw byte of the block's first bit, of
    the first bit after it), from block_bits() and the bytes."""
    rng = np.random.default_rng(5)
    big = _set({k: 1023 for k in range(1, 64)})
    fillers = [_filler(rng) for _ in range(S // 2 + 40)]
    for n in range(S // 8, S // 2):
        blocks = fillers[:n] + [big] + fillers[n:n + 30]
        c = _case("a block that covers a segment", [np.stack(blocks)[None].astype(np.int16)])
        first = sum(block_bits(f) for f in fillers[:n])
        c["big"] = (raw_byte_of_bit(c["data"], first), raw_byte_of_bit(c["data"], first + block_bits(big)))
        boundary = -(-c["big"][0] // S) * S
        if boundary - c["big"][0] <= 40 and c["big"][1] > boundary + S:
            return c
    raise AssertionError("no placement found")


# ---------------------------------------------------------------------------
# slow convergence
# ---------------------------------------------------------------------------
def dense(sampling, nbytes, seed=9):
    """Every coefficient non-zero (no EOB at all), values of sizes 8-10: blocks of some 200 bytes, a scan of at
    least nbytes bytes."""
    rng = np.random.default_rng(seed)
    n = nbytes // 150 + 8
    if sampling == "grey":
        shapes = [(1, n)]
    else:
        m = -(-n // 6)
        shapes = [(2, 2 * m), (1, m), (1, m)]

    def comp(shape):
        b = rng.integers(130, 1024, shape + (64,)) * rng.choice([-1, 1], shape + (64,))
        b[..., 0] = rng.integers(-200, 201, shape)
        return b.astype(np.int16)
    c = _case("dense %s" % sampling, [comp(s) for s in shapes], sampling)
    assert len(c["data"]) >= nbytes
    return c


def half(nbytes, seed=21):
    """4:2:0, half the coefficients non-zero, small values: at least nbytes bytes."""
    n = nbytes // 40 + 6
    m = -(-n // 6)
    shapes = [(2, 2 * m), (1, m), (1, m)]
    comps = [unscan_corpus.sparse_blocks(s, seed + i, density=0.5, top=60) for i, s in enumerate(shapes)]
    c = _case("half 420", comps, "420")
    assert len(c["data"]) >= nbytes
    return c


def stubborn(S, G, R, settles):
    """A grey interval that never falls into step: every symbol is 4 bits, 0100 or 0101 -- a DC difference of -1 or
    +1, and the AC symbol (run 0, size 2) with the value -3 or -2 -- and each reads as the other kind as well (0100
    is the DC code 010 and the bit 0, or the AC code 01 and the bits 00), so a walk that starts at a segment's
    boundary as if a block began there decodes valid symbols for ever, its block ends 52 coefficients from the
    true ones: the first block has ten coefficients and an EOB (6 bytes), every other one all 63 (32 bytes), and
    S is a multiple of 32.  Only the true start is right, and each launch carries it one group further:
    settles: the longest such scan of at most (R + 1) G S bytes, which settles in R launches exactly; else the
    shortest of more, R + 2 groups, which cannot.  -> case"""
    assert S % 32 == 0
    n = ((R + 1) * G * S - 6) // 32 + (0 if settles else 1)
    rng = np.random.default_rng(12)
    blocks = rng.choice([-3, -2], (1, n + 1, 64)).astype(np.int16)
    blocks[0, 0, 11:] = 0
    blocks[0, :, 0] = np.arange(1, n + 2) % 2             # DC 1, 0, 1, ...: differences +1, -1, +1, ...
    c = _case("stubborn, %s" % ("settles" if settles else "does not settle"), [blocks])
    assert len(c["data"]) == 6 + 32 * n and b"\xff" not in c["data"]
    return c


def overlapping(S, n=64):
    """Grey, one block per interval, n intervals, and an offsets table 0, B, 0, B, ... (B the scan's length): every
    even interval claims the whole scan, [0, B - 2), every odd one is out of range, and the segments asked for,
    n / 2 * ceil((B - 2) / S), exceed the budget of ceil(B / S) + n."""
    blocks = unscan_corpus.sparse_blocks((1, n), 8)
    data, _ = J.encode([blocks], "grey", 1)
    table = [0 if i % 2 == 0 else len(data) for i in range(n + 1)]
    return _case("overlapping offsets", [blocks], ri=1, offsets=table, data=data)
