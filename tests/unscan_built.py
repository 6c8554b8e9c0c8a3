"""Scans built for the entropy decoder's tests, blocks and bytes together (a
helper: no test in it).  Nothing here asks the library: the bytes come from
jpeg_scan._Bits and jpeg_scan.encode, the expectations from construction or
from tests/jpeg_unscan.py.

- catalogue(sampling): a clean scan in which every symbol of the Annex K tables
  starts at every bit phase 0..7 of its interval's bit stream, and every size's
  extra bits are all zeros once and all ones once; trace() recounts that from
  the blocks alone;
- as_420(): the catalogue's blocks laid out as a 4:2:0 frame;
- stuffed(): a grey scan of one block per interval, dense in FF 00 pairs, with
  interval lengths 2..24; pair_phases() says where its pairs lie for the eight
  addresses a buffer can start at;
- marker_cases(): the catalogue's grey blocks at one block per interval with
  FF Dn pairs written over the edges of the marker search's steps and chunks;
- far_markers(): the grey corpus base behind so many zero bytes that its
  markers lie in the search's second turn.
"""
import functools

import numpy as np

import jpeg_scan as J
import jpeg_unscan as U
import unscan_corpus

MCUS_PER_INTERVAL = 8
CHUNK = 4096                                            # unscan::kChunkBytes
LOCATE_WAVES = 4 * 8192                                 # the locate kernels' grid cap, four waves a workgroup


def all_combinations(kinds):
    """Every (kind, symbol, phase) of the tables `kinds`."""
    return {(k, s, p) for k in kinds for s in J.TABLES[k][1] for p in range(8)}


def _extra(v, n):
    return v if v > 0 else v + (1 << n) - 1


class _Interval:
    """One interval being written: the bits, the bit count and the predictors."""

    def __init__(self):
        self.w, self.at, self.pred = J._Bits(), 0, [0, 0, 0]

    def put(self, code, length):
        self.w.put(code, length)
        self.at += length


@functools.lru_cache(maxsize=None)
def catalogue(sampling="444", limit=40000):
    """-> dict(data, offsets, components, shapes, sampling, ri, seen, extremes), built once per process and
    shared by the tests: treat it as read-only.

    4:4:4 (one Y, Cb, Cr block per MCU) or grey, 8 MCUs per interval.  A block is a DC difference of a chosen
    category, up to three ZRLs, one AC symbol with a value and EOB unless coefficient 63 was written.  The choice
    is directed: of the categories and ZRL counts, take the one that starts the most codes still missing at their
    phase.  DC differences take the sign that brings the predictor back towards 0, so |DC| <= 2047 throughout.
    seen: the (kind, symbol, phase) written; extremes: the (kind, size, 0 or 1) of extra bits all zeros / all ones."""
    ncomp = 1 if sampling == "grey" else 3
    codes = [J.codes_of(t) for t in J.TABLES]
    need = all_combinations((0, 1) if ncomp == 1 else (0, 1, 2, 3))
    missing = {(k, p): sorted(s for (kk, s, pp) in need if kk == k and pp == p) for k in range(4) for p in range(8)}
    seen, extremes = set(), set()
    blocks = [[] for _ in range(ncomp)]
    data, offsets = bytearray(), []
    cur, mcus, turn = None, 0, 0

    def mark(kind, sym, phase):
        if (kind, sym, phase) not in seen:
            seen.add((kind, sym, phase))
            if sym in missing[(kind, phase)]:
                missing[(kind, phase)].remove(sym)

    while len(seen) < len(need) or mcus % MCUS_PER_INTERVAL != 0:
        assert mcus < limit, "the directed choice does not converge"
        if mcus % MCUS_PER_INTERVAL == 0:
            if cur is not None:
                data += cur.w.finish() + bytes([0xff, 0xd0 + ((len(offsets) - 1) & 7)])
            offsets.append(len(data))
            cur = _Interval()
        for c in range(ncomp):
            dk = 2 if c else 0
            ak = dk + 1
            zrl_len = codes[ak][0xf0][1]
            p = cur.at & 7
            best = None
            for cat in range(12):
                for z in range(4):
                    q = (p + codes[dk][cat][1] + cat + z * zrl_len) & 7
                    pending = [s for s in missing[(ak, q)] if s & 15 and 1 + 16 * z + (s >> 4) <= 63]
                    score = 4 * bool(pending) + 2 * ((dk, cat, p) not in seen)
                    score += sum((ak, 0xf0, (p + codes[dk][cat][1] + cat + i * zrl_len) & 7) not in seen
                                 for i in range(z))
                    if pending:
                        s = pending[0]
                        full = 1 + 16 * z + (s >> 4) == 63
                        score += (not full) and (ak, 0x00, (q + codes[ak][s][1] + (s & 15)) & 7) not in seen
                    # ties: turn over the categories and the ZRL counts, so that the phase keeps moving
                    key = (score, -((cat + 5 * z + turn) % 48))
                    if best is None or key > best[0]:
                        best = (key, cat, z, pending[0] if pending else None)
            _, cat, z, sym = best
            turn += 1
            if sym is None:                             # nothing missing starts here: any symbol, the phase moves on
                usable = [s for s in J.TABLES[ak][1] if s & 15 and 1 + 16 * z + (s >> 4) <= 63]
                sym = usable[turn % len(usable)]
            blk = np.zeros(64, np.int64)
            # the DC difference: the magnitudes 2^n - 1 (both signs: every extra bit 1, every extra bit 0), 2^(n-1)
            # and one between, in turn; the sign against the predictor
            pred = cur.pred[c]
            top, low = (1 << cat) - 1, 1 << (cat - 1) if cat else 0
            mag = 0 if cat == 0 else [top, low, (top + low) // 2][turn % 3]
            if (dk, cat, 1) not in extremes or (dk, cat, 0) not in extremes:
                mag = (1 << cat) - 1 if cat else 0
            diff = -mag if pred > 0 or (pred == 0 and turn & 1) else mag
            mark(dk, cat, cur.at & 7)
            cur.put(*codes[dk][cat])
            if cat:
                cur.put(_extra(diff, cat), cat)
                if abs(diff) == (1 << cat) - 1:
                    extremes.add((dk, cat, int(diff > 0)))
            cur.pred[c] = blk[0] = pred + diff
            k = 1
            for _ in range(z):
                mark(ak, 0xf0, cur.at & 7)
                cur.put(*codes[ak][0xf0])
                k += 16
            run, n = sym >> 4, sym & 15
            k += run
            want = [b for b in (1, 0) if (ak, n, b) not in extremes]
            if want:
                v = (1 << n) - 1 if want[0] else -((1 << n) - 1)
                extremes.add((ak, n, want[0]))
            else:
                v = [(1 << n) - 1, -(1 << (n - 1)), 1 << (n - 1), -((1 << n) - 1)][turn % 4]
            mark(ak, sym, cur.at & 7)
            cur.put(*codes[ak][sym])
            cur.put(_extra(v, n), n)
            blk[k] = v
            if k < 63:
                mark(ak, 0x00, cur.at & 7)
                cur.put(*codes[ak][0x00])
            blocks[c].append(blk)
        mcus += 1
    data += cur.w.finish()
    offsets.append(len(data))
    shape = (mcus // MCUS_PER_INTERVAL, MCUS_PER_INTERVAL)
    comps = [np.asarray(b, np.int16).reshape(shape + (64,)) for b in blocks]
    return dict(data=bytes(data), offsets=offsets, components=comps, shapes=[shape] * ncomp, sampling=sampling,
                ri=MCUS_PER_INTERVAL, seen=seen, extremes=extremes)


def trace(components, sampling, ri):
    """What a baseline coder writes for these blocks, recounted without the builder: the (kind, symbol, phase) of
    every code and the (kind, size, 0 or 1) of every run of extra bits that is all zeros or all ones."""
    comps = [np.asarray(c).astype(np.int64) for c in components]
    order, bpm = J.mcu_order(sampling, J._shapes(components, sampling))
    per = (len(order) // bpm if ri == 0 else ri) * bpm
    codes = [J.codes_of(t) for t in J.TABLES]
    seen, extremes = set(), set()
    at, pred = 0, [0, 0, 0]

    def put(kind, sym, value=None):
        nonlocal at
        seen.add((kind, sym, at & 7))
        n = sym & 15 if kind & 1 else sym
        at += codes[kind][sym][1] + (n if value is not None else 0)
        if value is not None and n and abs(value) == (1 << n) - 1:
            extremes.add((kind, n, int(value > 0)))

    for i, (c, r, col) in enumerate(order):
        if i % per == 0:
            at, pred = 0, [0, 0, 0]
        blk, dk = comps[c][r, col], 2 if c else 0
        d = int(blk[0]) - pred[c]
        pred[c] = int(blk[0])
        put(dk, J._category(d), d)
        run = 0
        for v in blk[1:]:
            if v == 0:
                run += 1
                continue
            while run >= 16:
                put(dk + 1, 0xf0)
                run -= 16
            put(dk + 1, (run << 4) | J._category(v), int(v))
            run = 0
        if run:
            put(dk + 1, 0x00)
    return seen, extremes


def as_420(built):
    """The 4:4:4 catalogue's blocks as a 4:2:0 frame, 2 MCUs per interval: Y (2r, 8), chroma (r, 4), each
    component's blocks taken cyclically in the order the scan visits them; r is such that every chroma block is
    taken once and every Y block four times.  An interval holds 8 Y blocks and 2 of each chroma, and the lists
    hold multiples of 8, so a list wraps at an interval's start only and every DC difference inside an interval
    is one the catalogue had or a block's own DC (|DC| <= 2047)."""
    lists = [c.reshape(-1, 64) for c in built["components"]]
    r = -(-len(lists[1]) // 4)
    shapes = [(2 * r, 8), (r, 4), (r, 4)]
    comps = [np.zeros(s + (64,), np.int16) for s in shapes]
    order, _ = J.mcu_order("420", shapes)
    count = [0, 0, 0]
    for c, row, col in order:
        comps[c][row, col] = lists[c][count[c] % len(lists[c])]
        count[c] += 1
    return comps, shapes, 2


# ---------------------------------------------------------------------------
# stuffing and the reader's word cache
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stuffed():
    """-> (blocks, data, offsets), built once per process: grey, one block per interval.  Candidates are drawn
    (seeded) from blocks that code long runs of 1 bits -- DC differences of +2047 (the code's nine bits start FF),
    AC values of +1023 and 2^n - 1, some with a last coefficient 2^n - 1, which needs no EOB and ends the interval
    on FF 00 -- and short plain ones; then for every interval length 2..24 bytes the candidates richest in FF are
    kept, and every kind of first and last pair."""
    rng = np.random.default_rng(77)
    cands = []
    for i in range(3000):
        blk = np.zeros(64, np.int64)
        style = i % 4
        blk[0] = [2047, 2047, int(rng.integers(-2047, 2048)), int(rng.choice([0, 1, -1, 255, -1024]))][style]
        if style == 3:
            for k in rng.choice(np.arange(1, 64), int(rng.integers(0, 3)), replace=False):
                blk[k] = int(rng.choice([1, -1, 3, 1023]))
        else:
            for k in rng.choice(np.arange(1, 63), int(rng.integers(0, 7)), replace=False):
                blk[k] = int(rng.choice([1023, 1023, 511, 255, 127, -1023, 1]))
            if rng.random() < 0.5:
                blk[63] = (1 << int(rng.integers(1, 11))) - 1
        coded, _ = J.encode([blk.reshape(1, 1, 64)], "grey", 0)
        if 2 <= len(coded) <= 24:
            cands.append((blk, coded))
    chosen = []
    for length in range(2, 25):
        of_len = sorted((c for c in cands if len(c[1]) == length), key=lambda c: -c[1].count(b"\xff"))
        assert of_len, length
        chosen += of_len[:6]
        chosen += [c for c in of_len[6:] if c[1].endswith(b"\xff\x00")][:3]
        chosen += [c for c in of_len[6:] if c[1].startswith(b"\xff\x00")][:3]
    # every distance 0..7 from an interval's first byte to a pair's FF
    for d in range(8):
        chosen += [c for c in cands if any(c[1][p] == 0xff and p % 8 == d for p in range(len(c[1])))][:2]
    blocks = np.asarray([c[0] for c in chosen], np.int16).reshape(1, len(chosen), 64)
    data, offsets = J.encode([blocks], "grey", 1)
    return blocks, data, offsets


def pair_phases(data, offsets):
    """Where the FF 00 pairs of a one-block-per-interval scan lie when its first byte is at each address s = 0..7
    (mod 8): -> (all, first, last): the (a, w) of every pair, a the address of its interval's first byte and w
    the address of its FF, both mod 8; the a for which a pair lies wholly in the first 8 bytes of its interval;
    the a for which one lies wholly in the last 8."""
    every, first, last = set(), set(), set()
    n = len(offsets) - 1
    for i in range(n):
        lo, hi = offsets[i], offsets[i + 1] - (0 if i + 1 == n else 2)
        for p in range(lo, hi - 1):
            if data[p] == 0xff and data[p + 1] == 0x00:
                for s in range(8):
                    a = (s + lo) & 7
                    every.add((a, (s + p) & 7))
                    if p + 2 <= lo + 8:
                        first.add(a)
                    if p >= hi - 8:
                        last.add(a)
    return every, first, last


# ---------------------------------------------------------------------------
# the marker search
# ---------------------------------------------------------------------------
def grey_single(built):
    """The grey catalogue's blocks at one block per interval: (shapes, data, offsets)."""
    assert built["sampling"] == "grey"
    data, offsets = J.encode(built["components"], "grey", 1)
    return built["shapes"], data, offsets


def marker_cases(built):
    """-> [(name, data, position of the written FF)]: FF Dn written over two bytes of the grey one-block-per-
    interval scan (the restatement says what that makes of it), with the number that is the marker's turn and
    with another; one FF as the last byte; 3,000 FF D0 pairs in front of the scan (a chunk holds 2,048 of them:
    the first chunk is nothing but markers, the second starts with 952)."""
    _, data, _ = grey_single(built)
    n = len(data)
    assert n > 2 * CHUNK + 64
    places = [("byte 63", 63), ("byte 191", 191), ("byte 4094", CHUNK - 2), ("byte 4095", CHUNK - 1),
              ("byte 4096", CHUNK), ("byte 8191", 2 * CHUNK - 1), ("bytes - 2", n - 2)]
    out = []
    for name, p in places:
        for right in (True, False):
            d = bytearray(data)
            d[p:p + 2] = b"\xff\xd0"
            j = U.markers(d).index(p)
            d[p + 1] = 0xd0 + ((j if right else j + 3) & 7)
            out.append(("marker at %s, %s number" % (name, "its" if right else "a wrong"), bytes(d), p))
    d = bytearray(data)
    d[n - 1] = 0xff
    out.append(("ff at bytes - 1", bytes(d), n - 1))
    out.append(("3000 markers first", b"\xff\xd0" * 3000 + data, 0))
    return out


def far_markers():
    """-> (zeros, base blocks, base scan): the grey corpus base (3 x 7 blocks, 2 per interval, 10 markers) behind
    `zeros` zero bytes, so that marker 0 has its FF in the last byte of chunk 32767 and its number in chunk 32768:
    one more chunk than the locate kernels have waves, the rank kernel's threads own 33 chunks each."""
    blocks, data, _ = unscan_corpus.base_grey()
    zeros = LOCATE_WAVES * CHUNK - 1 - U.markers(data)[0]
    return zeros, blocks, data


def far_expected(zeros, data):
    """What the restatement makes of zeros + data, interval by interval (the 128 MiB are never searched on the
    host): (blocks, status, markers_found, marker_errors)."""
    mk = U.markers(data)
    shapes, ri = unscan_corpus.GREY_SHAPES, unscan_corpus.GREY_RI
    out = np.zeros(shapes[0] + (64,), np.int16).reshape(-1, 64)
    bounds = [0] + [p + 2 for p in mk], mk + [len(data)]
    status = np.zeros(len(mk) + 1, np.uint64)
    for i, (lo, hi) in enumerate(zip(*bounds)):
        chunk = (bytes(zeros) if i == 0 else b"") + data[lo:hi]
        nblk = min(ri, len(out) - ri * i)
        got, status[i] = U._walk(chunk, (0,) * nblk)
        for j, blk in enumerate(got):
            out[ri * i + j] = blk
    errors = sum(1 for j, p in enumerate(mk) if (data[p + 1] & 7) != j % 8)   # all are below intervals - 1
    return [out.reshape(shapes[0] + (64,))], status, len(mk), errors


# ---------------------------------------------------------------------------
# the same scans as corpus cases, for the walker on the CPU under the sanitizers
# ---------------------------------------------------------------------------
def corpus_cases():
    """The built scans in the form of tests/unscan_corpus.py's cases: the catalogues (markers located and offsets
    given), the 4:2:0 arrangement, the stuffed scan and the marker cases."""
    case = unscan_corpus._case
    out = []
    for sampling in ("444", "grey"):
        b = catalogue(sampling)
        kw = dict(sampling=sampling, shapes=b["shapes"], ri=b["ri"])
        out += [case("catalogue %s located" % sampling, b["data"], **kw),
                case("catalogue %s offsets" % sampling, b["data"], list(b["offsets"]), **kw)]
    comps, shapes, ri = as_420(catalogue("444"))
    data, offs = J.encode(comps, "420", ri)
    out += [case("catalogue 420 located", data, sampling="420", shapes=shapes, ri=ri),
            case("catalogue 420 offsets", data, list(offs), sampling="420", shapes=shapes, ri=ri)]
    blocks, data, offs = stuffed()
    shapes = [tuple(blocks.shape[:2])]
    out += [case("stuffed located", data, shapes=shapes, ri=1),
            case("stuffed offsets", data, list(offs), shapes=shapes, ri=1)]
    shapes = catalogue("grey")["shapes"]
    out += [case(name, data, shapes=shapes, ri=1) for name, data, _ in marker_cases(catalogue("grey"))]
    return out
