"""hpdct_decode_scan_split restated in plain Python (a helper: no test in it):
jpeg_unscan.decode plus the plan, the segment walk, the group rule and the
launches between groups of cuda-dct-idct_amd/csrc/hpdct_unscan_split.hpp.

decode(data, sampling, shapes, restart_interval, offsets=None, split_min_bytes=0, geometry=None)
    -> (components, status, markers_found, marker_errors, counts)

The first four are what jpeg_unscan.decode returns -- the blocks of an interval
that passes every check are taken from the segment walks here, not from
jpeg_unscan -- and counts = {"split_intervals", "serial_intervals",
"unsettled_intervals", "rounds"}, exact because the settling is deterministic:
a group's state after a launch depends only on the bytes and on its predecessor
group's last exit after the launch before.

geometry: (segment bytes, segments of a group, launches between groups), by
default GEOMETRY, which test_unscan_split_host.py holds against the library's.
The reader below fetches as hpdct_unscan.hpp's does (whole bytes, up to 32 bits
ahead); nothing it returns depends on how far ahead it fetches.
"""
import numpy as np

import jpeg_scan as J
import jpeg_unscan as U

GEOMETRY = (256, 256, 4)
DEFAULT_MIN_BYTES = 3328
M64 = (1 << 64) - 1

_LOOK = [{(ln, code): sym for sym, (code, ln) in J.codes_of(t).items()} for t in J.TABLES]   # kinds 0..3


class _Reader:
    __slots__ = ("d", "pos", "hi", "acc", "avail", "err")

    def __init__(self, d, pos, hi):
        self.d, self.pos, self.hi, self.acc, self.avail, self.err = d, pos, hi, 0, 0, 0

    def fill(self):
        for _ in range(4):
            if self.avail >= 32 or self.err:
                break
            if self.pos >= self.hi:
                self.err = U.END
                break
            b = self.d[self.pos]
            if b == 0xff:
                if self.pos + 1 >= self.hi:
                    self.err = U.END
                    break
                if self.d[self.pos + 1] != 0:
                    self.err = U.MARKER
                    break
                self.pos += 2
            else:
                self.pos += 1
            self.acc |= b << (56 - self.avail)
            self.avail += 8

    def take(self, n):
        v = self.acc >> (64 - n)
        self.acc = (self.acc << n) & M64
        self.avail -= n
        return v

    def symbol(self, kind):
        """(status code, symbol): the 16 bits ahead against the table, zeros beyond what was fetched."""
        self.fill()
        peek = self.acc >> 48
        look = _LOOK[kind]
        for length in range(1, 17):
            sym = look.get((length, peek >> (16 - length)))
            if sym is not None:
                if length > self.avail:
                    return self.err, 0
                self.take(length)
                return U.OK, sym
        return (U.CODE if self.avail >= 16 else self.err), 0

    def extra(self, n):
        if n == 0:
            return U.OK, 0
        if n > self.avail:
            self.fill()
            if n > self.avail:
                return self.err, 0
        return U.OK, J._extend(self.take(n), n)

    def next_bit_at(self, floor):
        """(the raw byte that holds the next bit, the bit in it)."""
        p = self.pos
        for _ in range((self.avail + 7) >> 3):
            p -= 1
            if self.d[p] == 0 and p > floor and self.d[p - 1] == 0xff:
                p -= 1
        return p, (8 - (self.avail & 7)) & 7


def boundary_entry(d, lo, hi, q, seg):
    p = lo + q * seg
    if q != 0 and p < hi and d[p] == 0 and d[p - 1] == 0xff:
        p += 1
    return (p, 0, 0, 0)


def walk_segment(d, lo, hi, end, entry, bpm, seg, events=None):
    """entry: (pos, bit, kk, k) -> (exit (pos, bit, kk, k), error flag, blocks completed, DC sums).  events: a list
    that receives ("dc", component, difference), ("ac", k, value) and ("end",) in the order of the walk."""
    pos, bit, kk, k = entry
    if pos >= end:
        return entry, False, 0, (0, 0, 0)
    r = _Reader(d, pos, hi)
    dc = [0, 0, 0]
    nblk, err = 0, False
    dead = ((hi, 0, 0, 0), True)
    if bit:
        r.fill()
        if r.avail < bit:
            return dead + (0, (0, 0, 0))
        r.take(bit)
    for _ in range(8 * seg + 32):
        if r.pos >= end and r.next_bit_at(pos)[0] >= end:
            break
        comp = (0 if kk < 4 else kk - 3) if bpm == 6 else kk
        chroma = 2 if comp else 0
        done = False
        if k == 0:
            code, sym = r.symbol(chroma)
            if code == U.END:
                pad = r.avail & 7
                if r.avail < 8 and r.pos == r.hi and (pad == 0 or (r.acc >> (64 - pad)) == (1 << pad) - 1):
                    return (hi, 0, kk, 0), err, nblk, tuple(dc)
            diff = 0
            if code == U.OK:
                code, diff = r.extra(sym)
            if code == U.OK:
                dc[comp] += diff
                if events is not None:
                    events.append(("dc", comp, diff))
                k = 1
        else:
            code, sym = r.symbol(chroma + 1)
            if code == U.OK:
                run, n = sym >> 4, sym & 15
                if n == 0:
                    if run != 15:
                        done = True
                    else:
                        k += 16
                        if k > 64:
                            code = U.INDEX
                else:
                    k += run
                    if k > 63:
                        code = U.INDEX
                    else:
                        code, v = r.extra(n)
                        if code == U.OK:
                            if events is not None:
                                events.append(("ac", k, v))
                            k += 1
        if code != U.OK:
            err = True
            if code in (U.MARKER, U.END):
                return dead + (nblk, tuple(dc))
            if code == U.CODE:
                r.take(1)
            done = True
        if done or k >= 64:
            if events is not None:
                events.append(("end",))
            nblk, k = nblk + 1, 0
            kk = kk + 1 if kk + 1 < bpm else 0
    p, b = r.next_bit_at(pos)
    return (p, b, kk, k), err, nblk, tuple(dc)


_CACHE = {}
REASONS = {}    # why intervals went to the serial walker, summed over every decode() of the process: for the tests
                # that must reach each of the serial pass's conditions


def _interval(chunk, comps, bpm, geometry):
    """One split interval: its bytes and the component of each of its blocks -> (unsettled, the checks it fails,
    rounds, blocks or None).  Positions are relative to the interval's start.  Remembered, as jpeg_unscan's walk is."""
    key = (chunk, comps, bpm, geometry)
    if key not in _CACHE:
        _CACHE[key] = _settle(chunk, comps, bpm, geometry)
    return _CACHE[key]


def _settle(d, comps, bpm, geometry):
    seg, group, rounds_max = geometry
    hi = len(d)
    nseg = -(-hi // seg)
    ngrp = -(-nseg // group)
    end = lambda q: min((q + 1) * seg, hi)  # noqa: E731
    walks = [None] * nseg                   # per segment: (entry, exit, err, nblk, dc)

    def chain(g, entry):
        for q in range(g * group, min((g + 1) * group, nseg)):
            ex, err, nblk, dc = walk_segment(d, 0, hi, end(q), entry, bpm, seg)
            walks[q] = (entry, ex, err, nblk, dc)
            entry = ex
        return (ex, err, nblk)              # the group's last exit, flag and count included

    # launch 0: every group from its boundary
    gentry = [boundary_entry(d, 0, hi, g * group, seg) for g in range(ngrp)]
    glast = [chain(g, gentry[g]) for g in range(ngrp)]
    rounds = 0
    for launch in range(1, rounds_max + 1):
        before = list(glast)
        for g in range(1, ngrp):
            pred = before[g - 1][0]
            if pred != gentry[g]:
                gentry[g] = pred
                glast[g] = chain(g, pred)
                rounds = launch
    unsettled = any(gentry[g] != glast[g - 1][0] for g in range(1, ngrp))
    why = (["unsettled"] if unsettled else []) + (["error"] if any(w[2] for w in walks) else []) + \
          (["count"] if sum(w[3] for w in walks) != len(comps) else []) + \
          (["tail"] if walks[-1][1] != (hi, 0, 0, 0) else [])
    if why:
        return unsettled, why, rounds, None
    # the write walks: the first block and the predictors of a segment are sums over the segments before it
    blocks = [np.zeros(64, np.int16) for _ in comps]
    b, pred = 0, [0, 0, 0]
    for q in range(nseg):
        events = []
        assert walk_segment(d, 0, hi, end(q), walks[q][0], bpm, seg, events)[0] == walks[q][1]
        for e in events:
            if e[0] == "dc":
                pred[e[1]] += e[2]
                if not -32768 <= pred[e[1]] <= 32767:
                    return False, ["dc"], rounds, None
                if b < len(blocks):
                    blocks[b][0] = pred[e[1]]
            elif e[0] == "ac":
                if b < len(blocks):
                    blocks[b][e[1]] = e[2]
            else:
                b += 1
    return False, [], rounds, blocks


def decode(data, sampling, shapes, restart_interval, offsets=None, split_min_bytes=0, geometry=None):
    data = bytes(data)
    geometry = tuple(geometry or GEOMETRY)
    seg = geometry[0]
    split_min = split_min_bytes if split_min_bytes else DEFAULT_MIN_BYTES
    out, status, found, errors = U.decode(data, sampling, shapes, restart_interval, offsets)
    order, bpm = J.mcu_order(sampling, shapes)
    nmcu = len(order) // bpm
    per = nmcu if restart_interval == 0 else restart_interval
    intervals = len(status)
    mk = U.markers(data) if offsets is None else None
    budget = -(-len(data) // seg) + intervals
    counts = {"split_intervals": 0, "serial_intervals": 0, "unsettled_intervals": 0, "rounds": 0}
    why = {k: 0 for k in ("not split", "unsettled", "error", "count", "tail", "dc")}
    used = 0                                             # the segments of all intervals so far, fitting or not
    for i in range(intervals):
        blocks = order[i * per * bpm:(i + 1) * per * bpm]
        if offsets is not None:
            lo, hi = int(offsets[i]), int(offsets[i + 1]) - (0 if i + 1 == intervals else 2)
            ok = 0 <= lo <= hi <= len(data)
        else:
            ok = i <= found
            if ok:
                lo, hi = 0 if i == 0 else mk[i - 1] + 2, mk[i] if i < found else len(data)
        nseg = -(-(hi - lo) // seg) if ok and hi - lo >= max(1, split_min) else 0
        used += nseg
        if nseg == 0 or used > budget:
            counts["serial_intervals"] += 1
            why["not split"] += 1
            continue
        counts["split_intervals"] += 1
        unsettled, failed, rounds, got = _interval(data[lo:hi], tuple(c for c, _, _ in blocks), bpm, geometry)
        counts["unsettled_intervals"] += int(unsettled)
        counts["rounds"] = max(counts["rounds"], rounds)
        if failed:
            counts["serial_intervals"] += 1
            for k in failed:
                why[k] += 1
            continue
        assert status[i] == 0, "an interval that passes the split path's checks is clean"
        for (c, r, col), blk in zip(blocks, got):
            out[c][r, col] = blk
    REASONS.update({k: REASONS.get(k, 0) + v for k, v in why.items()})
    return out, status, found, errors, counts
