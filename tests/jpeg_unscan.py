"""hpdct_decode_scan's rules restated in plain Python (include/hpdct.h is the
specification), for the tests of the entropy decoder (a helper: no test in it).
Where jpeg_scan.decode asserts, this one reports: it reads any bytes and any
offsets table and returns what the library must return, bit for bit.

decode(data, sampling, shapes, restart_interval, offsets=None)
    -> (components, status, markers_found, marker_errors)

components as jpeg_scan's: int16 arrays shaped shapes[c] + (64,), zig-zag order;
status: uint64 per interval, code + 256 * failing block.  The reader takes one
bit at a time, so an error is raised exactly when the bit that needs the
offending byte is asked for.
"""
import numpy as np

import jpeg_scan as J

OK, RANGE, MARKER, END, CODE, INDEX, DC, TAIL, MISSING = range(9)
NAMES = ["OK", "RANGE", "MARKER", "END", "CODE", "INDEX", "DC", "TAIL", "MISSING"]


class _Stop(Exception):
    def __init__(self, code):
        self.code = code


class _Reader:
    """The bits of data[lo:hi], MSB first, unstuffed as they are read."""

    def __init__(self, data, lo, hi):
        self.data, self.pos, self.hi, self.acc, self.n = data, lo, hi, 0, 0

    def bit(self):
        if self.n == 0:
            if self.pos >= self.hi:
                raise _Stop(END)
            b = self.data[self.pos]
            if b == 0xff:
                if self.pos + 1 >= self.hi:
                    raise _Stop(END)
                if self.data[self.pos + 1] != 0x00:
                    raise _Stop(MARKER)
                self.pos += 2
            else:
                self.pos += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, lookup):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in lookup:
                return lookup[(length, code)]
        raise _Stop(CODE)


def _tables():
    inv = lambda t: {(ln, code): sym for sym, (code, ln) in J.codes_of(t).items()}  # noqa: E731
    return [inv(J.DC_LUMA), inv(J.DC_CHROMA)], [inv(J.AC_LUMA), inv(J.AC_CHROMA)]


_DC, _AC = _tables()


_CACHE = {}


def _interval(chunk, comps):
    """One interval: its bytes and the component of each of its blocks -> (the blocks decoded before a failure,
    the status).  Remembered: the corpus decodes the same interval many times."""
    key = (chunk, comps)
    if key not in _CACHE:
        _CACHE[key] = _walk(chunk, comps)
    return _CACHE[key]


def _walk(chunk, comps):
    rd, pred, j, done = _Reader(chunk, 0, len(chunk)), [0, 0, 0], 0, []
    try:
        for j, c in enumerate(comps):
            t = 1 if c else 0
            blk = np.zeros(64, np.int16)
            n = rd.symbol(_DC[t])
            value = pred[c] + J._extend(rd.bits(n), n)
            if not -32768 <= value <= 32767:
                raise _Stop(DC)
            pred[c] = blk[0] = value
            k = 1
            while k < 64:
                s = rd.symbol(_AC[t])
                run, n = s >> 4, s & 15
                if n == 0:
                    if run != 15:
                        break               # EOB
                    k += 16
                    if k > 64:
                        raise _Stop(INDEX)
                    continue
                k += run
                if k > 63:
                    raise _Stop(INDEX)      # judged before the extra bits are read
                blk[k] = J._extend(rd.bits(n), n)
                k += 1
            done.append(blk)
    except _Stop as e:
        return done, e.code + 256 * j       # block j and the later ones stay 0
    npad = rd.n
    if rd.bits(npad) != (1 << npad) - 1 or rd.pos != len(chunk):
        return done, TAIL
    return done, OK


def markers(data):
    """The positions of the restart markers, in byte order."""
    a = np.frombuffer(bytes(data), np.uint8)
    return np.flatnonzero((a[:-1] == 0xff) & (a[1:] >= 0xd0) & (a[1:] <= 0xd7)).tolist()


def decode(data, sampling, shapes, restart_interval, offsets=None):
    data = bytes(data)
    order, bpm = J.mcu_order(sampling, shapes)
    nmcu = len(order) // bpm
    per = nmcu if restart_interval == 0 else restart_interval
    intervals = -(-nmcu // per)
    out = [np.zeros(tuple(s) + (64,), np.int16) for s in shapes]
    status = np.zeros(intervals, np.uint64)
    found = errors = 0
    if offsets is None:
        mk = markers(data)
        found = len(mk)
        errors = sum(1 for j, p in enumerate(mk[:intervals - 1]) if (data[p + 1] & 7) != j % 8)
    for i in range(intervals):
        blocks = order[i * per * bpm:(i + 1) * per * bpm]
        if offsets is not None:
            lo, hi = int(offsets[i]), int(offsets[i + 1]) - (0 if i + 1 == intervals else 2)
            pre = OK if 0 <= lo <= hi <= len(data) else RANGE
        elif i > found:
            pre = MISSING
        else:
            lo, hi, pre = 0 if i == 0 else mk[i - 1] + 2, mk[i] if i < found else len(data), OK
        if pre != OK:
            status[i] = pre                     # the blocks stay 0
            continue
        got, status[i] = _interval(data[lo:hi], tuple(c for c, _, _ in blocks))
        for (c, r, col), blk in zip(blocks, got):
            out[c][r, col] = blk
    return out, status, found, errors
