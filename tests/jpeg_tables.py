"""The entropy coder, the serial entropy decoder, the statistics pass, the
optimal-table builder and hpdct_huffman_prepare's judgement restated in plain
Python, parameterised by the four Huffman tables (include/hpdct.h is the
specification; a helper: no test in it).

A table is a (bits, vals) pair as jpeg_scan.TABLES holds them; `tables` is a list
of four in hpdct_huffman_table's order (DC luma, AC luma, DC chroma, AC chroma),
None standing for an empty table.
"""
import numpy as np

import jpeg_scan as J
import jpeg_unscan as U

MAX_DC_CAT, MAX_AC_CAT = 11, 10
EMPTY = ([0] * 16, [])


def norm(tables):
    return [EMPTY if t is None else ([int(b) for b in t[0]], [int(v) for v in t[1]]) for t in tables]


# ---------------------------------------------------------------------------
# hpdct_huffman_prepare's judgement
# ---------------------------------------------------------------------------
def defect(table, kind, nvals=None):
    """The reason hpdct_huffman_prepare names for refusing `table` as table `kind`, or None."""
    bits, vals = table
    nvals = len(vals) if nvals is None else nvals
    if nvals > 256:
        return "nvals is above 256"
    if nvals != sum(bits):
        return "nvals is not the sum of bits"
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length):
            return "the code is over-subscribed"
        code <<= 1
    seen = set()
    for v in vals:
        if v in seen:
            return "a symbol appears twice"
        seen.add(v)
        if kind % 2 == 0 and v > 15:
            return "a DC symbol is above 15"
    return None


def kraft(bits):
    """The Kraft sum of a table's lengths, in units of 2^-16."""
    return sum(int(b) << (16 - length) for length, b in enumerate(bits, 1))


# ---------------------------------------------------------------------------
# the symbols of a scan: what the coder emits, what the statistics pass counts
# ---------------------------------------------------------------------------
def _symbols(components, sampling, restart_interval):
    """Per interval, the list of (kind, symbol, extra value, extra bits, clamped) the coder emits."""
    comps = [np.asarray(c).astype(np.int64) for c in components]
    order, bpm = J.mcu_order(sampling, J._shapes(components, sampling))
    nmcu = len(order) // bpm
    per = nmcu if restart_interval == 0 else restart_interval
    out = []
    for i in range(-(-nmcu // per)):
        syms, pred = [], [0, 0, 0]
        for c, r, col in order[i * per * bpm:(i + 1) * per * bpm]:
            blk = comps[c][r, col]
            kind = 2 if c else 0
            d = int(blk[0]) - pred[c]
            pred[c] = int(blk[0])
            n = J._category(d)
            clamped = n > MAX_DC_CAT
            n = min(n, MAX_DC_CAT)
            syms.append((kind, n, (d if d >= 0 else d - 1) & ((1 << n) - 1), n, clamped))
            run = 0
            for v in blk[1:]:
                v = int(v)
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    syms.append((kind + 1, 0xf0, 0, 0, False))
                    run -= 16
                n = J._category(v)
                clamped = n > MAX_AC_CAT
                n = min(n, MAX_AC_CAT)
                syms.append((kind + 1, (run << 4) | n, (v if v >= 0 else v - 1) & ((1 << n) - 1), n, clamped))
                run = 0
            if run:
                syms.append((kind + 1, 0x00, 0, 0, False))
        out.append(syms)
    return out


def histogram(components, sampling, restart_interval):
    """counts[kind][symbol] of hpdct_scan_histogram: (4, 256) int64."""
    counts = np.zeros((4, 256), np.int64)
    for syms in _symbols(components, sampling, restart_interval):
        for kind, s, _, _, _ in syms:
            counts[kind, s] += 1
    return counts


def encode(components, sampling, restart_interval, tables):
    """(scan bytes, interval offsets, out_of_range) of hpdct_encode_scan_tables.  out_of_range counts the
    coefficients beyond the categories and the symbols `tables` has no code for; with such a symbol the bytes
    are unspecified and None is returned for them."""
    codes = [J.codes_of(t) for t in norm(tables)]
    data, offsets, oor, missing = bytearray(), [], 0, False
    intervals = _symbols(components, sampling, restart_interval)
    for i, syms in enumerate(intervals):
        offsets.append(len(data))
        w = J._Bits()
        for kind, s, extra, n, clamped in syms:
            oor += clamped
            if s not in codes[kind]:
                oor += 1
                missing = True
                continue
            w.put(*codes[kind][s])
            if n:
                w.put(extra, n)
        data += w.finish()
        if i + 1 < len(intervals):
            data += bytes([0xff, 0xd0 + (i & 7)])
    offsets.append(len(data))
    return (None if missing else bytes(data)), offsets, oor


# ---------------------------------------------------------------------------
# the serial decoder under any tables (jpeg_unscan's walk with its lookups replaced)
# ---------------------------------------------------------------------------
def _lookups(tables):
    return [{(ln, code): sym for sym, (code, ln) in J.codes_of(t).items()} for t in norm(tables)]


def _walk(chunk, comps, look):
    rd, pred, j, done = U._Reader(chunk, 0, len(chunk)), [0, 0, 0], 0, []
    try:
        for j, c in enumerate(comps):
            kind = 2 if c else 0
            blk = np.zeros(64, np.int16)
            n = rd.symbol(look[kind])            # up to 15: hpdct_huffman_prepare refuses more
            value = pred[c] + J._extend(rd.bits(n), n)
            if not -32768 <= value <= 32767:
                raise U._Stop(U.DC)
            pred[c] = blk[0] = value
            k = 1
            while k < 64:
                s = rd.symbol(look[kind + 1])
                run, n = s >> 4, s & 15
                if n == 0:
                    if run != 15:
                        break
                    k += 16
                    if k > 64:
                        raise U._Stop(U.INDEX)
                    continue
                k += run
                if k > 63:
                    raise U._Stop(U.INDEX)
                blk[k] = J._extend(rd.bits(n), n)
                k += 1
            done.append(blk)
    except U._Stop as e:
        return done, e.code + 256 * j
    npad = rd.n
    if rd.bits(npad) != (1 << npad) - 1 or rd.pos != len(chunk):
        return done, U.TAIL
    return done, U.OK


def decode(data, sampling, shapes, restart_interval, tables, offsets=None):
    """jpeg_unscan.decode under `tables`: (components, status, markers_found, marker_errors)."""
    data = bytes(data)
    look = _lookups(tables)
    order, bpm = J.mcu_order(sampling, shapes)
    nmcu = len(order) // bpm
    per = nmcu if restart_interval == 0 else restart_interval
    intervals = -(-nmcu // per)
    out = [np.zeros(tuple(s) + (64,), np.int16) for s in shapes]
    status = np.zeros(intervals, np.uint64)
    found = errors = 0
    if offsets is None:
        mk = U.markers(data)
        found = len(mk)
        errors = sum(1 for j, p in enumerate(mk[:intervals - 1]) if (data[p + 1] & 7) != j % 8)
    for i in range(intervals):
        blocks = order[i * per * bpm:(i + 1) * per * bpm]
        if offsets is not None:
            lo, hi = int(offsets[i]), int(offsets[i + 1]) - (0 if i + 1 == intervals else 2)
            pre = U.OK if 0 <= lo <= hi <= len(data) else U.RANGE
        elif i > found:
            pre = U.MISSING
        else:
            lo, hi, pre = 0 if i == 0 else mk[i - 1] + 2, mk[i] if i < found else len(data), U.OK
        if pre != U.OK:
            status[i] = pre
            continue
        got, status[i] = _walk(data[lo:hi], tuple(c for c, _, _ in blocks), look)
        for (c, r, col), blk in zip(blocks, got):
            out[c][r, col] = blk
    return out, status, found, errors


# ---------------------------------------------------------------------------
# hpdct_huffman_optimal: T.81 K.2, figures K.1 - K.4
# ---------------------------------------------------------------------------
def optimal(counts, adjusted=None):
    """(bits, vals) for 256 counts.  adjusted: a list that gets True appended if figure K.3 moved a code."""
    freq = [int(c) for c in counts] + [1]
    assert len(freq) == 257
    size, other = [0] * 257, [-1] * 257
    while True:
        live = [i for i in range(257) if freq[i]]
        if len(live) < 2:
            break
        v1 = min(live, key=lambda i: (freq[i], -i))
        v2 = min((i for i in live if i != v1), key=lambda i: (freq[i], -i))
        freq[v1] += freq[v2]
        freq[v2] = 0
        # every symbol of both subtrees is one bit longer; v1's chain then runs on into v2's
        size[v1] += 1
        while other[v1] >= 0:
            v1 = other[v1]
            size[v1] += 1
        other[v1] = v2
        size[v2] += 1
        while other[v2] >= 0:
            v2 = other[v2]
            size[v2] += 1
    if not any(size[:256]):
        return [0] * 16, []
    nbits = [0] * max(max(size) + 3, 18)    # any depth up to 257
    for s in size:
        if s:
            nbits[s] += 1
    moved = False
    for i in range(len(nbits) - 1, 16, -1):
        while nbits[i] > 0:
            j = i - 2
            while nbits[j] == 0:
                j -= 1
            nbits[i] -= 2
            nbits[i - 1] += 1
            nbits[j + 1] += 2
            nbits[j] -= 1
            moved = True
    i = 16
    while nbits[i] == 0:
        i -= 1
    nbits[i] -= 1
    if adjusted is not None:
        adjusted.append(moved)
    vals = [s for _, s in sorted((size[s], s) for s in range(256) if size[s])]
    return nbits[1:17], vals


def cost(counts, table):
    """Sum of count * code length; None if a counted symbol has no code."""
    codes = J.codes_of(norm([table])[0])
    total = 0
    for s, c in enumerate(counts):
        if c:
            if s not in codes:
                return None
            total += int(c) * codes[s][1]
    return total


# ---------------------------------------------------------------------------
# the file: the DHT tables a scan's components select (a minimal reader for the tests' fixtures)
# ---------------------------------------------------------------------------
def file_tables(data):
    """(tables, dht_spans) of a baseline file: the four tables as jpeg_parse_tables returns them for a file whose
    components select destinations 0 (Y) and 1 (Cb, Cr) or 0 alone (grey), and the (offset, length) of each DHT
    segment's payload."""
    data = bytes(data)
    p, ht, spans, ncomp = 2, {}, [], 0
    while True:
        assert data[p] == 0xff
        m = data[p + 1]
        ln = (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + ln]
        if m == 0xc4:
            spans.append((p + 4, ln - 2))
            q = 0
            while q < len(seg):
                tc, th = seg[q] >> 4, seg[q] & 15
                bits = list(seg[q + 1:q + 17])
                n = sum(bits)
                ht[(tc, th)] = (bits, list(seg[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xc0:
            ncomp = seg[5]
        elif m == 0xda:
            sel = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ncomp)]
            tabs = [ht[(0, sel[0][0])], ht[(1, sel[0][1])]]
            tabs += [ht[(0, sel[1][0])], ht[(1, sel[1][1])]] if ncomp == 3 else [EMPTY, EMPTY]
            return tabs, spans
        p += 2 + ln


# ---------------------------------------------------------------------------
# the built tables: where Pillow's (longest code 9 bits) do not reach
# ---------------------------------------------------------------------------
# 16 DC symbols, one code of each length 1..16; category 11 has the 16-bit code
BUILT_DC = ([1] * 16, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 11])
# 256 AC symbols: one code at each length 1..7, 249 codes of length 16 (0x0a, run 0 / size 10, among them)
_SHORT = [0x00, 0x01, 0x11, 0x02, 0xf0, 0x21, 0x03]
BUILT_AC = ([1] * 7 + [0] * 8 + [249], _SHORT + [s for s in range(256) if s not in _SHORT])
BUILT = [BUILT_DC, BUILT_AC, BUILT_DC, BUILT_AC]
