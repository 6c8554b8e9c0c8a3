"""Baseline-JPEG entropy coding restated in plain Python, for the tests of
hpdct_encode_scan and hpdct_jpeg_header (a helper: no test in it).

- the four typical Huffman tables of ITU-T T.81 Annex K.3 as literals (data
  from the standard) and the zig-zag order;
- encode(components, sampling, restart_interval) -> (bytes, offsets): the scan
  the library must produce, byte for byte;
- out_of_range(...): the coefficients baseline Huffman cannot code;
- decode(data, sampling, shapes, restart_interval) -> components: an independent
  decoder that walks the tables bit by bit;
- idct(blocks, q): the float64 exact inverse DCT of dequantised blocks.

components: a list of one (grey) or three (Y, Cb, Cr) int arrays shaped
(tile rows, tile columns, 64), each block in ZIG-ZAG order.  sampling: "grey",
"444" or "420".
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63]

# Annex K.3: (BITS, HUFFVAL); BITS[l-1] = number of codes of length l
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
TABLES = [DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA]      # hpdct_huffman_table's kinds 0..3
MAX_DC, MAX_AC = 2047, 1023                            # the largest magnitudes baseline codes


def codes_of(table):
    """{symbol: (code, length)} by Annex C: codes of each length count up, then shift."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def mcu_order(sampling, shapes):
    """The (component, tile row, tile column) of every block of the scan, MCU after MCU in row-major order, and
    the number of blocks per MCU."""
    if sampling == "grey":
        (ty, tx), = shapes
        return [(0, r, c) for r in range(ty) for c in range(tx)], 1
    ty, tx = shapes[1]
    order = []
    for my in range(ty):
        for mx in range(tx):
            if sampling == "420":
                order += [(0, 2 * my + dy, 2 * mx + dx) for dy in (0, 1) for dx in (0, 1)]
            else:
                order.append((0, my, mx))
            order += [(1, my, mx), (2, my, mx)]
    return order, 6 if sampling == "420" else 3


def _shapes(components, sampling):
    shapes = [tuple(int(s) for s in np.asarray(c).shape[:2]) for c in components]
    assert all(np.asarray(c).shape[2] == 64 for c in components)
    if sampling == "grey":
        assert len(shapes) == 1
    else:
        assert len(shapes) == 3 and shapes[1] == shapes[2]
        f = 2 if sampling == "420" else 1
        assert shapes[0] == (f * shapes[1][0], f * shapes[1][1]), shapes
    return shapes


def _category(v):
    return int(abs(int(v))).bit_length()


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | value
        self.n += nbits
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xff)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        """Pads the partial byte with 1 bits; returns the stuffed bytes."""
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out).replace(b"\xff", b"\xff\x00")


def encode(components, sampling, restart_interval):
    """(scan bytes, interval offsets): offsets[i] is the first byte of interval i, offsets[-1] the length."""
    comps = [np.asarray(c).astype(np.int64) for c in components]
    order, bpm = mcu_order(sampling, _shapes(components, sampling))
    nmcu = len(order) // bpm
    per = nmcu if restart_interval == 0 else restart_interval
    dc = [codes_of(DC_LUMA), codes_of(DC_CHROMA)]
    ac = [codes_of(AC_LUMA), codes_of(AC_CHROMA)]
    data, offsets = bytearray(), []
    intervals = -(-nmcu // per)
    for i in range(intervals):
        offsets.append(len(data))
        w, pred = _Bits(), [0, 0, 0]
        for c, r, col in order[i * per * bpm:(i + 1) * per * bpm]:
            blk = comps[c][r, col]
            t = 1 if c else 0
            d = int(blk[0]) - pred[c]
            pred[c] = int(blk[0])
            if abs(d) > MAX_DC:
                raise ValueError("DC difference %d has no baseline code" % d)
            n = _category(d)
            w.put(*dc[t][n])
            if n:
                w.put(d if d > 0 else d + (1 << n) - 1, n)
            run = 0
            for v in blk[1:]:
                v = int(v)
                if v == 0:
                    run += 1
                    continue
                if abs(v) > MAX_AC:
                    raise ValueError("AC value %d has no baseline code" % v)
                while run >= 16:
                    w.put(*ac[t][0xf0])
                    run -= 16
                n = _category(v)
                w.put(*ac[t][(run << 4) | n])
                w.put(v if v > 0 else v + (1 << n) - 1, n)
                run = 0
            if run:
                w.put(*ac[t][0x00])
        data += w.finish()
        if i + 1 < intervals:
            data += bytes([0xff, 0xd0 + (i & 7)])
    offsets.append(len(data))
    return bytes(data), offsets


def out_of_range(components, sampling, restart_interval):
    """How many coefficients baseline cannot code: DC differences (against the previous block of the component,
    0 at an interval's start) beyond +-2047 and AC values beyond +-1023."""
    comps = [np.asarray(c).astype(np.int64) for c in components]
    order, bpm = mcu_order(sampling, _shapes(components, sampling))
    per = len(order) // bpm if restart_interval == 0 else restart_interval
    count, pred = 0, [0, 0, 0]
    for k, (c, r, col) in enumerate(order):
        if k % (per * bpm) == 0:
            pred = [0, 0, 0]
        blk = comps[c][r, col]
        count += int(abs(int(blk[0]) - pred[c]) > MAX_DC) + int((np.abs(blk[1:]) > MAX_AC).sum())
        pred[c] = int(blk[0])
    return count


class _Reader:
    """Bits of one interval's bytes, unstuffed as they are read."""

    def __init__(self, data):
        self.data, self.pos, self.acc, self.n = data, 0, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.data[self.pos]
            self.pos += 1
            if b == 0xff:
                assert self.data[self.pos] == 0x00, "a marker inside an interval"
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
        raise AssertionError("no code of 16 bits or fewer")


def _extend(v, n):
    return v if n == 0 or v >= 1 << (n - 1) else v - (1 << n) + 1


def decode(data, sampling, shapes, restart_interval):
    """The blocks of a scan: a list of int16 arrays shaped shapes[c] + (64,), zig-zag order.  Checks that the
    intervals end with 1-bit padding and RSTm markers in sequence, and that nothing follows the last one."""
    order, bpm = mcu_order(sampling, shapes)
    nmcu = len(order) // bpm
    per = nmcu if restart_interval == 0 else restart_interval
    inv = lambda t: {(ln, code): sym for sym, (code, ln) in codes_of(t).items()}  # noqa: E731
    dc, ac = [inv(DC_LUMA), inv(DC_CHROMA)], [inv(AC_LUMA), inv(AC_CHROMA)]
    out = [np.zeros(tuple(s) + (64,), np.int16) for s in shapes]
    pos, intervals = 0, -(-nmcu // per)
    for i in range(intervals):
        rd, pred = _Reader(data[pos:]), [0, 0, 0]
        for c, r, col in order[i * per * bpm:(i + 1) * per * bpm]:
            t = 1 if c else 0
            n = rd.symbol(dc[t])
            pred[c] += _extend(rd.bits(n), n)
            out[c][r, col, 0] = pred[c]
            k = 1
            while k < 64:
                s = rd.symbol(ac[t])
                run, n = s >> 4, s & 15
                if n == 0:
                    if run != 15:
                        break           # EOB
                    k += 16
                    continue
                k += run
                out[c][r, col, k] = _extend(rd.bits(n), n)
                k += 1
            assert k <= 64
        npad = rd.n
        assert rd.bits(npad) == (1 << npad) - 1, "padding must be 1 bits"
        pos += rd.pos
        if i + 1 < intervals:
            assert data[pos:pos + 2] == bytes([0xff, 0xd0 + (i & 7)]), (i, data[pos:pos + 2])
            pos += 2
    assert pos == len(data), (pos, len(data))
    return out


def dct_matrix():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.sqrt(2.0 / 8.0) * np.cos((2 * n + 1) * k * np.pi / 16.0)
    c[0] = np.sqrt(1.0 / 8.0)
    return c


def fdct(pixels):
    """float64 exact DCT of (..., 8, 8) level-shifted pixel tiles."""
    c = dct_matrix()
    return c @ np.asarray(pixels, np.float64) @ c.T


def idct(blocks, q):
    """(..., 64) zig-zag blocks and the 64-entry row-major table q -> (..., 8, 8) float64 pixels (+128)."""
    b = np.asarray(blocks, np.float64)
    nat = np.zeros_like(b)
    nat[..., ZIGZAG] = b
    nat = nat * np.asarray(q, np.float64).reshape(64)
    c = dct_matrix()
    return c.T @ nat.reshape(b.shape[:-1] + (8, 8)) @ c + 128.0


def plane(tiles):
    """(ty, tx, 8, 8) -> (8 ty, 8 tx)."""
    ty, tx = tiles.shape[:2]
    return tiles.transpose(0, 2, 1, 3).reshape(8 * ty, 8 * tx)
