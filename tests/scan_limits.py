"""Inputs that drive the entropy coder (hpdct_encode_scan) to the limits its
buffers and loops allow, and what the restatement of tests/jpeg_scan.py says of
them.  A plain helper (no test in it): tests/test_scan_limits_host.py proves on
the CPU that the inputs reach what they claim, tests/test_gpu_scan_limits.py
feeds them to the GPU.  Every input comes from a fixed seed.

components: as in jpeg_scan, a list of one or three int16 arrays shaped
(tile rows, tile columns, 64), each block in ZIG-ZAG order.

- saturated(sampling, shape, ac): every AC coefficient +-1023, the DC of each
  component alternating +1023 / -1023 in scan order: the longest codes baseline
  has, so a 64-block step fills the wave's bit buffer (csrc/hpdct_scan.hpp);
- saturated_out_of_range(sampling, shape): every coefficient 32767 or -32768;
- sparse_grey(n) / sparse_420(): one interval per block (or per two MCUs), more
  than the 1024 threads of the offsets kernel;
- GridCap: 1025 x 1025 grey tiles at restart_interval 1, 2049 intervals past the
  2^20 workgroups the coding launches are capped at.
"""
import numpy as np

import decoder_blocks
import jpeg_scan as J

# csrc/hpdct_scan.hpp: the longest block, the words of a wave's bit buffer, the blocks of one step
MAX_BLOCK_BITS = 1660
BIT_WORDS = 3322
STEP = 64
# csrc/hpdct_policy.hpp (kScanMaxWgs; tests/tools/policy_scan_check.cpp pins it) and the offsets kernel's threads
MAX_WGS = 1 << 20
OFFSET_THREADS = 1024

# (sampling, (height, width)): grey two full steps; two and a tail of 8; 4:4:4 one and a tail of 2; 4:2:0 two and
# a tail of 4
SATURATED_SHAPES = [("grey", (8, 1024)), ("grey", (8, 1088)), ("444", (16, 88)), ("420", (32, 176))]
SATURATED_AC = ["neg", "pos", "mixed"]
UNEVEN_INTERVAL = {"grey": 50, "444": 7, "420": 3}       # cuts a 64-block step unevenly

_memo = {}


def component_shapes(sampling, shape):
    """The (tile rows, tile columns) of each component of an (h, w) frame."""
    h, w = shape
    if sampling == "grey":
        return [(h // 8, w // 8)]
    f = 2 if sampling == "420" else 1
    return [(h // 8, w // 8)] + 2 * [(h // 8 // f, w // 8 // f)]


def blocks_of(sampling, shape):
    return sum(ty * tx for ty, tx in component_shapes(sampling, shape))


def intervals_of(sampling, shape, ri):
    ty, tx = component_shapes(sampling, shape)[-1]
    nmcu = ty * tx
    return 1 if ri == 0 else -(-nmcu // ri)


def natural(zz_blocks):
    """Zig-zag blocks -> the same blocks in natural (row-major) order."""
    nat = np.zeros_like(zz_blocks)
    nat[..., J.ZIGZAG] = zz_blocks
    return nat


def _alternate_dc(comps, sampling, first=1023):
    """Sets the DC of each component to +first, -first, ... in that component's scan order."""
    order, _ = J.mcu_order(sampling, [c.shape[:2] for c in comps])
    seen = [0, 0, 0]
    for c, r, col in order:
        comps[c][r, col, 0] = first if seen[c] % 2 == 0 else -first
        seen[c] += 1


def saturated(sampling, shape, ac):
    """Every AC coefficient -1023 ("neg": extra bits all 0), +1023 ("pos": all 1, the most 0xFF bytes) or a seeded
    mix of the two ("mixed"); DC differences after the first +-2046, category 11.  All within baseline's range."""
    k = ("sat", sampling, shape, ac)
    if k not in _memo:
        rng = np.random.default_rng(1660)
        comps = []
        for ty, tx in component_shapes(sampling, shape):
            if ac == "mixed":
                c = np.where(rng.integers(0, 2, (ty, tx, 64)) == 1, 1023, -1023).astype(np.int16)
            else:
                c = np.full((ty, tx, 64), {"neg": -1023, "pos": 1023}[ac], np.int16)
            comps.append(c)
        _alternate_dc(comps, sampling)
        for c in comps:
            c.setflags(write=False)
        _memo[k] = comps
    return _memo[k]


def saturated_out_of_range(sampling, shape):
    """Every coefficient 32767 or -32768, alternating along a block and from block to block (so the DC differences
    are +-65535): nothing in it has a baseline code but the bytes must still be safe."""
    k = ("oor", sampling, shape)
    if k not in _memo:
        comps = []
        for ty, tx in component_shapes(sampling, shape):
            par = (np.arange(ty * tx)[:, None] + np.arange(64)[None, :]) % 2
            c = np.where(par == 0, 32767, -32768).astype(np.int16).reshape(ty, tx, 64)
            c.setflags(write=False)
            comps.append(c)
        _memo[k] = comps
    return _memo[k]


def _sparse(shape_tiles, seed, clip):
    """About one coefficient in ten kept (the same mask for both ranges), values in +-1023 or +-32767."""
    ty, tx = shape_tiles
    keep = np.random.default_rng(seed).random((ty, tx, 64)) < 0.1
    a = 1023 if clip else 32767
    rng = np.random.default_rng(seed + 1000)
    vals = rng.integers(1, a + 1, (ty, tx, 64)) * np.where(rng.integers(0, 2, (ty, tx, 64)) == 1, 1, -1)
    c = np.where(keep, vals, 0).astype(np.int16)
    c.setflags(write=False)
    return c


MANY_GREY = [1023, 1024, 1025, 2049, 2500]     # intervals of the offsets kernel: chunk 1, 1, 2, 3, 3
MANY_420 = (16, 35200)                         # 2200 MCUs, restart_interval 2: 1100 intervals, 13,200 blocks


def sparse_grey(n, clip=True):
    """An 8 x 8n grey frame for restart_interval 1: n intervals of differing lengths."""
    k = ("sparse", n, clip)
    if k not in _memo:
        _memo[k] = [_sparse((1, n), 31 + n, clip)]
    return _memo[k]


def sparse_420():
    if "sparse420" not in _memo:
        _memo["sparse420"] = [_sparse(s, 77 + i, True) for i, s in enumerate(component_shapes("420", MANY_420))]
    return _memo["sparse420"]


def offsets_chunk(intervals):
    """Intervals per thread of the offsets kernel (csrc/hpdct_scan.hpp, scan_offsets_kernel)."""
    return -(-intervals // OFFSET_THREADS)


def expected(key, components, sampling, ri):
    """jpeg_scan.encode, computed once per input and interval."""
    k = ("want", key, sampling, ri)
    if k not in _memo:
        _memo[k] = J.encode(components, sampling, ri)
    return _memo[k]


# ---------------------------------------------------------------------------
# how full the coder's buffers get: the bit lengths of the blocks, by the tables of jpeg_scan
# ---------------------------------------------------------------------------
def block_bits(components, sampling, ri):
    """The bit length of every block in scan order, and the number of blocks per interval."""
    comps = [np.asarray(c).astype(np.int64) for c in components]
    order, bpm = J.mcu_order(sampling, [c.shape[:2] for c in comps])
    per = len(order) if ri == 0 else ri * bpm
    dc = [J.codes_of(J.DC_LUMA), J.codes_of(J.DC_CHROMA)]
    ac = [J.codes_of(J.AC_LUMA), J.codes_of(J.AC_CHROMA)]
    bits, pred = [], [0, 0, 0]
    for k, (c, r, col) in enumerate(order):
        if k % per == 0:
            pred = [0, 0, 0]
        blk, t = comps[c][r, col], 1 if c else 0
        d = int(blk[0]) - pred[c]
        pred[c] = int(blk[0])
        n = abs(d).bit_length()
        total, run = dc[t][n][1] + n, 0
        for v in blk[1:]:
            v = int(v)
            if v == 0:
                run += 1
                continue
            total += (run // 16) * ac[t][0xf0][1]
            n = abs(v).bit_length()
            total += ac[t][((run % 16) << 4) | n][1] + n
            run = 0
        if run:
            total += ac[t][0x00][1]
        bits.append(total)
    return bits, per


def step_fill(bits, per):
    """What the coding kernel holds in its bit buffer at each 64-block step of each interval: the bits carried from
    the step before (fewer than 8) and those of the step's blocks.  Returns the list over all steps."""
    out = []
    for i0 in range(0, len(bits), per):
        carry = 0
        iv = bits[i0:i0 + per]
        for s in range(0, len(iv), STEP):
            n = carry + sum(iv[s:s + STEP])
            out.append(n)
            carry = n % 8
    return out


def buffer_words(nbits):
    """The words of the bit buffer a step of nbits bits clears and may touch (scan_code_kernel)."""
    return (nbits + 31) // 32 + 1


# ---------------------------------------------------------------------------
# more intervals than the coding launches have workgroups
# ---------------------------------------------------------------------------
class GridCap:
    """A grey frame of TILES x TILES tiles at restart_interval 1: block i is clipped-catalogue block i % 381.
    Every block is an interval of its own with predictor 0, so the scan is the 381 blocks' own scans, each coded
    once, joined with the RSTm markers.  per: the 381 scans (bytes)."""
    TILES = 1025
    N = TILES * TILES                       # 1,050,625 intervals, 2049 past MAX_WGS
    PERIOD = decoder_blocks.FIRST * 8       # after 381 * 8 intervals block and marker both repeat

    def __init__(self, T):
        cat, _ = decoder_blocks.catalogue(T)
        self.blocks = np.ascontiguousarray(np.clip(cat[:decoder_blocks.FIRST], -1023, 1023)[:, J.ZIGZAG])
        self.per = [J.encode([b.reshape(1, 1, 64)], "grey", 1)[0] for b in self.blocks]

    def lengths(self, n):
        """The byte length of each of the first n intervals, marker included (the frame's last has none)."""
        one = np.array([len(p) + 2 for p in self.per], np.int64)
        lens = np.resize(one, n)
        if n == self.N:
            lens[-1] -= 2
        return lens

    def offsets(self, n):
        return np.concatenate(([0], np.cumsum(self.lengths(n))))

    def scan(self, n):
        """The first n intervals as a uint8 array, each followed by its marker (the frame's last by none)."""
        m = len(self.per)
        period = b"".join(self.per[i % m] + bytes([0xff, 0xd0 + (i & 7)]) for i in range(min(n, self.PERIOD)))
        data = np.frombuffer(period, np.uint8)
        if n > self.PERIOD:
            data = np.resize(data, int(self.lengths(n).sum()) + (2 if n == self.N else 0))
        return data[:-2] if n == self.N else data
