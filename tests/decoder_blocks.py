"""A catalogue of int16 coefficient blocks as a JPEG decoder meets them, for the
inverse kernels: the inputs the library's own forward never makes from noise
images.  A plain helper (no test in it); tests/test_decoder_blocks.py checks
the catalogue itself on the CPU, tests/test_gpu_decoder_input.py feeds it to
the GPU.

catalogue() returns (blocks, classes): at most 1024 blocks of 64 int16 in
natural (row-major) order and the class name of each, shuffled once with a
fixed seed chosen so that the first FIRST entries hold every class.

Classes:
  zero          the all-zero block
  dc            DC only: 1, -1, -1024, 1016, -64, 63, -65, 64, 32767, -32768
                (under the default table -64, 63 and 64 land on 7.6e-6, 254 and
                256, the edges of the clamp; -65 lands on -2)
  basis         one non-zero coefficient at each of the 64 positions, with
                1, -1, 37, -37, 32767, -32768: the classic IDCT conformance set
  dense-A       every coefficient uniform in [-A, A)
  sparse-A      the same with about one coefficient in ten kept
  worst-sign    32767 * sign(T[:, i] (x) T[:, j]) for the pixel (i, j) with the
                largest column abs-sums of T, and its negation
"""
import numpy as np

SIZE = 1024
FIRST = 381            # the tiles of a 24 x 1016 frame
SEED = 5               # of the one shuffle; test_decoder_blocks asserts what it was chosen for
DC_VALUES = [1, -1, -1024, 1016, -64, 63, -65, 64, 32767, -32768]
BASIS_VALUES = [1, -1, 37, -37, 32767, -32768]
AMPLITUDES = [2, 8, 32, 128, 1024, 32768]
# Blocks per dense and sparse class: the 627 left beside the 397 fixed ones.
# The small amplitudes keep pixels inside (0, 255), the large ones clamp nearly
# all of them; the split keeps each of the three shares of
# test_decoder_blocks above 20 %.
DENSE_COUNT = {2: 40, 8: 40, 32: 60, 128: 70, 1024: 70, 32768: 70}
SPARSE_COUNT = {2: 30, 8: 30, 32: 40, 128: 57, 1024: 60, 32768: 60}

_memo = {}


def worst_sign_blocks(T):
    """The two blocks that drive one pixel's two chains furthest: every term of both passes with one sign."""
    T = np.asarray(T, np.float64).reshape(8, 8)
    k = int(np.argmax(np.abs(T).sum(axis=0)))
    s = np.sign(np.outer(T[:, k], T[:, k])).astype(np.int64).reshape(64)
    return np.stack([32767 * s, -32767 * s]).astype(np.int16)


def catalogue(T):
    """(blocks (n, 64) int16, classes: list of n names) for the transform matrix T; read-only, built once."""
    if "cat" in _memo:
        return _memo["cat"]
    rng = np.random.default_rng(2024)
    blocks, classes = [np.zeros(64, np.int16)], ["zero"]
    for v in DC_VALUES:
        b = np.zeros(64, np.int16)
        b[0] = v
        blocks.append(b)
        classes.append("dc")
    for pos in range(64):
        for v in BASIS_VALUES:
            b = np.zeros(64, np.int16)
            b[pos] = v
            blocks.append(b)
            classes.append("basis")
    for a in AMPLITUDES:
        for _ in range(DENSE_COUNT[a]):
            blocks.append(rng.integers(-a, a, 64).astype(np.int16))
            classes.append("dense-%d" % a)
        for _ in range(SPARSE_COUNT[a]):
            b = rng.integers(-a, a, 64)
            blocks.append(np.where(rng.random(64) < 0.1, b, 0).astype(np.int16))
            classes.append("sparse-%d" % a)
    for b in worst_sign_blocks(T):
        blocks.append(b)
        classes.append("worst-sign")
    assert len(blocks) == SIZE, len(blocks)
    order = np.random.default_rng(SEED).permutation(len(blocks))
    cat = np.stack(blocks)[order]
    cat.setflags(write=False)
    _memo["cat"] = (cat, [classes[i] for i in order])
    return _memo["cat"]


def of_classes(T, names):
    """The catalogue's blocks of the named classes, in catalogue order."""
    cat, classes = catalogue(T)
    return cat[[i for i, c in enumerate(classes) if c in names]]


def take(T, n, offset=0):
    """n blocks, the catalogue taken cyclically from `offset`."""
    cat, _ = catalogue(T)
    return cat[(offset + np.arange(n)) % len(cat)]


def plane_of(blocks, h, w):
    """Natural-order blocks in row-major tile order -> the (h, w) fp32 plane holding (float)block."""
    b = np.asarray(blocks).reshape(h // 8, w // 8, 8, 8)
    return np.ascontiguousarray(b.transpose(0, 2, 1, 3).reshape(h, w).astype(np.float32))


def in_order(blocks, zz, order):
    """Natural-order blocks -> the array a call is given: element n is the coefficient at position zz[n]."""
    b = np.asarray(blocks).reshape(-1, 64)
    return np.ascontiguousarray(b[:, zz] if order == "zigzag" else b)
