"""JPEG-style int16 coefficient blocks, the CPU side (no GPU, no kernel runs):

- hpdct_forward_blocks / hpdct_inverse_blocks validate their arguments and
  return the documented status before any device work (the pointers here are
  never dereferenced);
- the int16 range rule: a table that can give |q| > 32767 is refused with
  HPDCT_ERROR_RANGE and a last-error text that says int16; the int8 wire
  format's own rule (it refuses a DC entry of 8) is unchanged;
- hpdct_zigzag_order is the JPEG scan, and hpdct_quality uses the same table;
- the policy rows of the two launchers, and the validation paths once more in
  a stand-alone program under ASan + UBSan;
- the Python wrappers check their buffers before the library is reached.
"""
import ctypes
import os

import numpy as np
import pytest

import host_programs
from test_host_validation import FakeDev


def _diagonal_walk():
    """The zig-zag scan of an 8x8 block, generated: anti-diagonals v + u = s in
    turn, walked upwards (u rising) for even s and downwards for odd s."""
    order = []
    for s in range(15):
        cells = [(v, s - v) for v in range(8) if 0 <= s - v < 8]  # v rising: walking down
        if s % 2 == 0:
            cells.reverse()
        order += [8 * v + u for v, u in cells]
    return order


A, B = 1 << 20, 1 << 30  # far apart, 16-byte aligned, never dereferenced


def _p(x):
    return ctypes.c_void_p(x)


def test_forward_blocks_arguments_rejected(hp):
    L = hp.load_library()
    fb = L.hpdct_forward_blocks
    assert fb(None, _p(B), 8, 8, 0, None) == 1
    assert fb(_p(A), None, 8, 8, 0, None) == 1
    for h, w in ((12, 8), (8, 20)):
        assert fb(_p(A), _p(B), h, w, 0, None) == 1
        assert b"multiples of 8" in L.hpdct_last_error_string()
    assert fb(_p(A), _p(B + 8), 8, 8, 0, None) == 1        # blocks: 16-byte alignment
    assert b"aligned" in L.hpdct_last_error_string()
    assert fb(_p(A + 4), _p(B), 8, 8, 0, None) == 1        # uint8 frame: 8-byte alignment
    assert fb(_p(A), _p(A + 32), 8, 8, 0, None) == 1       # blocks start inside the 64-byte frame
    assert b"overlap" in L.hpdct_last_error_string()
    assert fb(_p(A + 64), _p(A), 8, 8, 0, None) == 1       # frame inside the 128 bytes of blocks
    assert fb(_p(A), _p(B), 8, 8, 0x80, None) == 2         # unknown flag
    assert fb(_p(A), _p(B), 8, 8, hp.BLOCKS_NATURAL | 0x2, None) == 2


def test_inverse_blocks_arguments_rejected(hp):
    L = hp.load_library()
    ib = L.hpdct_inverse_blocks
    assert ib(None, _p(B), hp.F32, 8, 8, 0, None) == 1
    assert ib(_p(A), None, hp.U8, 8, 8, 0, None) == 1
    for h, w in ((12, 8), (8, 20)):
        assert ib(_p(A), _p(B), hp.F32, h, w, 0, None) == 1
        assert b"multiples of 8" in L.hpdct_last_error_string()
    assert ib(_p(A + 8), _p(B), hp.F32, 8, 8, 0, None) == 1   # blocks: 16-byte alignment
    assert ib(_p(A), _p(B + 8), hp.F32, 8, 8, 0, None) == 1   # fp32 pixels: 16-byte alignment
    assert ib(_p(A), _p(B + 4), hp.U8, 8, 8, 0, None) == 1    # uint8 pixels: 8-byte alignment
    assert ib(_p(A), _p(A + 64), hp.U8, 8, 8, 0, None) == 1   # pixels inside the blocks
    assert b"overlap" in L.hpdct_last_error_string()
    assert ib(_p(A + 128), _p(A), hp.F32, 8, 8, 0, None) == 1  # blocks inside the 256 bytes of fp32 pixels
    assert ib(_p(A), _p(B), hp.F32, 8, 8, 0x80, None) == 2
    assert ib(_p(A), _p(B), hp.I8, 8, 8, 0, None) == 2        # int8 is not a pixel type
    assert ib(_p(A), _p(B), 7, 8, 8, 0, None) == 2


def test_int16_range_rule(hp):
    """1/64 everywhere: the DC quotient reaches 1024 * 64 > 32767 -> status 3,
    and the text names int16.  hpdct_status_string keeps its int8 wording."""
    L = hp.load_library()
    hp.set_quant_table(np.full(64, 1.0 / 64.0, np.float32))
    try:
        assert L.hpdct_forward_blocks(_p(A), _p(B), 8, 8, 0, None) == 3
        assert b"int16" in L.hpdct_last_error_string()
        # arguments are still judged first
        assert L.hpdct_forward_blocks(_p(A), _p(B), 8, 8, 0x80, None) == 2
        assert L.hpdct_forward_blocks(None, _p(B), 8, 8, 0, None) == 1
    finally:
        hp.set_quant_table(None)
    assert L.hpdct_status_string(3).startswith(b"quantised")
    # the int8 wire format's own rule is unchanged: libjpeg's quality-75 luminance table (DC entry 8) is refused
    q75 = np.floor((hp.default_quant_table() * 50 + 50) / 100).astype(np.float32)
    assert q75[0, 0] == 8
    hp.set_quant_table(q75)
    try:
        assert L.hpdct_forward(_p(A), hp.U8, _p(B), hp.I8, 8, 8, None, 0, None) == 3
        assert b"127" in L.hpdct_last_error_string()
    finally:
        hp.set_quant_table(None)


def test_zigzag_order(hp):
    z = hp.zigzag_order()
    assert z.dtype == np.uint8 and z.shape == (64,)
    assert sorted(z.tolist()) == list(range(64))
    assert z.tolist() == _diagonal_walk()
    import hpdct_quality
    assert list(hpdct_quality.ZIGZAG) == z.tolist()
    # NULL is a no-op, as the other table getters
    hp.load_library().hpdct_zigzag_order(None)


def test_blocks_policy_table(tmp_path):
    """policy::forward_blocks / inverse_blocks pinned on the CPU (tests/tools/policy_blocks_check.cpp):
    the staged forward, the tile mapping whatever hpdct_set_mapping says, the straddle variant by width."""
    host_programs.policy_check("policy_blocks_check", tmp_path)


_KOBJ = os.path.join(host_programs.PKG, "build", "hpdct_blocks_fwd.o")


@pytest.mark.skipif(not os.path.exists(_KOBJ), reason="library objects not built (__graft_entry__.build())")
def test_block_validation_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/tools/asan_blocks_check.cpp) drives the new validation paths with
    the C ABI's host sources (tests/tools/asan.mk's HOST) compiled by g++ under ASan + UBSan and the library's kernel objects linked as they are
    (the Makefile's KOBJ line, as tests/tools/asan.mk reads it).  CPU only: nothing is launched."""
    host_programs.sanitised_check("asan_blocks_check", tmp_path, "hpdct_blocks_fwd.o")


def test_forward_blocks_wrapper_checks(hp):
    import torch as t
    img = FakeDev((64, 64), t.uint8)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.forward_blocks(FakeDev((64, 64), t.uint8, cuda=False))
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.forward_blocks(t.zeros((8, 8), dtype=t.uint8))        # a real CPU tensor
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_blocks(FakeDev((64, 64), t.float32))          # the frame must be uint8
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_blocks(img, FakeDev((8, 8, 64), t.float32))   # the blocks must be int16
    with pytest.raises(hp.HpdctError, match="holds"):
        hp.forward_blocks(img, FakeDev((8, 7, 64), t.int16))     # too small
    with pytest.raises(hp.HpdctError, match="contiguous"):
        hp.forward_blocks(img, FakeDev((8, 8, 64), t.int16, contiguous=False))
    with pytest.raises(hp.HpdctError, match="is on"):
        hp.forward_blocks(img, FakeDev((8, 8, 64), t.int16, device="cuda:1"))
    with pytest.raises(hp.HpdctError, match="multiples of 8"):
        hp.forward_blocks(FakeDev((12, 64), t.uint8), FakeDev((8, 8, 64), t.int16))
    with pytest.raises(ValueError):
        hp.forward_blocks(img, FakeDev((8, 8, 64), t.int16), order="diagonal")
    with pytest.raises(hp.HpdctError, match="holds"):
        hp.bind_blocks("fwd", img, FakeDev((8, 7, 64), t.int16))


def test_inverse_blocks_wrapper_checks(hp):
    import torch as t
    blk = FakeDev((8, 8, 64), t.int16)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.inverse_blocks(FakeDev((8, 8, 64), t.int16, cuda=False))
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.inverse_blocks(t.zeros((1, 1, 64), dtype=t.int16))
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_blocks(FakeDev((8, 8, 64), t.int8))           # the blocks must be int16
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_blocks(blk, FakeDev((64, 64), t.int8))        # pixels are fp32 or uint8
    with pytest.raises(hp.HpdctError, match="holds"):
        hp.inverse_blocks(blk, FakeDev((64, 56), t.float32))     # too small
    with pytest.raises(hp.HpdctError, match="height and width"):
        hp.inverse_blocks(FakeDev((4096,), t.int16), FakeDev((64, 64), t.uint8))  # flat blocks: no shape
    with pytest.raises(hp.HpdctError, match="hold"):
        hp.inverse_blocks(FakeDev((4096,), t.int16), FakeDev((64, 128), t.uint8), height=64, width=128)
    with pytest.raises(hp.HpdctError, match="holds"):
        hp.bind_blocks("inv", blk, FakeDev((64, 56), t.uint8))
    with pytest.raises(ValueError):
        hp.bind_blocks("both", blk, FakeDev((64, 64), t.uint8))
