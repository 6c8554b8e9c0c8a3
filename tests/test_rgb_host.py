"""Colour frames, the CPU side (no GPU, no kernel runs):

- hpdct_forward_rgb_blocks / hpdct_inverse_rgb_blocks validate every argument
  and return the documented status before any device work (the pointers here
  are never dereferenced);
- hpdct_default_chroma_quant_table is the JPEG Annex K chrominance table;
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

RGB, Y, CB, CR = 1 << 20, 1 << 30, 1 << 31, 1 << 32  # far apart, 16-byte aligned, never dereferenced
S444, S420 = 0, 1

CHROMA = [17, 18, 24, 47, 99, 99, 99, 99,
          18, 21, 26, 66, 99, 99, 99, 99,
          24, 26, 56, 99, 99, 99, 99, 99,
          47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def _p(x):
    return None if x is None else ctypes.c_void_p(x)


def _t(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _fwd(L, rgb=RGB, y=Y, cb=CB, cr=CR, h=16, w=16, sub=S420, ql=None, qc=None, flags=0):
    return L.hpdct_forward_rgb_blocks(_p(rgb), _p(y), _p(cb), _p(cr), h, w, sub, _t(ql), _t(qc), flags, None)


def _inv(L, rgb=RGB, y=Y, cb=CB, cr=CR, h=16, w=16, sub=S420, ql=None, qc=None, flags=0):
    return L.hpdct_inverse_rgb_blocks(_p(y), _p(cb), _p(cr), _p(rgb), h, w, sub, _t(ql), _t(qc), flags, None)


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["forward", "inverse"])
def test_rgb_arguments_rejected(hp, call):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    for name in ("rgb", "y", "cb", "cr"):
        assert call(L, **{name: None}) == 1
        assert b"null" in err()
    # the size rule of each subsampling
    for h, w in ((8, 8), (16, 24), (24, 16), (0, 16), (-16, 16)):
        assert call(L, h=h, w=w, sub=S420) == 1
        assert b"multiples of 16" in err()
    for h, w in ((12, 8), (8, 20)):
        assert call(L, h=h, w=w, sub=S444) == 1
        assert b"multiples of 8" in err()
    assert call(L, h=1 << 23, w=1 << 23, sub=S444) == 1
    assert b"too large" in err()
    for sub in (2, -1, 77):
        assert call(L, sub=sub) == 1
        assert b"subsampling" in err()
    assert call(L, flags=0x80) == 2
    assert call(L, flags=hp.BLOCKS_NATURAL | 0x2) == 2
    for name, base in (("rgb", RGB), ("y", Y), ("cb", CB), ("cr", CR)):
        assert call(L, **{name: base + 8}) == 1
        assert b"aligned" in err()
    # 16x16: rgb 768 bytes, y 512, cb and cr 128 each (4:2:0) or 512 (4:4:4)
    assert call(L, y=RGB + 752) == 1 and b"overlap" in err()
    assert call(L, rgb=Y + 496) == 1 and b"overlap" in err()
    assert call(L, cb=Y + 496) == 1 and b"overlap" in err()
    assert call(L, cr=CB) == 1 and b"overlap" in err()
    assert call(L, cr=CB + 128, sub=S444) == 1 and b"overlap" in err()
    nan = np.array(CHROMA, np.float32)
    nan[5] = np.nan
    # 4:2:0: cr right behind cb's 128 bytes is no overlap, the call gets as far as the tables
    assert call(L, cr=CB + 128, qc=nan) == 1 and b"chroma" in err()


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["forward", "inverse"])
def test_rgb_tables_rejected(hp, call):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    good = np.array(CHROMA, np.float32)
    for bad_value in (np.nan, np.inf, -np.inf, 0.0):
        bad = good.copy()
        bad[63] = bad_value
        assert call(L, ql=bad, qc=good) == 1 and b"luma" in err() and b"finite and non-zero" in err()
        assert call(L, ql=good, qc=bad) == 1 and b"chroma" in err()
        assert call(L, qc=bad) == 1 and b"chroma" in err()
    # 1/64 everywhere: the DC quotient reaches 1024 * 64 > 32767
    tiny = np.full(64, 1.0 / 64.0, np.float32)
    assert call(L, ql=tiny) == 3 and b"luma" in err() and b"int16" in err()
    assert call(L, qc=tiny) == 3 and b"chroma" in err() and b"int16" in err()
    assert call(L, ql=tiny, flags=0x80) == 2            # arguments are still judged first
    assert call(L, ql=tiny, rgb=None) == 1
    # q_luma NULL is the library-owned table, under the same rule
    hp.set_quant_table(tiny)
    try:
        assert call(L) == 3 and b"luma" in err()
        # a per-call luma table replaces it: this call passes the luma rule and stops at the chroma table
        bad = good.copy()
        bad[0] = np.nan
        assert call(L, ql=good, qc=bad) == 1 and b"chroma" in err()
    finally:
        hp.set_quant_table(None)


def test_default_chroma_table(hp):
    q = hp.default_chroma_quant_table()
    assert q.dtype == np.float32 and q.shape == (8, 8)
    assert q.reshape(-1).tolist() == [float(v) for v in CHROMA]
    assert (q[4:] == 99).all() and np.array_equal(q, q.T)
    hp.load_library().hpdct_default_chroma_quant_table(None)     # NULL is a no-op, as the other table getters
    # the luma default is untouched by it
    assert hp.default_quant_table()[0, 0] == 16


def test_rgb_symbols_are_declared(hp):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hpdct.h")).read()
    for name in ("hpdct_default_chroma_quant_table", "hpdct_forward_rgb_blocks", "hpdct_inverse_rgb_blocks"):
        assert name in hp.C_SYMBOLS and name + "(" in text
        getattr(hp.load_library(), name)
    assert "HPDCT_SUBSAMPLING_444 = 0" in text and "HPDCT_SUBSAMPLING_420 = 1" in text
    assert hp.SUBSAMPLINGS == {"444": 0, "420": 1}


def test_rgb_policy_table(tmp_path):
    """policy::forward_rgb / inverse_rgb pinned on the CPU (tests/tools/policy_rgb_check.cpp): the staged
    forward, the three quotient pairs, the grid of one wave per 64 units."""
    host_programs.policy_check("policy_rgb_check", tmp_path)


_KOBJ = os.path.join(host_programs.PKG, "build", "hpdct_rgb_inv.o")


@pytest.mark.skipif(not os.path.exists(_KOBJ), reason="library objects not built (__graft_entry__.build())")
def test_rgb_validation_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/tools/asan_rgb_check.cpp) drives the new validation paths with
    the C ABI's host sources (tests/tools/asan.mk's HOST) compiled by g++ under ASan + UBSan and the library's kernel objects linked as they are
    (the Makefile's KOBJ line).  CPU only: nothing is launched."""
    host_programs.sanitised_check("asan_rgb_check", tmp_path, "hpdct_rgb_inv.o")


class _Dev(FakeDev):
    """A FakeDev with an address, for the overlap check (still never dereferenced)."""

    def __init__(self, shape, dtype, ptr, **kw):
        super().__init__(shape, dtype, **kw)
        self._ptr = ptr

    def data_ptr(self):
        return self._ptr


def test_forward_rgb_wrapper_checks(hp):
    import torch as t
    rgb = FakeDev((32, 32, 3), t.uint8)
    yb, cb = FakeDev((4, 4, 64), t.int16), FakeDev((2, 2, 64), t.int16)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.forward_rgb_blocks(FakeDev((32, 32, 3), t.uint8, cuda=False))
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.forward_rgb_blocks(t.zeros((16, 16, 3), dtype=t.uint8))          # a real CPU tensor
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_rgb_blocks(FakeDev((32, 32, 3), t.float32))
    with pytest.raises(hp.HpdctError, match=r"\(H, W, 3\)"):
        hp.forward_rgb_blocks(FakeDev((32, 32), t.uint8))
    with pytest.raises(hp.HpdctError, match=r"\(H, W, 3\)"):
        hp.forward_rgb_blocks(FakeDev((32, 32, 4), t.uint8))
    with pytest.raises(hp.HpdctError, match="multiples of 16"):
        hp.forward_rgb_blocks(FakeDev((24, 32, 3), t.uint8), out=(yb, cb, cb))
    with pytest.raises(hp.HpdctError, match="multiples of 8"):
        hp.forward_rgb_blocks(FakeDev((24, 36, 3), t.uint8), subsampling="444", out=(yb, cb, cb))
    with pytest.raises(hp.HpdctError, match="contiguous"):
        hp.forward_rgb_blocks(FakeDev((32, 32, 3), t.uint8, contiguous=False), out=(yb, cb, cb))
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_rgb_blocks(rgb, out=(FakeDev((4, 4, 64), t.float32), cb, cb))
    with pytest.raises(hp.HpdctError, match="y blocks holds"):
        hp.forward_rgb_blocks(rgb, out=(FakeDev((4, 3, 64), t.int16), cb, cb))
    with pytest.raises(hp.HpdctError, match="cr blocks holds"):
        hp.forward_rgb_blocks(rgb, out=(yb, cb, FakeDev((2, 1, 64), t.int16)))
    with pytest.raises(hp.HpdctError, match="cb blocks holds"):
        hp.forward_rgb_blocks(rgb, subsampling="444", out=(yb, cb, cb))     # 4:4:4 chroma is full size
    with pytest.raises(hp.HpdctError, match="contiguous"):
        hp.forward_rgb_blocks(rgb, out=(yb, FakeDev((2, 2, 64), t.int16, contiguous=False), cb))
    with pytest.raises(hp.HpdctError, match="is on"):
        hp.forward_rgb_blocks(rgb, out=(yb, cb, FakeDev((2, 2, 64), t.int16, device="cuda:1")))
    with pytest.raises(ValueError):
        hp.forward_rgb_blocks(rgb, subsampling="422", out=(yb, cb, cb))
    with pytest.raises(ValueError):
        hp.forward_rgb_blocks(rgb, order="diagonal", out=(yb, cb, cb))
    # overlap: 32x32 rgb is 3072 bytes, y 2048, cb and cr 512
    r = _Dev((32, 32, 3), t.uint8, 1 << 20)
    y = _Dev((4, 4, 64), t.int16, 1 << 21)
    with pytest.raises(hp.HpdctError, match="rgb and y buffers overlap"):
        hp.forward_rgb_blocks(r, out=(_Dev((4, 4, 64), t.int16, (1 << 20) + 3056),
                                      _Dev((2, 2, 64), t.int16, 1 << 22), _Dev((2, 2, 64), t.int16, 1 << 23)))
    with pytest.raises(hp.HpdctError, match="cb and cr buffers overlap"):
        hp.forward_rgb_blocks(r, out=(y, _Dev((2, 2, 64), t.int16, 1 << 22), _Dev((2, 2, 64), t.int16, (1 << 22) + 496)))
    with pytest.raises(hp.HpdctError, match="64 floats"):
        hp.forward_rgb_blocks(r, q_chroma=np.ones(63, np.float32),
                              out=(y, _Dev((2, 2, 64), t.int16, 1 << 22), _Dev((2, 2, 64), t.int16, 1 << 23)))
    with pytest.raises(hp.HpdctError, match="y blocks holds"):
        hp.bind_rgb_blocks("fwd", rgb, FakeDev((4, 3, 64), t.int16), cb, cb)
    with pytest.raises(ValueError):
        hp.bind_rgb_blocks("both", rgb, yb, cb, cb)


def test_inverse_rgb_wrapper_checks(hp):
    import torch as t
    yb, cb = FakeDev((4, 4, 64), t.int16), FakeDev((2, 2, 64), t.int16)
    out = FakeDev((32, 32, 3), t.uint8)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.inverse_rgb_blocks(FakeDev((4, 4, 64), t.int16, cuda=False), cb, cb, subsampling="420")
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_rgb_blocks(FakeDev((4, 4, 64), t.int8), cb, cb, subsampling="420")
    with pytest.raises(hp.HpdctError, match="height and width"):
        hp.inverse_rgb_blocks(FakeDev((1024,), t.int16), cb, cb, subsampling="420", out=out)   # flat: no shape
    with pytest.raises(hp.HpdctError, match="multiples of 16"):
        hp.inverse_rgb_blocks(FakeDev((3, 4, 64), t.int16), cb, cb, subsampling="420", out=out)
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_rgb_blocks(yb, cb, cb, subsampling="420", out=FakeDev((32, 32, 3), t.float32))
    with pytest.raises(hp.HpdctError, match="rgb holds"):
        hp.inverse_rgb_blocks(yb, cb, cb, subsampling="420", out=FakeDev((32, 31, 3), t.uint8))
    with pytest.raises(hp.HpdctError, match="cb blocks holds"):
        hp.inverse_rgb_blocks(yb, FakeDev((2, 1, 64), t.int16), cb, subsampling="420", out=out)
    with pytest.raises(hp.HpdctError, match="cr blocks holds"):
        hp.inverse_rgb_blocks(yb, yb, cb, subsampling="444", out=out)
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_rgb_blocks(yb, cb, FakeDev((2, 2, 64), t.float32), subsampling="420", out=out)
    with pytest.raises(hp.HpdctError, match="y blocks holds"):
        hp.inverse_rgb_blocks(FakeDev((512,), t.int16), cb, cb, subsampling="420", out=out, height=32, width=32)
    with pytest.raises(TypeError):
        hp.inverse_rgb_blocks(yb, cb, cb, out=out)                    # the subsampling has no default here
    with pytest.raises(hp.HpdctError, match="cr blocks holds"):
        hp.bind_rgb_blocks("inv", out, yb, cb, FakeDev((2, 1, 64), t.int16))
