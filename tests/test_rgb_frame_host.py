"""Colour frames of any size and row pitch, the CPU side (no GPU, no kernel runs):

- hpdct_rgb_frame_geometry, hpdct_forward_rgb_frame and hpdct_inverse_rgb_frame
  validate every argument and return the documented status before any device
  work (the pointers here are never dereferenced);
- the policy rows of the two launchers for whole-unit and for ragged or
  unaligned frames, and the validation paths once more in a stand-alone
  program under ASan + UBSan;
- the Python wrappers check strides and sizes before the library is reached.
"""
import ctypes
import os

import numpy as np
import pytest

import host_programs
from test_host_validation import FakeDev
from test_rgb_host import CHROMA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB, Y, CB, CR = 1 << 20, 1 << 30, 1 << 31, 1 << 32  # far apart, 16-byte aligned, never dereferenced
S444, S420 = 0, 1
WIDE = (1 << 35) - 15      # 2^32 - 1 tiles a row for 4:4:4; 2^32 once padded to whole MCUs


def _p(x):
    return None if x is None else ctypes.c_void_p(x)


def _t(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# a 15x17 frame: padded to 16x24 (4:4:4: y, cb, cr 768 bytes each) or 16x32 (4:2:0: y 1024, cb and cr 256)
def _fwd(L, rgb=RGB, pitch=51, y=Y, cb=CB, cr=CR, h=15, w=17, sub=S420, ql=None, qc=None, flags=0):
    return L.hpdct_forward_rgb_frame(_p(rgb), pitch, _p(y), _p(cb), _p(cr), h, w, sub, _t(ql), _t(qc), flags, None)


def _inv(L, rgb=RGB, pitch=51, y=Y, cb=CB, cr=CR, h=15, w=17, sub=S420, ql=None, qc=None, flags=0):
    return L.hpdct_inverse_rgb_frame(_p(y), _p(cb), _p(cr), _p(rgb), pitch, h, w, sub, _t(ql), _t(qc), flags, None)


def _nan_chroma():
    q = np.array(CHROMA, np.float32)
    q[5] = np.nan
    return q


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["forward", "inverse"])
def test_frame_arguments_rejected(hp, call):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    nan = _nan_chroma()

    def passes_the_pointer_checks(**kw):
        """The call gets as far as the tables, the last thing judged."""
        return call(L, qc=nan, **kw) == 1 and b"chroma" in err()

    assert passes_the_pointer_checks()
    for name in ("rgb", "y", "cb", "cr"):
        assert call(L, **{name: None}) == 1
        assert b"null" in err()
    for h, w in ((0, 17), (15, 0), (-15, 17), (15, -1)):
        assert call(L, h=h, w=w) == 1
        assert b"positive" in err()
    # any positive size is taken, in both subsamplings
    for h, w in ((1, 1), (7, 9), (1080, 1920), (667, 1000)):
        for sub in (S444, S420):
            assert passes_the_pointer_checks(h=h, w=w, pitch=3 * w, sub=sub)
    for pitch in (50, 0, -64):
        assert call(L, pitch=pitch) == 1
        assert b"pitch_bytes" in err()
    assert passes_the_pointer_checks(pitch=51) and passes_the_pointer_checks(pitch=52) and \
        passes_the_pointer_checks(pitch=4096)
    # the padded tile-count limit
    assert call(L, h=1 << 23, w=1 << 23, pitch=3 << 23, sub=S444) == 1 and b"too large" in err()
    assert passes_the_pointer_checks(h=8, w=WIDE, pitch=3 * WIDE, sub=S444, y=1 << 50, cb=1 << 52, cr=1 << 54)
    assert call(L, h=8, w=WIDE, pitch=3 * WIDE, sub=S420) == 1 and b"too large" in err()
    assert call(L, pitch=(1 << 63) // 4) == 1 and b"too large" in err()
    for sub in (2, -1, 77):
        assert call(L, sub=sub) == 1
        assert b"subsampling" in err()
    assert call(L, flags=0x80) == 2
    assert call(L, flags=hp.BLOCKS_NATURAL | 0x2) == 2
    for name, base in (("y", Y), ("cb", CB), ("cr", CR)):
        assert call(L, **{name: base + 8}) == 1
        assert b"aligned" in err()
    # d_rgb has no alignment rule
    for off in (1, 2, 4, 8):
        assert passes_the_pointer_checks(rgb=RGB + off)


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["forward", "inverse"])
def test_frame_overlap_uses_the_pitched_extent_and_the_padded_sizes(hp, call):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    nan = _nan_chroma()

    def overlap(**kw):
        st = call(L, qc=nan, **kw)
        assert st == 1 and (b"overlap" in err() or b"chroma" in err()), (st, err())
        return b"overlap" in err()

    # dense: the extent is 14 * 51 + 51 = 765 bytes
    assert not overlap(rgb=RGB + 3, y=RGB + 768)
    assert overlap(rgb=RGB + 4, y=RGB + 768)
    # pitch 64: 14 * 64 + 51 = 947 bytes, caught only when the pitched extent is used
    assert not overlap(pitch=51, y=RGB + 768)
    assert overlap(pitch=64, y=RGB + 768)
    assert overlap(pitch=64, y=RGB + 944)
    assert not overlap(pitch=64, y=RGB + 960)
    # one row: the pitch does not count
    assert not overlap(h=1, pitch=4096, y=RGB + 64)
    assert overlap(h=1, pitch=4096, y=RGB + 48)
    # the block arrays have the padded frame's sizes
    assert overlap(cr=CB + 240) and not overlap(cr=CB + 256)
    assert overlap(cb=Y + 1008) and not overlap(cb=Y + 1024)
    assert overlap(cr=CB + 752, sub=S444) and not overlap(cr=CB + 768, sub=S444)
    assert overlap(rgb=Y - 752) and not overlap(rgb=Y - 768)


def test_frame_tables_rejected(hp):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    good = np.array(CHROMA, np.float32)
    for call in (_fwd, _inv):
        for bad_value in (np.nan, np.inf, 0.0):
            bad = good.copy()
            bad[63] = bad_value
            assert call(L, ql=bad, qc=good) == 1 and b"luma" in err() and b"finite and non-zero" in err()
            assert call(L, qc=bad) == 1 and b"chroma" in err()
        tiny = np.full(64, 1.0 / 64.0, np.float32)
        assert call(L, ql=tiny) == 3 and b"luma" in err() and b"int16" in err()
        assert call(L, qc=tiny) == 3 and b"chroma" in err()
        assert call(L, ql=tiny, pitch=50) == 1            # arguments are still judged first


def test_frame_geometry(hp):
    g = hp.rgb_frame_geometry
    assert g(1, 1, "444") == (8, 8, 1, 1)
    assert g(1, 1, "420") == (16, 16, 4, 1)
    assert g(1080, 1920, "444") == (1080, 1920, 135 * 240, 135 * 240)
    assert g(1080, 1920, "420") == (1088, 1920, 136 * 240, 68 * 120)
    assert g(667, 1000, "444") == (672, 1000, 84 * 125, 84 * 125)
    assert g(667, 1000, "420") == (672, 1008, 84 * 126, 42 * 63)
    assert g(8, WIDE, "444") == (8, (1 << 35) - 8, (1 << 32) - 1, (1 << 32) - 1)
    assert g(16, 16) == (16, 16, 4, 1)                    # 4:2:0 is the default, as forward_rgb_frame's
    for h, w, sub in ((0, 16, "420"), (16, -1, "444"), (8, WIDE, "420"), (1 << 23, 1 << 23, "444"),
                      ((1 << 63) - 1, 16, "420")):
        with pytest.raises(hp.HpdctError) as e:
            g(h, w, sub)
        assert e.value.status == 1
    with pytest.raises(ValueError):
        g(16, 16, "422")
    L = hp.load_library()
    assert L.hpdct_rgb_frame_geometry(13, 515, S444, None, None, None, None) == 0       # every output may be NULL
    hpw = ctypes.c_int64(-1)
    assert L.hpdct_rgb_frame_geometry(13, 515, S420, None, ctypes.byref(hpw), None, None) == 0 and hpw.value == 528
    assert L.hpdct_rgb_frame_geometry(13, 515, 3, None, None, None, None) == 1
    assert b"subsampling" in L.hpdct_last_error_string()


def test_frame_symbols_are_declared(hp):
    text = open(os.path.join(ROOT, "include", "hpdct.h")).read()
    for name in ("hpdct_rgb_frame_geometry", "hpdct_forward_rgb_frame", "hpdct_inverse_rgb_frame"):
        assert name in hp.C_SYMBOLS and name + "(" in text
        getattr(hp.load_library(), name)


def test_rgb_frame_policy_table(tmp_path):
    """tests/tools/policy_rgb_frame_check.cpp: a whole-unit aligned call gets exactly the Choice of the existing
    policy rows, a ragged or unaligned one the clip variant with the padded grid's wave count."""
    host_programs.policy_check("policy_rgb_frame_check", tmp_path)


def test_frame_validation_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/tools/asan_rgb_frame_check.cpp, its own main) drives the validation paths
    with the C ABI's host sources (tests/tools/asan.mk's HOST) compiled by g++ under tests/tools/asan.mk's ASan + UBSan flags and the library's kernel
    objects linked as they are.  CPU only: nothing is launched, nothing is loaded into Python."""
    host_programs.sanitised_check("asan_rgb_frame_check", tmp_path, "hpdct_rgb_fwd420_clip.o")


class _View(FakeDev):
    """A FakeDev with strides and an address (still never dereferenced)."""

    def __init__(self, shape, dtype, ptr=None, strides=None, **kw):
        super().__init__(shape, dtype, **kw)
        if strides is None:
            strides, n = [], 1
            for s in reversed(self.shape):
                strides.insert(0, n)
                n *= s
        self._strides, self._ptr = tuple(strides), ptr

    def stride(self, d=None):
        return self._strides if d is None else self._strides[d]

    def data_ptr(self):
        if self._ptr is None:
            raise AssertionError("the library must not be reached")
        return self._ptr


def test_forward_rgb_frame_wrapper_checks(hp):
    import torch as t
    rgb = _View((15, 17, 3), t.uint8, 1 << 20)
    yb, cb = _View((2, 4, 64), t.int16, 1 << 21), _View((1, 2, 64), t.int16, 1 << 22)
    cr = _View((1, 2, 64), t.int16, 1 << 23)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.forward_rgb_frame(_View((15, 17, 3), t.uint8, cuda=False))
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.forward_rgb_frame(t.zeros((15, 17, 3), dtype=t.uint8))           # a real CPU tensor
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_rgb_frame(_View((15, 17, 3), t.float32))
    with pytest.raises(hp.HpdctError, match=r"\(H, W, 3\)"):
        hp.forward_rgb_frame(_View((15, 17), t.uint8))
    with pytest.raises(hp.HpdctError, match=r"\(H, W, 3\)"):
        hp.forward_rgb_frame(_View((2, 15, 17, 3), t.uint8))                # no stacks: a frame has its own edges
    with pytest.raises(hp.HpdctError, match=r"\(H, W, 3\)"):
        hp.forward_rgb_frame(_View((15, 17, 4), t.uint8))
    with pytest.raises(hp.HpdctError, match="positive"):
        hp.forward_rgb_frame(_View((0, 17, 3), t.uint8))
    # strides: channels and pixels dense, rows at least 3 W apart
    with pytest.raises(hp.HpdctError, match="interleaved"):
        hp.forward_rgb_frame(_View((15, 17, 3), t.uint8, strides=(102, 6, 2)))      # every other byte
    with pytest.raises(hp.HpdctError, match="interleaved"):
        hp.forward_rgb_frame(_View((15, 17, 3), t.uint8, strides=(68, 4, 1)))       # an RGBA frame's RGB
    with pytest.raises(hp.HpdctError, match="interleaved"):
        hp.forward_rgb_frame(_View((15, 17, 3), t.uint8, strides=(3, 45, 1)))       # a transposed view
    with pytest.raises(hp.HpdctError, match="3\\*W = 51"):
        hp.forward_rgb_frame(_View((15, 17, 3), t.uint8, strides=(50, 3, 1)))
    with pytest.raises(hp.HpdctError, match="3\\*W = 51"):
        hp.forward_rgb_frame(_View((15, 17, 3), t.uint8, strides=(0, 3, 1)))        # an expanded row
    # block-array sizes against the padded geometry: 15x17 pads to 16x32 (4:2:0) or 16x24 (4:4:4)
    with pytest.raises(hp.HpdctError, match="y blocks holds"):
        hp.forward_rgb_frame(rgb, out=(_View((2, 3, 64), t.int16), cb, cr))
    with pytest.raises(hp.HpdctError, match="cb blocks holds"):
        hp.forward_rgb_frame(rgb, out=(yb, _View((1, 1, 64), t.int16), cr))
    with pytest.raises(hp.HpdctError, match="cr blocks holds"):
        hp.forward_rgb_frame(rgb, out=(yb, cb, _View((1, 1, 64), t.int16)))
    with pytest.raises(hp.HpdctError, match="cb blocks holds"):
        hp.forward_rgb_frame(rgb, subsampling="444", out=(yb, cb, cr))      # 4:4:4 chroma is full size
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_rgb_frame(rgb, out=(_View((2, 4, 64), t.float32), cb, cr))
    with pytest.raises(hp.HpdctError, match="contiguous"):
        hp.forward_rgb_frame(rgb, out=(yb, _View((1, 2, 64), t.int16, contiguous=False), cr))
    with pytest.raises(hp.HpdctError, match="is on"):
        hp.forward_rgb_frame(rgb, out=(yb, cb, _View((1, 2, 64), t.int16, device="cuda:1")))
    with pytest.raises(ValueError):
        hp.forward_rgb_frame(rgb, subsampling="422", out=(yb, cb, cr))
    with pytest.raises(ValueError):
        hp.forward_rgb_frame(rgb, order="diagonal", out=(yb, cb, cr))
    # overlap with the pitched extent: dense 765 bytes, pitch 64: 947
    y_near = _View((2, 4, 64), t.int16, (1 << 20) + 768)
    with pytest.raises(hp.HpdctError, match="rgb and y buffers overlap"):
        hp.forward_rgb_frame(_View((15, 17, 3), t.uint8, 1 << 20, strides=(64, 3, 1)), out=(y_near, cb, cr))
    with pytest.raises(hp.HpdctError, match="64 floats"):                   # dense: no overlap, on to the tables
        hp.forward_rgb_frame(rgb, q_chroma=np.ones(63, np.float32), out=(y_near, cb, cr))
    with pytest.raises(hp.HpdctError, match="cb and cr buffers overlap"):
        hp.forward_rgb_frame(rgb, out=(yb, cb, _View((1, 2, 64), t.int16, (1 << 22) + 240)))
    with pytest.raises(hp.HpdctError, match="y blocks holds"):
        hp.bind_rgb_frame("fwd", rgb, _View((2, 3, 64), t.int16), cb, cr)
    with pytest.raises(hp.HpdctError, match="interleaved"):
        hp.bind_rgb_frame("inv", _View((15, 17, 3), t.uint8, strides=(68, 4, 1)), yb, cb, cr)
    with pytest.raises(ValueError):
        hp.bind_rgb_frame("both", rgb, yb, cb, cr)


def test_inverse_rgb_frame_wrapper_checks(hp):
    import torch as t
    yb, cb = _View((2, 4, 64), t.int16, 1 << 21), _View((1, 2, 64), t.int16, 1 << 22)
    cr = _View((1, 2, 64), t.int16, 1 << 23)
    out = _View((15, 17, 3), t.uint8, 1 << 20, strides=(64, 3, 1))
    kw = dict(height=15, width=17, subsampling="420")
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.inverse_rgb_frame(_View((2, 4, 64), t.int16, cuda=False), cb, cr, out=out, **kw)
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_rgb_frame(_View((2, 4, 64), t.int8), cb, cr, out=out, **kw)
    with pytest.raises(TypeError):
        hp.inverse_rgb_frame(yb, cb, cr, out=out, subsampling="420")        # the frame's size is not in the blocks
    with pytest.raises(TypeError):
        hp.inverse_rgb_frame(yb, cb, cr, out=out, height=15, width=17)      # nor is the subsampling
    with pytest.raises(hp.HpdctError, match="positive"):
        hp.inverse_rgb_frame(yb, cb, cr, out=out, height=0, width=17, subsampling="420")
    with pytest.raises(hp.HpdctError, match="rgb is 15x16"):
        hp.inverse_rgb_frame(yb, cb, cr, out=_View((15, 16, 3), t.uint8), **kw)
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_rgb_frame(yb, cb, cr, out=_View((15, 17, 3), t.float32), **kw)
    with pytest.raises(hp.HpdctError, match="interleaved"):
        hp.inverse_rgb_frame(yb, cb, cr, out=_View((15, 17, 3), t.uint8, strides=(68, 4, 1)), **kw)
    with pytest.raises(hp.HpdctError, match="3\\*W = 51"):
        hp.inverse_rgb_frame(yb, cb, cr, out=_View((15, 17, 3), t.uint8, strides=(48, 3, 1)), **kw)
    with pytest.raises(hp.HpdctError, match="is on"):
        hp.inverse_rgb_frame(yb, cb, cr, out=_View((15, 17, 3), t.uint8, device="cuda:1"), **kw)
    with pytest.raises(hp.HpdctError, match="y blocks holds"):
        hp.inverse_rgb_frame(_View((2, 3, 64), t.int16), cb, cr, out=out, **kw)
    with pytest.raises(hp.HpdctError, match="cr blocks holds"):
        hp.inverse_rgb_frame(yb, cb, _View((1, 1, 64), t.int16), out=out, **kw)
    with pytest.raises(hp.HpdctError, match="cb blocks holds"):
        hp.inverse_rgb_frame(yb, cb, cr, out=out, height=15, width=17, subsampling="444")
    with pytest.raises(hp.HpdctError, match="rgb and y buffers overlap"):
        hp.inverse_rgb_frame(_View((2, 4, 64), t.int16, (1 << 20) + 944), cb, cr, out=out, **kw)
    with pytest.raises(hp.HpdctError, match="64 floats"):                   # 960 is past the 947-byte extent
        hp.inverse_rgb_frame(_View((2, 4, 64), t.int16, (1 << 20) + 960), cb, cr, out=out,
                             q_luma=np.ones(65, np.float32), **kw)
