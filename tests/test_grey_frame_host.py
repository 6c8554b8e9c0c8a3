"""Grey frames of any size, row pitch and quant table, the CPU side (no GPU, no
kernel runs):

- hpdct_grey_frame_geometry, hpdct_forward_grey_frame and hpdct_inverse_grey_frame
  validate every argument and return the documented status before any device
  work (the pointers here are never dereferenced);
- the policy rows of the two launchers for whole-tile and for ragged or
  unaligned frames, and the validation paths once more in a stand-alone program
  under ASan + UBSan;
- the Python wrappers check dtype, strides, sizes and overlap before the library
  is reached, and jpeg_decode its quant keyword before it reads the file.
"""
import ctypes
import os

import numpy as np
import pytest

import host_programs
from test_rgb_frame_host import _View

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG, BLK = 1 << 20, 1 << 30          # far apart, 16-byte aligned, never dereferenced
WIDE = (1 << 35) - 15                # 2^32 - 1 tiles a row; eight pixels more pad to 2^32


def _p(x):
    return None if x is None else ctypes.c_void_p(x)


def _t(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# a 15x17 frame: padded to 16x24, 6 blocks of 128 bytes
def _fwd(L, img=IMG, pitch=17, blk=BLK, h=15, w=17, q=None, flags=0):
    return L.hpdct_forward_grey_frame(_p(img), pitch, _p(blk), h, w, _t(q), flags, None)


def _inv(L, img=IMG, pitch=17, blk=BLK, h=15, w=17, q=None, flags=0):
    return L.hpdct_inverse_grey_frame(_p(blk), _p(img), pitch, h, w, _t(q), flags, None)


def _nan_table(hp):
    q = hp.default_quant_table().reshape(-1).copy()
    q[5] = np.nan
    return q


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["forward", "inverse"])
def test_frame_arguments_rejected(hp, call):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    nan = _nan_table(hp)

    def passes_the_argument_checks(**kw):
        """The call gets as far as the table, the last thing judged."""
        return call(L, q=nan, **kw) == 1 and b"finite and non-zero" in err()

    assert passes_the_argument_checks()
    for name in ("img", "blk"):
        assert call(L, **{name: None}) == 1
        assert b"null" in err()
    for h, w in ((0, 17), (15, 0), (-15, 17), (15, -1)):
        assert call(L, h=h, w=w) == 1
        assert b"positive" in err()
    # any positive size is taken
    for h, w in ((1, 1), (7, 9), (8, 8), (1080, 1920), (667, 1000)):
        assert passes_the_argument_checks(h=h, w=w, pitch=w)
    for pitch in (16, 0, -64):
        assert call(L, pitch=pitch) == 1
        assert b"pitch_bytes" in err()
    assert passes_the_argument_checks(pitch=17) and passes_the_argument_checks(pitch=18) and \
        passes_the_argument_checks(pitch=4096)
    # the padded tile-count limit
    assert call(L, h=1 << 23, w=1 << 23, pitch=1 << 23) == 1 and b"too large" in err()
    assert passes_the_argument_checks(h=8, w=WIDE, pitch=WIDE, blk=1 << 50)
    assert call(L, h=8, w=WIDE + 8, pitch=WIDE + 8) == 1 and b"too large" in err()
    assert call(L, h=9, w=WIDE, pitch=WIDE) == 1 and b"too large" in err()
    # the extent (height - 1) * pitch + width overflows an int64
    assert call(L, pitch=(1 << 63) // 4) == 1 and b"too large" in err()
    assert call(L, flags=0x80) == 2
    assert call(L, flags=hp.BLOCKS_NATURAL | 0x2) == 2
    assert passes_the_argument_checks(flags=hp.BLOCKS_NATURAL)
    for off in (2, 8):
        assert call(L, blk=BLK + off) == 1
        assert b"aligned" in err()
    # d_image has no alignment rule
    for off in (1, 2, 3, 4, 8):
        assert passes_the_argument_checks(img=IMG + off)


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["forward", "inverse"])
def test_frame_overlap_uses_the_pitched_extent_and_the_padded_size(hp, call):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    nan = _nan_table(hp)

    def overlap(**kw):
        st = call(L, q=nan, **kw)
        assert st == 1 and (b"overlap" in err() or b"finite" in err()), (st, err())
        return b"overlap" in err()

    # dense: the extent is 14 * 17 + 17 = 255 bytes
    assert not overlap(img=IMG + 1, blk=IMG + 256)
    assert overlap(img=IMG + 2, blk=IMG + 256)
    # pitch 64: 14 * 64 + 17 = 913 bytes, caught only when the pitched extent is used
    assert not overlap(pitch=17, blk=IMG + 256)
    assert overlap(pitch=64, blk=IMG + 256)
    assert overlap(pitch=64, blk=IMG + 912)
    assert not overlap(pitch=64, blk=IMG + 928)
    # one row: the pitch does not count
    assert not overlap(h=1, pitch=4096, blk=IMG + 32)
    assert overlap(h=1, pitch=4096, blk=IMG + 16)
    # the block array has the padded frame's size: 6 blocks, 768 bytes
    assert overlap(img=BLK + 767) and not overlap(img=BLK + 768)
    assert overlap(img=BLK - 254) and not overlap(img=BLK - 255)
    # an extent that would wrap the address space
    assert call(L, img=(1 << 64) - 100) == 1 and b"wrap" in err()


def test_frame_tables_rejected(hp):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    good = hp.default_quant_table().reshape(-1).copy()
    for call in (_fwd, _inv):
        for bad_value in (np.nan, np.inf, -np.inf, 0.0):
            bad = good.copy()
            bad[63] = bad_value
            assert call(L, q=bad) == 1 and b"finite and non-zero" in err()
        tiny = np.full(64, 1.0 / 64.0, np.float32)
        assert call(L, q=tiny) == 3 and b"int16" in err()
        assert call(L, q=tiny, pitch=16) == 1 and b"pitch_bytes" in err()     # arguments are still judged first
        # NULL is the library table at the time of the call
        hp.set_quant_table(tiny)
        try:
            assert call(L) == 3 and b"int16" in err()
            assert call(L, q=bad) == 1                                        # a per-call table passes it by
        finally:
            hp.set_quant_table(None)
        assert np.array_equal(hp.get_quant_table().reshape(-1), good)


def test_frame_geometry(hp):
    g = hp.grey_frame_geometry
    assert g(1, 1) == (8, 8, 1)
    assert g(7, 9) == (8, 16, 2)
    assert g(8, 8) == (8, 8, 1)
    assert g(1080, 1920) == (1080, 1920, 135 * 240)
    assert g(667, 1000) == (672, 1000, 84 * 125)
    assert g(8, WIDE) == (8, (1 << 35) - 8, (1 << 32) - 1)
    for h, w in ((0, 16), (16, -1), (8, WIDE + 8), (9, WIDE), (1 << 23, 1 << 23), ((1 << 63) - 1, 16)):
        with pytest.raises(hp.HpdctError) as e:
            g(h, w)
        assert e.value.status == 1
    L = hp.load_library()
    assert L.hpdct_grey_frame_geometry(13, 515, None, None, None) == 0          # every output may be NULL
    wp = ctypes.c_int64(-1)
    assert L.hpdct_grey_frame_geometry(13, 515, None, ctypes.byref(wp), None) == 0 and wp.value == 520
    assert L.hpdct_grey_frame_geometry(8, WIDE + 8, None, None, None) == 1
    assert b"too large" in L.hpdct_last_error_string()


def test_frame_symbols_are_declared(hp):
    text = open(os.path.join(ROOT, "include", "hpdct.h")).read()
    for name in ("hpdct_grey_frame_geometry", "hpdct_forward_grey_frame", "hpdct_inverse_grey_frame"):
        assert name in hp.C_SYMBOLS and name + "(" in text
        getattr(hp.load_library(), name)


def test_grey_frame_policy_table(tmp_path):
    """tests/tools/policy_grey_frame_check.cpp: a whole-tile aligned call gets the launch of the blocks rows, a
    ragged or unaligned one the clip variant with the padded grid's wave count."""
    host_programs.policy_check("policy_grey_frame_check", tmp_path)


def test_frame_validation_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/tools/asan_grey_frame_check.cpp, its own main) drives the validation paths
    with the C ABI's host sources (tests/tools/asan.mk's HOST) compiled by g++ under asan.mk's ASan + UBSan flags
    and the library's kernel objects linked as they are.  CPU only: nothing is launched, nothing is loaded into
    Python."""
    host_programs.sanitised_check("asan_grey_frame_check", tmp_path, "hpdct_grey_frame_fwd_clip.o")


def test_forward_grey_frame_wrapper_checks(hp):
    import torch as t
    img = _View((15, 17), t.uint8, 1 << 20)
    blk = _View((2, 3, 64), t.int16, 1 << 21)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.forward_grey_frame(_View((15, 17), t.uint8, cuda=False))
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.forward_grey_frame(t.zeros((15, 17), dtype=t.uint8))             # a real CPU tensor
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_grey_frame(_View((15, 17), t.float32))
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_grey_frame(_View((15, 17), t.int8))
    with pytest.raises(hp.HpdctError, match=r"\(H, W\)"):
        hp.forward_grey_frame(_View((15, 17, 1), t.uint8))
    with pytest.raises(hp.HpdctError, match=r"\(H, W\)"):
        hp.forward_grey_frame(_View((255,), t.uint8))
    with pytest.raises(hp.HpdctError, match="positive"):
        hp.forward_grey_frame(_View((0, 17), t.uint8))
    # strides: pixels dense, rows at least W apart
    with pytest.raises(hp.HpdctError, match=r"stride\(1\) == 1"):
        hp.forward_grey_frame(_View((15, 17), t.uint8, strides=(34, 2)))    # every other byte
    with pytest.raises(hp.HpdctError, match=r"stride\(1\) == 1"):
        hp.forward_grey_frame(_View((15, 17), t.uint8, strides=(1, 15)))    # a transposed view
    with pytest.raises(hp.HpdctError, match="W = 17"):
        hp.forward_grey_frame(_View((15, 17), t.uint8, strides=(16, 1)))
    with pytest.raises(hp.HpdctError, match="W = 17"):
        hp.forward_grey_frame(_View((15, 17), t.uint8, strides=(0, 1)))     # an expanded row
    # the block array against the padded geometry: 15x17 pads to 16x24, 6 blocks
    with pytest.raises(hp.HpdctError, match="blocks holds 320 elements, 384 needed"):
        hp.forward_grey_frame(img, out=_View((1, 5, 64), t.int16))
    with pytest.raises(hp.HpdctError, match="blocks holds"):
        hp.forward_grey_frame(img, out=_View((15, 17), t.int16))            # the frame's own size is too small
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.forward_grey_frame(img, out=_View((2, 3, 64), t.float32))
    with pytest.raises(hp.HpdctError, match="contiguous"):
        hp.forward_grey_frame(img, out=_View((2, 3, 64), t.int16, contiguous=False))
    with pytest.raises(hp.HpdctError, match="is on"):
        hp.forward_grey_frame(img, out=_View((2, 3, 64), t.int16, device="cuda:1"))
    with pytest.raises(ValueError):
        hp.forward_grey_frame(img, order="diagonal", out=blk)
    # overlap with the pitched extent: dense 255 bytes, pitch 64: 913
    near = _View((2, 3, 64), t.int16, (1 << 20) + 256)
    with pytest.raises(hp.HpdctError, match="image and blocks buffers overlap"):
        hp.forward_grey_frame(_View((15, 17), t.uint8, 1 << 20, strides=(64, 1)), out=near)
    with pytest.raises(hp.HpdctError, match="64 floats"):                   # dense: no overlap, on to the table
        hp.forward_grey_frame(img, q=np.ones(63, np.float32), out=near)
    with pytest.raises(hp.HpdctError, match="image and blocks buffers overlap"):
        hp.forward_grey_frame(_View((15, 17), t.uint8, (1 << 21) + 767), out=blk)
    with pytest.raises(hp.HpdctError, match="blocks holds"):
        hp.bind_grey_frame("fwd", img, _View((1, 5, 64), t.int16))
    with pytest.raises(hp.HpdctError, match=r"stride\(1\) == 1"):
        hp.bind_grey_frame("inv", _View((15, 17), t.uint8, strides=(34, 2)), blk)
    with pytest.raises(hp.HpdctError, match="image and blocks buffers overlap"):
        hp.bind_grey_frame("inv", _View((15, 17), t.uint8, 1 << 20, strides=(64, 1)), near)
    with pytest.raises(ValueError):
        hp.bind_grey_frame("both", img, blk)


def test_inverse_grey_frame_wrapper_checks(hp):
    import torch as t
    blk = _View((2, 3, 64), t.int16, 1 << 21)
    out = _View((15, 17), t.uint8, 1 << 20, strides=(64, 1))
    kw = dict(height=15, width=17)
    with pytest.raises(hp.HpdctError, match="CUDA"):
        hp.inverse_grey_frame(_View((2, 3, 64), t.int16, cuda=False), out=out, **kw)
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_grey_frame(_View((2, 3, 64), t.int8), out=out, **kw)
    with pytest.raises(TypeError):
        hp.inverse_grey_frame(blk, out=out)                                 # the frame's size is not in the blocks
    with pytest.raises(hp.HpdctError, match="positive"):
        hp.inverse_grey_frame(blk, out=out, height=0, width=17)
    with pytest.raises(hp.HpdctError, match="image is 15x16"):
        hp.inverse_grey_frame(blk, out=_View((15, 16), t.uint8), **kw)
    with pytest.raises(hp.HpdctError, match="dtype"):
        hp.inverse_grey_frame(blk, out=_View((15, 17), t.float32), **kw)    # uint8 output only
    with pytest.raises(hp.HpdctError, match=r"stride\(1\) == 1"):
        hp.inverse_grey_frame(blk, out=_View((15, 17), t.uint8, strides=(34, 2)), **kw)
    with pytest.raises(hp.HpdctError, match="W = 17"):
        hp.inverse_grey_frame(blk, out=_View((15, 17), t.uint8, strides=(16, 1)), **kw)
    with pytest.raises(hp.HpdctError, match="is on"):
        hp.inverse_grey_frame(blk, out=_View((15, 17), t.uint8, device="cuda:1"), **kw)
    with pytest.raises(hp.HpdctError, match="blocks holds 320 elements, 384 needed"):
        hp.inverse_grey_frame(_View((1, 5, 64), t.int16), out=out, **kw)
    with pytest.raises(hp.HpdctError, match="image and blocks buffers overlap"):
        hp.inverse_grey_frame(_View((2, 3, 64), t.int16, (1 << 20) + 912), out=out, **kw)
    with pytest.raises(hp.HpdctError, match="64 floats"):                   # 928 is past the 913-byte extent
        hp.inverse_grey_frame(_View((2, 3, 64), t.int16, (1 << 20) + 928), out=out, q=np.ones(65, np.float32), **kw)


def test_jpeg_keywords_rejected_before_the_file_is_read(hp):
    with pytest.raises(ValueError, match="quant"):
        hp.jpeg_decode(b"", quant="other")
    with pytest.raises(ValueError, match="quant"):
        hp.jpeg_decode(b"not a file", quant=None)
    import torch as t
    with pytest.raises(hp.HpdctError, match="chroma") as e:
        hp.jpeg_encode(_View((15, 17), t.uint8), q_chroma=np.ones(64, np.float32))
    assert e.value.status == 2
