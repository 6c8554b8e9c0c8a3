"""The exact DCT on the frame calls (HPDCT_FRAME_DCT, transform="dct"), the CPU side (no GPU, no kernel runs):

- hpdct_dct_transform is the float64 formula rounded to fp32, bit for bit, and orthonormal within 1e-6;
- the four frame calls take 0x100 alone and with HPDCT_BLOCKS_NATURAL (the pointers here are never
  dereferenced: each call is stopped by a table with a NaN, the last thing judged), refuse it with any other
  bit, and every other entry point still refuses it;
- the range rule under the flag is judged with the DCT's row norms;
- the Python keyword is validated before anything else is looked at;
- the policy rows (tests/tools/policy_dct_check.cpp) and the new argument paths under ASan + UBSan
  (tests/tools/asan_dct_frames_check.cpp), both stand-alone programs.
"""
import os

import numpy as np
import pytest

import host_programs
import test_grey_frame_host as G
import test_rgb_frame_host as C
from test_rgb_frame_host import _View

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DCT = 0x100


def formula():
    """fp32 of sqrt(1/8) in row 0 and of 0.5 * cos((2i+1) v pi / 16) elsewhere, evaluated in float64."""
    i = np.arange(8, dtype=np.float64)
    rows = [np.full(8, np.sqrt(1.0 / 8.0))] + [0.5 * np.cos((2.0 * i + 1.0) * v * np.pi / 16.0) for v in range(1, 8)]
    return np.array(rows, np.float64).astype(np.float32)


def test_dct_transform_is_the_formula(hp):
    t = hp.dct_transform()
    assert t.dtype == np.float32 and t.shape == (8, 8)
    assert np.array_equal(t.view(np.uint32), formula().view(np.uint32))
    assert (t != 0).all()                                                   # nothing to skip in a chain
    t64 = t.astype(np.float64)
    assert np.abs(t64 @ t64.T - np.eye(8)).max() < 1e-6
    assert float(np.abs(t64).sum(axis=1).max()) <= 2.8284272                # the bound the 3-op quotient's range uses
    assert not np.array_equal(t, hp.default_transform())
    assert hp.FRAME_DCT == DCT and hp.FRAME_TRANSFORMS == {"hpappr": 0, "dct": DCT}


def test_symbol_is_declared(hp):
    text = open(os.path.join(ROOT, "include", "hpdct.h")).read()
    assert "hpdct_dct_transform" in hp.C_SYMBOLS and "hpdct_dct_transform(" in text
    getattr(hp.load_library(), "hpdct_dct_transform")
    assert "#define HPDCT_FRAME_DCT 0x100u" in text
    hp.load_library().hpdct_dct_transform(None)                             # NULL: nothing is written


FRAME_CALLS = [(G._fwd, "q"), (G._inv, "q"), (C._fwd, "qc"), (C._inv, "qc")]
FRAME_IDS = ["grey-forward", "grey-inverse", "rgb-forward", "rgb-inverse"]


@pytest.mark.parametrize("call,table", FRAME_CALLS, ids=FRAME_IDS)
def test_frame_calls_take_the_flag(hp, call, table):
    L = hp.load_library()
    err = L.hpdct_last_error_string
    nan = G._nan_table(hp)
    subs = [{}] if table == "q" else [{"sub": C.S444}, {"sub": C.S420}]
    for kw in subs:
        for flags in (DCT, DCT | hp.BLOCKS_NATURAL):
            # past every argument check, as far as the table
            assert call(L, flags=flags, **{table: nan}, **kw) == 1 and b"finite and non-zero" in err(), hex(flags)
        for flags in (DCT | 0x2, DCT | 0x80, 0x102, 0x180, 0x200, DCT | 0x200):
            assert call(L, flags=flags, **kw) == 2 and b"flag" in err(), hex(flags)
        # the other arguments are judged as without the flag
        assert call(L, flags=DCT, pitch=16, **kw) == 1 and b"pitch_bytes" in err()
        assert call(L, flags=DCT, h=0, **kw) == 1 and b"positive" in err()


def test_range_rule_uses_the_dct_row_norms(hp):
    """1/64 everywhere overflows int16 under either matrix.  An entry of 0.02 at (7, 7) does under the DCT only:
    HpApprDCT's row 7 has L1 norm 1.414 (128 * 2 / 0.02 = 12,800), the DCT's 2.563 (128 * 6.57 / 0.02 = 42,040).
    Only refused calls are made: the table that passes without the flag is paired with a refused pitch."""
    L = hp.load_library()
    err = L.hpdct_last_error_string
    tiny = np.full(64, 1.0 / 64.0, np.float32)
    edge = hp.default_quant_table().reshape(-1).copy()
    edge[63] = np.float32(0.02)
    for call in (G._fwd, G._inv):
        assert call(L, q=tiny, flags=DCT) == 3 and b"int16" in err()
        assert call(L, q=edge, flags=DCT) == 3 and b"int16" in err()
        assert call(L, q=edge, flags=DCT, pitch=16) == 1 and b"pitch_bytes" in err()   # arguments first
    for call in (C._fwd, C._inv):
        assert call(L, ql=edge, flags=DCT) == 3 and b"luma" in err()
        assert call(L, qc=edge, flags=DCT | hp.BLOCKS_NATURAL) == 3 and b"chroma" in err()
    t = hp.dct_transform().astype(np.float64)
    assert 128.0 * np.abs(t[7]).sum() ** 2 / 0.02 > 32767 > 128.0 * np.abs(hp.default_transform()[7]).sum() ** 2 / 0.02


def test_other_entry_points_still_refuse_the_flag(hp):
    import test_rgb_host as R
    L = hp.load_library()
    err = L.hpdct_last_error_string
    A, B = 1 << 20, 1 << 30
    for flags in (DCT, DCT | hp.BLOCKS_NATURAL):
        assert L.hpdct_forward_blocks(G._p(A), G._p(B), 16, 32, flags, None) == 2 and b"flag" in err()
        assert L.hpdct_inverse_blocks(G._p(B), G._p(A), hp.U8, 16, 32, flags, None) == 2 and b"flag" in err()
        assert R._fwd(L, flags=flags) == 2 and b"flag" in err()
        assert R._inv(L, flags=flags) == 2 and b"flag" in err()
    assert L.hpdct_forward(G._p(A), hp.U8, G._p(B), hp.F32, 16, 32, None, DCT, None) == 2
    assert L.hpdct_inverse(G._p(B), hp.F32, G._p(A), hp.F32, 16, 32, None, DCT, None) == 2
    assert L.hpdct_encode_scan is not None                                  # (the entropy stage has no transform)


def test_python_keyword_is_validated(hp):
    import torch as t
    img, blk = _View((15, 17), t.uint8, 1 << 20), _View((2, 3, 64), t.int16, 1 << 21)
    rgb = _View((15, 17, 3), t.uint8, 1 << 22)
    ycc = [_View((2, 4, 64), t.int16, 1 << 23), _View((1, 2, 64), t.int16, 1 << 24),
           _View((1, 2, 64), t.int16, 1 << 25)]
    for bad in ("exact", "DCT", "", None, 1, np.eye(8, dtype=np.float32)):
        with pytest.raises(ValueError, match="transform"):
            hp.forward_grey_frame(img, out=blk, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            hp.inverse_grey_frame(blk, height=15, width=17, out=img, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            hp.bind_grey_frame("fwd", img, blk, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            hp.forward_rgb_frame(rgb, out=ycc, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            hp.inverse_rgb_frame(*ycc, height=15, width=17, subsampling="420", out=rgb, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            hp.bind_rgb_frame("inv", rgb, *ycc, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            hp.jpeg_encode(img, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            hp.jpeg_decode(b"not a file", transform=bad)
    # the other checks still run under the keyword
    with pytest.raises(hp.HpdctError, match="blocks holds 320 elements, 384 needed"):
        hp.forward_grey_frame(img, out=_View((1, 5, 64), t.int16), transform="dct")
    with pytest.raises(ValueError, match="order"):
        hp.forward_grey_frame(img, out=blk, order="diagonal", transform="dct")
    with pytest.raises(ValueError, match="quant"):
        hp.jpeg_decode(b"", quant="other", transform="dct")
    # the blocks calls have no such keyword
    with pytest.raises(TypeError):
        hp.forward_blocks(img, transform="dct")


def test_dct_policy_table(tmp_path):
    """tests/tools/policy_dct_check.cpp: under the DCT no row carries kVarJpegQ, the inverse does not read
    full_chain, and every launch shape is the HpApprDCT row's."""
    host_programs.policy_check("policy_dct_check", tmp_path)


def test_dct_argument_paths_clean_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/tools/asan_dct_frames_check.cpp, its own main) drives the flag's argument
    paths with the C ABI's host sources compiled by g++ under asan.mk's ASan + UBSan flags and the library's
    kernel objects linked as they are.  CPU only: nothing is launched, nothing is loaded into Python."""
    host_programs.sanitised_check("asan_dct_frames_check", tmp_path, "hpdct_dct_grey_fwd.o")
