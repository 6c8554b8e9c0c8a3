"""hpdct -- Python host-side mirror of the reference's DCT/IDCT call surface,
bound to the gfx950 library ``lib/libhpdct.so`` through its C-ABI
(``include/hpdct.h``) with ctypes.

PyTorch only supplies device memory and streams here: tensors are passed to
the library as raw device pointers and the kernels run on torch's current HIP
stream (or the one given).  There is no CPU or PyTorch fallback: if the
shared library is missing, every entry point raises ``HpdctLibraryError``.

Reference names mirrored (file:line into GerryDps/CUDA-DCT-IDCT):
  dct_all_blocks_cuda(image, h, w, T, result)   main_newAppr.cu:252-291
  idct_all_blocks_cuda(coef, h, w, T, result)   main_newAppr.cu:293-332
  set_quant_table(q)      cudaMemcpyToSymbol(const_quant_matrix, ...) :19,70
  convert_to_float / convert_to_unsigned_char   utils.cu:10-24
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HPDCT_LIB", os.path.join(_HERE, "lib", "libhpdct.so"))

# include/hpdct.h
U8, I8, F32 = 0, 1, 2
FLAG_NO_QUANT = 0x1
FLAG_WRITEBACK_SHIFT = 0x2
FLAG_NO_SHIFT = 0x4
FLAG_ROW_FIRST = 0x8
FLAG_WRITEBACK_DEQUANT = 0x10
BLOCKS_NATURAL = 0x1
BLOCK_ORDERS = {"zigzag": 0, "natural": BLOCKS_NATURAL}
FRAME_DCT = 0x100
# the frame calls' built-in matrix: HpApprDCT's (the reference's) or the exact DCT's
FRAME_TRANSFORMS = {"hpappr": 0, "dct": FRAME_DCT}

STATUS = {
    0: "HPDCT_SUCCESS",
    1: "HPDCT_ERROR_INVALID_VALUE",
    2: "HPDCT_ERROR_UNSUPPORTED",
    3: "HPDCT_ERROR_RANGE",
    4: "HPDCT_ERROR_DEVICE",
}

# every symbol include/hpdct.h, hpdct_baseline.h (A/B and measurement only)
# and hpdct_compat.h declare
C_SYMBOLS = [
    "hpdct_version", "hpdct_build_info", "hpdct_status_string", "hpdct_last_error_string",
    "hpdct_default_quant_table", "hpdct_default_transform", "hpdct_dct_transform",
    "hpdct_set_quant_table", "hpdct_get_quant_table",
    "hpdct_forward", "hpdct_inverse",
    "hpdct_forward_u8_f32", "hpdct_forward_u8_i8", "hpdct_inverse_f32_f32",
    "hpdct_fill_hash_u8", "hpdct_fill_rand_u8", "hpdct_u8_to_f32", "hpdct_f32_to_u8",
    "hpdct_baseline_forward", "hpdct_stream_forward", "hpdct_set_mapping", "hpdct_get_mapping",
    "hpdct_roundtrip_u8", "hpdct_roundtrip_u8_accumulate", "hpdct_forward_frames",
    "hpdct_stream_create", "hpdct_stream_run", "hpdct_stream_destroy", "hpdct_decode_i8_f32",
    "hpdct_roundtrip_release_sums", "hpdct_floor_probe", "hpdct_copy_ceiling",
    "hpdct_forward_blocks", "hpdct_inverse_blocks", "hpdct_zigzag_order",
    "hpdct_default_chroma_quant_table", "hpdct_forward_rgb_blocks", "hpdct_inverse_rgb_blocks",
    "hpdct_rgb_frame_geometry", "hpdct_forward_rgb_frame", "hpdct_inverse_rgb_frame",
    "hpdct_grey_frame_geometry", "hpdct_forward_grey_frame", "hpdct_inverse_grey_frame",
    "hpdct_encode_scan", "hpdct_scan_bound", "hpdct_scan_workspace_bytes", "hpdct_jpeg_header",
    "hpdct_huffman_table",
    "hpdct_decode_scan", "hpdct_decode_workspace_bytes", "hpdct_jpeg_parse",
    "hpdct_decode_scan_split", "hpdct_decode_split_workspace_bytes", "hpdct_decode_split_geometry",
    "hpdct_huffman_blob_bytes", "hpdct_huffman_prepare", "hpdct_huffman_optimal", "hpdct_scan_histogram",
    "hpdct_scan_bound_tables", "hpdct_encode_scan_tables", "hpdct_decode_scan_tables",
    "hpdct_decode_scan_split_tables",
    "hpdct_jpeg_header_tables", "hpdct_jpeg_parse_tables",
]
MAPPINGS = {"auto": 0, "tile": 1, "octet": 2, "duo": 3}
BASELINES = {"reference_3pass": 0, "fastappr_3pass": 1}
COMPAT_SYMBOLS = {
    "dct_all_blocks_cuda": "_Z19dct_all_blocks_cudaPfiiPKfS_",
    "idct_all_blocks_cuda": "_Z20idct_all_blocks_cudaPKfiiS0_Pf",
    # cublasDCTv2 surface (main_cublass_2.cu:36-37); last argument: cublasHandle_t (ignored)
    "dct_all_blocks": "_Z14dct_all_blocksPfiiPKfS_P13cublasContext",
    "idct_all_blocks": "_Z15idct_all_blocksPfiiPKfS_P13cublasContext",
}


class HpdctLibraryError(RuntimeError):
    """libhpdct.so is missing or failed to load (no fallback exists)."""


class HpdctError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS.get(status, status)}: {message}")
        self.status = status


_lib = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load (once) and return the native library; raise loudly if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    # libhpdct.so and torch both need libamdhip64.so.7 and the first one loaded
    # wins the soname for the whole process.  Two HIP runtimes (torch's bundled
    # copy and /opt/rocm's) in one process see no device, so let torch load
    # its runtime first and bind the library to that same instance.
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover - host-only use without torch
        pass
    if not os.path.exists(p):
        raise HpdctLibraryError(
            f"{p} not found: build it with `make -C cuda-dct-idct_amd` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    try:
        lib = ctypes.CDLL(p)
    except OSError as e:  # pragma: no cover - depends on the loader
        raise HpdctLibraryError(f"cannot load {p}: {e}") from e
    vp, i64, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32
    lib.hpdct_version.restype = ctypes.c_char_p
    lib.hpdct_build_info.restype = ctypes.c_char_p
    lib.hpdct_decode_i8_f32.argtypes = [vp, vp, i64, vp]
    lib.hpdct_decode_i8_f32.restype = ctypes.c_int
    lib.hpdct_floor_probe.argtypes = [ctypes.c_int, vp, vp, i64, i64, vp]
    lib.hpdct_floor_probe.restype = ctypes.c_int
    lib.hpdct_copy_ceiling.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, i64, ctypes.c_int, vp]
    lib.hpdct_copy_ceiling.restype = ctypes.c_int
    lib.hpdct_roundtrip_release_sums.argtypes = [vp]
    lib.hpdct_roundtrip_release_sums.restype = ctypes.c_int
    lib.hpdct_forward_blocks.argtypes = [vp, vp, i64, i64, ctypes.c_uint, vp]
    lib.hpdct_forward_blocks.restype = ctypes.c_int
    lib.hpdct_inverse_blocks.argtypes = [vp, vp, ctypes.c_int, i64, i64, ctypes.c_uint, vp]
    lib.hpdct_inverse_blocks.restype = ctypes.c_int
    lib.hpdct_zigzag_order.argtypes = [vp]
    lib.hpdct_zigzag_order.restype = None
    lib.hpdct_default_chroma_quant_table.argtypes = [vp]
    lib.hpdct_default_chroma_quant_table.restype = None
    for f in (lib.hpdct_forward_rgb_blocks, lib.hpdct_inverse_rgb_blocks):
        f.argtypes = [vp, vp, vp, vp, i64, i64, ctypes.c_int, vp, vp, ctypes.c_uint, vp]
        f.restype = ctypes.c_int
    lib.hpdct_rgb_frame_geometry.argtypes = [i64, i64, ctypes.c_int, vp, vp, vp, vp]
    lib.hpdct_rgb_frame_geometry.restype = ctypes.c_int
    lib.hpdct_forward_rgb_frame.argtypes = [vp, i64, vp, vp, vp, i64, i64, ctypes.c_int, vp, vp, ctypes.c_uint, vp]
    lib.hpdct_forward_rgb_frame.restype = ctypes.c_int
    lib.hpdct_inverse_rgb_frame.argtypes = [vp, vp, vp, vp, i64, i64, i64, ctypes.c_int, vp, vp, ctypes.c_uint, vp]
    lib.hpdct_inverse_rgb_frame.restype = ctypes.c_int
    lib.hpdct_grey_frame_geometry.argtypes = [i64, i64, vp, vp, vp]
    lib.hpdct_grey_frame_geometry.restype = ctypes.c_int
    lib.hpdct_forward_grey_frame.argtypes = [vp, i64, vp, i64, i64, vp, ctypes.c_uint, vp]
    lib.hpdct_forward_grey_frame.restype = ctypes.c_int
    lib.hpdct_inverse_grey_frame.argtypes = [vp, vp, i64, i64, i64, vp, ctypes.c_uint, vp]
    lib.hpdct_inverse_grey_frame.restype = ctypes.c_int
    lib.hpdct_encode_scan.argtypes = [vp, vp, vp, i64, i64, ctypes.c_int, i64, ctypes.c_uint, vp, i64, vp, vp, vp, i64,
                                      vp]
    lib.hpdct_encode_scan.restype = ctypes.c_int
    lib.hpdct_scan_bound.argtypes = [i64, i64]
    lib.hpdct_scan_bound.restype = i64
    lib.hpdct_scan_workspace_bytes.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int, i64]
    lib.hpdct_scan_workspace_bytes.restype = i64
    lib.hpdct_jpeg_header.argtypes = [vp, i64, vp, i64, i64, ctypes.c_int, ctypes.c_int, vp, vp, i64]
    lib.hpdct_jpeg_header.restype = ctypes.c_int
    lib.hpdct_huffman_table.argtypes = [ctypes.c_int, vp, vp, vp]
    lib.hpdct_huffman_table.restype = None
    lib.hpdct_decode_scan.argtypes = [vp, i64, vp, vp, vp, vp, i64, i64, ctypes.c_int, i64, ctypes.c_uint, vp, vp, vp,
                                      i64, vp]
    lib.hpdct_decode_scan.restype = ctypes.c_int
    lib.hpdct_decode_workspace_bytes.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int, i64, i64]
    lib.hpdct_decode_workspace_bytes.restype = i64
    lib.hpdct_decode_scan_split.argtypes = [vp, i64, vp, vp, vp, vp, i64, i64, ctypes.c_int, i64, ctypes.c_uint, i64,
                                            vp, vp, vp, i64, vp]
    lib.hpdct_decode_scan_split.restype = ctypes.c_int
    lib.hpdct_decode_split_workspace_bytes.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int, i64, i64]
    lib.hpdct_decode_split_workspace_bytes.restype = i64
    lib.hpdct_decode_split_geometry.argtypes = [ctypes.POINTER(ctypes.c_int)] * 3
    lib.hpdct_decode_split_geometry.restype = None
    lib.hpdct_jpeg_parse.argtypes = [vp, i64, vp]
    lib.hpdct_jpeg_parse.restype = ctypes.c_int
    lib.hpdct_huffman_blob_bytes.argtypes = []
    lib.hpdct_huffman_blob_bytes.restype = i64
    lib.hpdct_huffman_prepare.argtypes = [vp, vp, i64]
    lib.hpdct_huffman_prepare.restype = ctypes.c_int
    lib.hpdct_huffman_optimal.argtypes = [vp, vp]
    lib.hpdct_huffman_optimal.restype = ctypes.c_int
    lib.hpdct_scan_histogram.argtypes = [vp, vp, vp, i64, i64, ctypes.c_int, i64, ctypes.c_uint, vp, vp]
    lib.hpdct_scan_histogram.restype = ctypes.c_int
    lib.hpdct_scan_bound_tables.argtypes = [i64, i64]
    lib.hpdct_scan_bound_tables.restype = i64
    lib.hpdct_encode_scan_tables.argtypes = lib.hpdct_encode_scan.argtypes[:-1] + [vp, vp]
    lib.hpdct_encode_scan_tables.restype = ctypes.c_int
    lib.hpdct_decode_scan_tables.argtypes = lib.hpdct_decode_scan.argtypes[:-1] + [vp, vp]
    lib.hpdct_decode_scan_tables.restype = ctypes.c_int
    lib.hpdct_decode_scan_split_tables.argtypes = lib.hpdct_decode_scan_split.argtypes[:-1] + [vp, vp]
    lib.hpdct_decode_scan_split_tables.restype = ctypes.c_int
    lib.hpdct_jpeg_header_tables.argtypes = lib.hpdct_jpeg_header.argtypes + [vp]
    lib.hpdct_jpeg_header_tables.restype = ctypes.c_int
    lib.hpdct_jpeg_parse_tables.argtypes = [vp, i64, vp, vp]
    lib.hpdct_jpeg_parse_tables.restype = ctypes.c_int
    lib.hpdct_status_string.restype = ctypes.c_char_p
    lib.hpdct_status_string.argtypes = [ctypes.c_int]
    lib.hpdct_last_error_string.restype = ctypes.c_char_p
    for f in (lib.hpdct_default_quant_table, lib.hpdct_default_transform, lib.hpdct_dct_transform):
        f.argtypes = [vp]
        f.restype = None
    lib.hpdct_set_quant_table.argtypes = [vp]
    lib.hpdct_get_quant_table.argtypes = [vp]
    for f in (lib.hpdct_forward, lib.hpdct_inverse):
        f.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, i64, i64, vp, ctypes.c_uint, vp]
        f.restype = ctypes.c_int
    for f in (lib.hpdct_forward_u8_f32, lib.hpdct_forward_u8_i8, lib.hpdct_inverse_f32_f32):
        f.argtypes = [vp, vp, i64, i64, vp]
        f.restype = ctypes.c_int
    lib.hpdct_fill_hash_u8.argtypes = [vp, i64, ctypes.c_uint64, i64, vp]
    lib.hpdct_fill_hash_u8.restype = ctypes.c_int
    lib.hpdct_fill_rand_u8.argtypes = [vp, i64, u32]
    lib.hpdct_fill_rand_u8.restype = None
    lib.hpdct_u8_to_f32.argtypes = [vp, vp, i64]
    lib.hpdct_u8_to_f32.restype = None
    lib.hpdct_f32_to_u8.argtypes = [vp, vp, i64]
    lib.hpdct_f32_to_u8.restype = None
    lib.hpdct_set_mapping.argtypes = [ctypes.c_int]
    lib.hpdct_set_mapping.restype = ctypes.c_int
    lib.hpdct_get_mapping.argtypes = []
    lib.hpdct_get_mapping.restype = ctypes.c_int
    lib.hpdct_stream_forward.argtypes = [vp, vp, i64, i64, i64, ctypes.c_int, ctypes.c_int, vp]
    lib.hpdct_stream_forward.restype = ctypes.c_int
    lib.hpdct_stream_create.argtypes = [vp, i64, i64, ctypes.c_int, ctypes.c_int]
    lib.hpdct_stream_run.argtypes = [vp, vp, vp, i64, vp]
    lib.hpdct_stream_destroy.argtypes = [vp]
    for f in (lib.hpdct_stream_create, lib.hpdct_stream_run, lib.hpdct_stream_destroy):
        f.restype = ctypes.c_int
    lib.hpdct_forward_frames.argtypes = [vp, vp, ctypes.c_int, i64, i64, i64, vp]
    lib.hpdct_forward_frames.restype = ctypes.c_int
    lib.hpdct_baseline_forward.argtypes = [ctypes.c_int, vp, vp, vp, i64, i64, vp, vp]
    lib.hpdct_baseline_forward.restype = ctypes.c_int
    for f in (lib.hpdct_roundtrip_u8, lib.hpdct_roundtrip_u8_accumulate):
        f.argtypes = [vp, vp, vp, ctypes.c_int, vp, i64, i64, vp]
        f.restype = ctypes.c_int
    for name, mangled in COMPAT_SYMBOLS.items():
        f = getattr(lib, mangled)
        f.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp] + ([vp] if not name.endswith("_cuda") else [])
        f.restype = None
    if path is None:
        _lib = lib
    return lib


def _check(status: int) -> None:
    if status != 0:
        msg = load_library().hpdct_last_error_string().decode(errors="replace")
        raise HpdctError(status, msg)


def _bound(fn, args, keep=None):
    """The zero-argument callable every bind_*() returns: the per-call host cost
    is one ctypes call.  keep: host tables the library reads during the call,
    alive as call.tables for as long as the callable is."""
    def call():
        st = fn(*args)
        if st:
            _check(st)
    if keep is not None:
        call.tables = keep
    return call


def version() -> str:
    return load_library().hpdct_version().decode()


def build_info() -> str:
    """'src=<sha256 of csrc/ + include/> git=<rev> arch=gfx950' stamped at build
    time (src_digest.py)."""
    return load_library().hpdct_build_info().decode()


def provenance() -> dict:
    """The loaded library's build stamp and whether it matches the sources of
    this tree (bench.py / smoke() report it)."""
    import src_digest
    return src_digest.provenance(build_info())


def set_mapping(name: str) -> None:
    """Kernel work mapping, process-wide: "auto" (per frame size), "tile"
    (one lane per 8x8 tile), "octet" (eight lanes per tile) or "duo" (two
    lanes per tile, fp32 -> fp32 kernels).  Results are bit-identical; for
    A/B timing and tests (include/hpdct.h)."""
    if name not in MAPPINGS:
        raise ValueError(f"mapping must be one of {sorted(MAPPINGS)}")
    _check(load_library().hpdct_set_mapping(MAPPINGS[name]))


def get_mapping() -> str:
    m = load_library().hpdct_get_mapping()
    return {v: k for k, v in MAPPINGS.items()}[m]


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
def default_quant_table() -> np.ndarray:
    q = np.empty(64, np.float32)
    load_library().hpdct_default_quant_table(q.ctypes.data)
    return q.reshape(8, 8)


def default_transform() -> np.ndarray:
    t = np.empty(64, np.float32)
    load_library().hpdct_default_transform(t.ctypes.data)
    return t.reshape(8, 8)


def dct_transform() -> np.ndarray:
    """The exact 8x8 DCT-II matrix that transform="dct" uses (hpdct_dct_transform):
    fp32(sqrt(1/8)) in row 0, fp32(0.5 * cos((2i+1) v pi / 16)) elsewhere."""
    t = np.empty(64, np.float32)
    load_library().hpdct_dct_transform(t.ctypes.data)
    return t.reshape(8, 8)


def set_quant_table(q) -> None:
    """Library-owned Q (replaces cudaMemcpyToSymbol(const_quant_matrix, ...)).
    ``None`` restores the default JPEG luminance table."""
    lib = load_library()
    if q is None:
        _check(lib.hpdct_set_quant_table(None))
        return
    a = np.ascontiguousarray(np.asarray(q, dtype=np.float32).reshape(64))
    _check(lib.hpdct_set_quant_table(a.ctypes.data))


def get_quant_table() -> np.ndarray:
    q = np.empty(64, np.float32)
    _check(load_library().hpdct_get_quant_table(q.ctypes.data))
    return q.reshape(8, 8)


# ---------------------------------------------------------------------------
# device entry points (torch tensors in HBM)
# ---------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _dtype_code(t) -> int:
    torch = _torch()
    m = {torch.uint8: U8, torch.int8: I8, torch.float32: F32}
    if t.dtype not in m:
        raise HpdctError(2, f"unsupported tensor dtype {t.dtype}")
    return m[t.dtype]


def _stream_ptr(stream):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _hw(t, height, width):
    if height is None or width is None:
        if t.dim() < 2:
            raise HpdctError(1, "pass height/width for a flat tensor")
        height = t.numel() // t.shape[-1] if t.shape[-1] else 0
        width = t.shape[-1]
    h, w = int(height), int(width)
    if h < 0 or w < 0:
        raise HpdctError(1, f"negative frame shape {h}x{w}")
    if h * w > t.numel():
        raise HpdctError(1, f"a {h}x{w} frame needs {h * w} elements, the source holds {t.numel()}")
    return h, w


def _unit_hw(h: int, w: int, side: int):
    if h <= 0 or w <= 0 or h % side or w % side:
        raise HpdctError(1, f"height and width must be positive multiples of {side} (got {h}x{w})")
    return h, w


def _blocks_hw(t, height, width, what: str = "blocks"):
    """height and width as given, or from a (H/8, W/8, 64) block tensor."""
    if height is None or width is None:
        if t.dim() != 3 or t.shape[-1] != 64:
            raise HpdctError(1, f"pass height and width for {what} that are not (H/8, W/8, 64)")
        height, width = 8 * t.shape[0], 8 * t.shape[1]
    return int(height), int(width)


def _disjoint(spans):
    """spans: (first byte, one past the last, name) of every buffer of a launch."""
    for i, (a0, a1, a) in enumerate(spans):
        for b0, b1, b in spans[i + 1:]:
            if a0 < b1 and b0 < a1:
                raise HpdctError(1, f"the {a} and {b} buffers overlap")


def _device_plane(t, what: str, device, need: int, dtypes=None):
    """The C-ABI cannot see buffer sizes: every device plane is checked here
    (CUDA, contiguous, on `device`, >= `need` elements, dtype allowed)."""
    if not hasattr(t, "is_cuda") or not t.is_cuda:
        raise HpdctError(1, f"{what} must be a CUDA tensor")
    if not t.is_contiguous():
        raise HpdctError(1, f"{what} must be contiguous")
    if device is not None and t.device != device:
        raise HpdctError(1, f"{what} is on {t.device}, the source on {device}")
    if t.numel() < need:
        raise HpdctError(1, f"{what} holds {t.numel()} elements, {need} needed")
    if dtypes is not None and t.dtype not in dtypes:
        raise HpdctError(2, f"{what} dtype {t.dtype} not in {list(dtypes)}")


def _transform_ptr(transform, device):
    """None (built-in T) or a contiguous 64-element float32 CUDA tensor."""
    if transform is None:
        return None
    torch = _torch()
    _device_plane(transform, "transform", device, 64, (torch.float32,))
    if transform.numel() != 64:
        raise HpdctError(1, f"transform must hold 64 floats, not {transform.numel()}")
    return ctypes.c_void_p(transform.data_ptr())


def _planes(src, dst, direction: str, height, width):
    """Shape and buffer checks of one forward/inverse launch; returns (h, w)."""
    torch = _torch()
    what = "image" if direction == "fwd" else "coefficients"
    ins = (torch.uint8, torch.float32) if direction == "fwd" else (torch.int8, torch.float32)
    outs = (torch.float32, torch.int8) if direction == "fwd" else (torch.float32, torch.uint8)
    _device_plane(src, what, None, 0, ins)
    h, w = _hw(src, height, width)
    _device_plane(dst, "out", src.device, h * w, outs)
    return h, w


def forward(image, out=None, *, out_dtype=None, transform=None, quantise=True, writeback_shift=False,
            level_shift=True, row_first=False, height=None, width=None, stream=None):
    """Fused forward pass on the GPU: round((T.(X-128).T^T)/Q) per 8x8 tile.

    image: CUDA tensor, uint8 or float32, (..., H, W) contiguous (a stack of
    frames is treated as one (F*H) x W image).  Returns the coefficient
    tensor (float32 by default, int8 on request) in the reference layout."""
    torch = _torch()
    _device_plane(image, "image", None, 0)
    if out is None:
        out = torch.empty(image.shape, dtype=out_dtype or torch.float32, device=image.device)
    bind("fwd", image, out, transform=transform, quantise=quantise, level_shift=level_shift,
         writeback_shift=writeback_shift, row_first=row_first, stream=stream, height=height, width=width)()
    return out


def inverse(coef, out=None, *, out_dtype=None, transform=None, dequantise=True, level_shift=True,
            row_first=False, writeback_dequant=False, height=None, width=None, stream=None):
    """Fused inverse pass: T^T.(q*Q).T + 128 per tile.  out float32 (no clamp,
    as the reference) or uint8 (clamp + truncate, convertToUnsignedChar)."""
    torch = _torch()
    _device_plane(coef, "coefficients", None, 0)
    if out is None:
        out = torch.empty(coef.shape, dtype=out_dtype or torch.float32, device=coef.device)
    bind("inv", coef, out, transform=transform, quantise=dequantise, level_shift=level_shift, row_first=row_first,
         writeback_dequant=writeback_dequant, stream=stream, height=height, width=width)()
    return out


def bind(direction: str, src, dst, *, transform=None, quantise=True, level_shift=True, writeback_shift=False,
         row_first=False, writeback_dequant=False, stream=None, height=None, width=None):
    """Pre-resolve every argument of one forward ("fwd") or inverse ("inv")
    launch and return a zero-argument callable: the per-call host cost is one
    ctypes call (used by bench.py's timed loop)."""
    if direction not in ("fwd", "inv"):
        raise ValueError('direction must be "fwd" or "inv"')
    h, w = _planes(src, dst, direction, height, width)
    lib = load_library()
    fn = {"fwd": lib.hpdct_forward, "inv": lib.hpdct_inverse}[direction]
    flags = (0 if quantise else FLAG_NO_QUANT) | (0 if level_shift else FLAG_NO_SHIFT) | \
        (FLAG_WRITEBACK_SHIFT if writeback_shift else 0) | (FLAG_ROW_FIRST if row_first else 0) | \
        (FLAG_WRITEBACK_DEQUANT if writeback_dequant else 0)
    tptr = _transform_ptr(transform, src.device)
    args = (ctypes.c_void_p(src.data_ptr()), _dtype_code(src), ctypes.c_void_p(dst.data_ptr()), _dtype_code(dst),
            h, w, tptr, flags, _stream_ptr(stream))
    return _bound(fn, args)


# ---------------------------------------------------------------------------
# JPEG-style int16 coefficient blocks (hpdct_forward_blocks / _inverse_blocks)
# ---------------------------------------------------------------------------
def zigzag_order() -> np.ndarray:
    """The JPEG zig-zag scan (hpdct_zigzag_order): element n is the row-major
    index 8*v + u of the n-th coefficient of a block."""
    z = np.empty(64, np.uint8)
    load_library().hpdct_zigzag_order(z.ctypes.data)
    return z


def _block_flags(order: str) -> int:
    if order not in BLOCK_ORDERS:
        raise ValueError(f"order must be one of {sorted(BLOCK_ORDERS)}")
    return BLOCK_ORDERS[order]


def _frame_flags(order: str, transform: str) -> int:
    """The flags of a frame call: the block order and the built-in matrix."""
    if not isinstance(transform, str) or transform not in FRAME_TRANSFORMS:
        raise ValueError(f"transform must be one of {sorted(FRAME_TRANSFORMS)} (got {transform!r})")
    return _block_flags(order) | FRAME_TRANSFORMS[transform]


def _block_planes(direction: str, src, dst, height, width):
    """Buffer checks of one block launch (the C-ABI sees raw pointers only);
    returns (image, blocks, h, w).  fwd: src the uint8 frame, dst the int16
    blocks; inv: src the blocks, dst the fp32 or uint8 pixels."""
    torch = _torch()
    if direction == "fwd":
        _device_plane(src, "image", None, 0, (torch.uint8,))
        h, w = _unit_hw(*_hw(src, height, width), 8)
        _device_plane(dst, "out", src.device, h * w, (torch.int16,))
        return src, dst, h, w
    _device_plane(src, "blocks", None, 0, (torch.int16,))
    h, w = _unit_hw(*_blocks_hw(src, height, width), 8)
    if src.numel() < h * w:
        raise HpdctError(1, f"blocks hold {src.numel()} elements, a {h}x{w} frame needs {h * w}")
    _device_plane(dst, "out", src.device, h * w, (torch.float32, torch.uint8))
    return dst, src, h, w


def forward_blocks(image, out=None, *, order: str = "zigzag", height=None, width=None, stream=None):
    """uint8 frame -> JPEG-style int16 blocks, shape (H/8, W/8, 64): block
    [by, bx] holds tile (by, bx)'s quantised coefficients in zig-zag (or
    "natural", row-major) order.  The values of forward() cast to int16.  A
    stack of frames is one (F*H) x W image: each frame's blocks stay together."""
    torch = _torch()
    flags = _block_flags(order)
    _device_plane(image, "image", None, 0, (torch.uint8,))
    h, w = _unit_hw(*_hw(image, height, width), 8)
    if out is None:
        out = torch.empty((h // 8, w // 8, 64), dtype=torch.int16, device=image.device)
    _block_planes("fwd", image, out, h, w)
    _check(load_library().hpdct_forward_blocks(ctypes.c_void_p(image.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                               h, w, flags, _stream_ptr(stream)))
    return out


def inverse_blocks(blocks, out=None, *, out_dtype=None, order: str = "zigzag", height=None, width=None,
                   stream=None):
    """int16 blocks -> pixels: float32 (R + 128, no clamp) or uint8 (clamp +
    truncate), as inverse() on the spatial plane of the same values.  height
    and width come from a (H/8, W/8, 64) tensor when not given."""
    torch = _torch()
    flags = _block_flags(order)
    _device_plane(blocks, "blocks", None, 0, (torch.int16,))
    if out is None:
        h, w = _unit_hw(*_blocks_hw(blocks, height, width), 8)
        out = torch.empty((h, w), dtype=out_dtype or torch.float32, device=blocks.device)
    _, _, h, w = _block_planes("inv", blocks, out, height, width)
    _check(load_library().hpdct_inverse_blocks(ctypes.c_void_p(blocks.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                               _dtype_code(out), h, w, flags, _stream_ptr(stream)))
    return out


def bind_blocks(direction: str, src, dst, *, order: str = "zigzag", height=None, width=None, stream=None):
    """Pre-resolved forward_blocks ("fwd": uint8 frame -> int16 blocks) or
    inverse_blocks ("inv": blocks -> fp32 / uint8 pixels) launch: a
    zero-argument callable like bind(), for timing."""
    if direction not in ("fwd", "inv"):
        raise ValueError('direction must be "fwd" or "inv"')
    flags = _block_flags(order)
    image, blocks, h, w = _block_planes(direction, src, dst, height, width)
    lib = load_library()
    ip, bp = ctypes.c_void_p(image.data_ptr()), ctypes.c_void_p(blocks.data_ptr())
    if direction == "fwd":
        fn, args = lib.hpdct_forward_blocks, (ip, bp, h, w, flags, _stream_ptr(stream))
    else:
        fn, args = lib.hpdct_inverse_blocks, (bp, ip, _dtype_code(image), h, w, flags, _stream_ptr(stream))
    return _bound(fn, args)


# ---------------------------------------------------------------------------
# Colour frames (hpdct_forward_rgb_blocks / hpdct_inverse_rgb_blocks)
# ---------------------------------------------------------------------------
SUBSAMPLINGS = {"444": 0, "420": 1}  # HPDCT_SUBSAMPLING_*


def default_chroma_quant_table() -> np.ndarray:
    """The JPEG Annex K chrominance table (hpdct_default_chroma_quant_table)."""
    q = np.empty(64, np.float32)
    load_library().hpdct_default_chroma_quant_table(q.ctypes.data)
    return q.reshape(8, 8)


def _subsampling(name) -> int:
    if name not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLINGS)}")
    return SUBSAMPLINGS[name]


def _host_table(q):
    """None, or the 64 floats of a per-call table as a contiguous host array
    (the library reads it during the call)."""
    if q is None:
        return None
    a = np.ascontiguousarray(np.asarray(q, dtype=np.float32).reshape(-1))
    if a.size != 64:
        raise HpdctError(1, f"a quant table holds 64 floats, not {a.size}")
    return a


def _rgb_hw(rgb, sub: int):
    """(h, w) of an (..., H, W, 3) uint8 frame or stack, checked against the subsampling."""
    if rgb.dim() < 3 or rgb.shape[-1] != 3:
        raise HpdctError(1, "the RGB frame must be shaped (H, W, 3)")
    w = int(rgb.shape[-2])
    h = rgb.numel() // (3 * w) if w else 0
    return _unit_hw(h, w, 16 if sub == 1 else 8)


def _rgb_planes(rgb, y, cb, cr, h: int, w: int, sub: int):
    """Buffer checks of one colour launch, those of _block_planes: device,
    dtype, contiguity, size and overlap of the RGB frame and the three block
    arrays (the C-ABI sees raw pointers only)."""
    torch = _torch()
    _device_plane(rgb, "rgb", None, 3 * h * w, (torch.uint8,))
    ch, cw = (h // 2, w // 2) if sub == 1 else (h, w)
    for t, what, need in ((y, "y blocks", h * w), (cb, "cb blocks", ch * cw), (cr, "cr blocks", ch * cw)):
        _device_plane(t, what, rgb.device, need, (torch.int16,))
    _disjoint([(t.data_ptr(), t.data_ptr() + n, what) for t, n, what in
               ((rgb, 3 * h * w, "rgb"), (y, 2 * h * w, "y"), (cb, 2 * ch * cw, "cb"), (cr, 2 * ch * cw, "cr"))])


def _rgb_block_shapes(h: int, w: int, sub: int):
    ch, cw = (h // 2, w // 2) if sub == 1 else (h, w)
    return (h // 8, w // 8, 64), (ch // 8, cw // 8, 64)


def _rgb_call(fn, ptrs, h, w, sub, ql, qc, flags, stream):
    args = tuple(ctypes.c_void_p(p) for p in ptrs) + (
        h, w, sub, None if ql is None else ql.ctypes.data, None if qc is None else qc.ctypes.data, flags,
        _stream_ptr(stream))
    return _bound(fn, args, keep=(ql, qc))


def forward_rgb_blocks(rgb, *, subsampling: str = "420", q_luma=None, q_chroma=None, order: str = "zigzag",
                       out=None, stream=None):
    """Interleaved uint8 RGB (H, W, 3) -> (y, cb, cr) int16 blocks in one launch:
    y (H/8, W/8, 64), cb and cr (Hc/8, Wc/8, 64) with Hc x Wc = H x W ("444")
    or H/2 x W/2 ("420").  q_luma None: the library table (set_quant_table);
    q_chroma None: default_chroma_quant_table().  out: (y, cb, cr) to fill."""
    torch = _torch()
    sub, flags = _subsampling(subsampling), _block_flags(order)
    _device_plane(rgb, "rgb", None, 0, (torch.uint8,))
    h, w = _rgb_hw(rgb, sub)
    if out is None:
        ys, cs = _rgb_block_shapes(h, w, sub)
        out = (torch.empty(ys, dtype=torch.int16, device=rgb.device),
               torch.empty(cs, dtype=torch.int16, device=rgb.device),
               torch.empty(cs, dtype=torch.int16, device=rgb.device))
    y, cb, cr = out
    _rgb_planes(rgb, y, cb, cr, h, w, sub)
    _rgb_call(load_library().hpdct_forward_rgb_blocks, (rgb.data_ptr(), y.data_ptr(), cb.data_ptr(), cr.data_ptr()),
              h, w, sub, _host_table(q_luma), _host_table(q_chroma), flags, stream)()
    return y, cb, cr


def _rgb_inverse_hw(y, sub: int, height, width):
    return _unit_hw(*_blocks_hw(y, height, width, "y blocks"), 16 if sub == 1 else 8)


def inverse_rgb_blocks(y, cb, cr, *, subsampling: str, q_luma=None, q_chroma=None, order: str = "zigzag",
                       out=None, height=None, width=None, stream=None):
    """(y, cb, cr) int16 blocks -> interleaved uint8 RGB (H, W, 3) in one launch;
    H and W come from a (H/8, W/8, 64) y tensor when not given."""
    torch = _torch()
    sub, flags = _subsampling(subsampling), _block_flags(order)
    _device_plane(y, "y blocks", None, 0, (torch.int16,))
    h, w = _rgb_inverse_hw(y, sub, height, width)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=y.device)
    _device_plane(out, "rgb", y.device, 3 * h * w, (torch.uint8,))
    _rgb_planes(out, y, cb, cr, h, w, sub)
    _rgb_call(load_library().hpdct_inverse_rgb_blocks, (y.data_ptr(), cb.data_ptr(), cr.data_ptr(), out.data_ptr()),
              h, w, sub, _host_table(q_luma), _host_table(q_chroma), flags, stream)()
    return out


def bind_rgb_blocks(direction: str, rgb, y, cb, cr, *, subsampling: str = "420", q_luma=None, q_chroma=None,
                    order: str = "zigzag", stream=None):
    """Pre-resolved forward_rgb_blocks ("fwd") or inverse_rgb_blocks ("inv")
    launch on the given buffers: a zero-argument callable like bind_blocks(),
    for timing."""
    if direction not in ("fwd", "inv"):
        raise ValueError('direction must be "fwd" or "inv"')
    torch = _torch()
    sub, flags = _subsampling(subsampling), _block_flags(order)
    _device_plane(rgb, "rgb", None, 0, (torch.uint8,))
    h, w = _rgb_hw(rgb, sub)
    _rgb_planes(rgb, y, cb, cr, h, w, sub)
    lib = load_library()
    if direction == "fwd":
        fn, ptrs = lib.hpdct_forward_rgb_blocks, (rgb.data_ptr(), y.data_ptr(), cb.data_ptr(), cr.data_ptr())
    else:
        fn, ptrs = lib.hpdct_inverse_rgb_blocks, (y.data_ptr(), cb.data_ptr(), cr.data_ptr(), rgb.data_ptr())
    return _rgb_call(fn, ptrs, h, w, sub, _host_table(q_luma), _host_table(q_chroma), flags, stream)


# ---------------------------------------------------------------------------
# Colour frames of any size and row pitch (hpdct_forward_rgb_frame /
# hpdct_inverse_rgb_frame): edge-replicated to whole units, cropped on the way back
# ---------------------------------------------------------------------------
def rgb_frame_geometry(height: int, width: int, subsampling: str = "420"):
    """(padded_height, padded_width, y_blocks, chroma_blocks) of a height x width
    frame (hpdct_rgb_frame_geometry): the sizes rounded up to 8 ("444") or 16
    ("420") and the block counts of the three arrays."""
    out = [ctypes.c_int64() for _ in range(4)]
    _check(load_library().hpdct_rgb_frame_geometry(int(height), int(width), _subsampling(subsampling),
                                                   *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def _rgb_frame_view(rgb, what: str, device):
    """(h, w, pitch_bytes) of an (H, W, 3) uint8 device tensor whose pixels are
    dense (stride(2) == 1, stride(1) == 3) and whose rows lie stride(0) >= 3 W
    bytes apart: a whole frame, or a row- and column-sliced view of one."""
    torch = _torch()
    if not hasattr(rgb, "is_cuda") or not rgb.is_cuda:
        raise HpdctError(1, f"{what} must be a CUDA tensor")
    if device is not None and rgb.device != device:
        raise HpdctError(1, f"{what} is on {rgb.device}, the source on {device}")
    if rgb.dtype != torch.uint8:
        raise HpdctError(2, f"{what} dtype {rgb.dtype} not in {[torch.uint8]}")
    if rgb.dim() != 3 or rgb.shape[-1] != 3:
        raise HpdctError(1, f"the {what} frame must be shaped (H, W, 3)")
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    if h <= 0 or w <= 0:
        raise HpdctError(1, f"height and width must be positive (got {h}x{w})")
    s0, s1, s2 = (int(s) for s in rgb.stride())
    if s2 != 1 or (w > 1 and s1 != 3):
        raise HpdctError(1, f"{what} must hold interleaved pixels: stride(2) == 1 and stride(1) == 3 "
                            f"(got strides {(s0, s1, s2)})")
    if h == 1:
        s0 = 3 * w          # a single row: its stride is never used
    if s0 < 3 * w:
        raise HpdctError(1, f"{what} rows must lie at least 3*W = {3 * w} bytes apart (stride(0) is {s0})")
    return h, w, s0


def _rgb_frame_blocks(rgb, extent: int, y, cb, cr, geometry):
    """Buffer checks of the three block arrays of a frame launch, those of
    _rgb_planes against the padded geometry, and the overlap with the pitched
    RGB extent."""
    torch = _torch()
    _, _, yb, cbk = geometry
    for t, what, need in ((y, "y blocks", 64 * yb), (cb, "cb blocks", 64 * cbk), (cr, "cr blocks", 64 * cbk)):
        _device_plane(t, what, rgb.device, need, (torch.int16,))
    _disjoint([(t.data_ptr(), t.data_ptr() + n, what) for t, n, what in
               ((rgb, extent, "rgb"), (y, 128 * yb, "y"), (cb, 128 * cbk, "cb"), (cr, 128 * cbk, "cr"))])


def _rgb_frame_shapes(geometry, sub: int):
    hp, wp, _, _ = geometry
    ch, cw = (hp // 2, wp // 2) if sub == 1 else (hp, wp)
    return (hp // 8, wp // 8, 64), (ch // 8, cw // 8, 64)


def _rgb_frame_call(direction, rgb, pitch, y, cb, cr, h, w, sub, ql, qc, flags, stream):
    lib = load_library()
    vp = ctypes.c_void_p
    tail = (h, w, sub, None if ql is None else ql.ctypes.data, None if qc is None else qc.ctypes.data, flags,
            _stream_ptr(stream))
    if direction == "fwd":
        fn = lib.hpdct_forward_rgb_frame
        args = (vp(rgb.data_ptr()), pitch, vp(y.data_ptr()), vp(cb.data_ptr()), vp(cr.data_ptr())) + tail
    else:
        fn = lib.hpdct_inverse_rgb_frame
        args = (vp(y.data_ptr()), vp(cb.data_ptr()), vp(cr.data_ptr()), vp(rgb.data_ptr()), pitch) + tail
    return _bound(fn, args, keep=(ql, qc))


def forward_rgb_frame(rgb, *, subsampling: str = "420", q_luma=None, q_chroma=None, order: str = "zigzag",
                      out=None, stream=None, transform: str = "hpappr"):
    """forward_rgb_blocks for an (H, W, 3) uint8 frame of any size, row pitch
    and alignment (a row- or column-sliced view of a larger frame works without
    a copy): the frame is extended to whole units by repeating its last column
    and row, in the kernel.  Returns (y, cb, cr) shaped (Hp/8, Wp/8, 64) and
    (Hc/8, Wc/8, 64), Hp x Wp from rgb_frame_geometry, Hc x Wc = Hp x Wp
    ("444") or Hp/2 x Wp/2 ("420").  transform: "hpappr" (the reference's
    matrix) or "dct" (the exact DCT, HPDCT_FRAME_DCT: the blocks a standard JPEG
    decoder expects)."""
    torch = _torch()
    sub, flags = _subsampling(subsampling), _frame_flags(order, transform)
    h, w, pitch = _rgb_frame_view(rgb, "rgb", None)
    geometry = rgb_frame_geometry(h, w, subsampling)
    if out is None:
        ys, cs = _rgb_frame_shapes(geometry, sub)
        out = (torch.empty(ys, dtype=torch.int16, device=rgb.device),
               torch.empty(cs, dtype=torch.int16, device=rgb.device),
               torch.empty(cs, dtype=torch.int16, device=rgb.device))
    y, cb, cr = out
    _rgb_frame_blocks(rgb, (h - 1) * pitch + 3 * w, y, cb, cr, geometry)
    _rgb_frame_call("fwd", rgb, pitch, y, cb, cr, h, w, sub, _host_table(q_luma), _host_table(q_chroma), flags,
                    stream)()
    return y, cb, cr


def inverse_rgb_frame(y, cb, cr, *, height: int, width: int, subsampling: str, q_luma=None, q_chroma=None,
                      order: str = "zigzag", out=None, stream=None, transform: str = "hpappr"):
    """inverse_rgb_blocks cropped to height x width: (y, cb, cr) hold the blocks
    of the padded frame (rgb_frame_geometry), out is an (height, width, 3) uint8
    tensor or view (any row pitch; bytes between the rows are left alone).
    transform="dct": the exact inverse DCT with each component rounded (R +
    128.5, clamp, truncate) before the colour conversion (HPDCT_FRAME_DCT)."""
    torch = _torch()
    sub, flags = _subsampling(subsampling), _frame_flags(order, transform)
    _device_plane(y, "y blocks", None, 0, (torch.int16,))
    h, w = int(height), int(width)
    geometry = rgb_frame_geometry(h, w, subsampling)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=y.device)
    oh, ow, pitch = _rgb_frame_view(out, "rgb", y.device)
    if (oh, ow) != (h, w):
        raise HpdctError(1, f"rgb is {oh}x{ow}, the frame {h}x{w}")
    _rgb_frame_blocks(out, (h - 1) * pitch + 3 * w, y, cb, cr, geometry)
    _rgb_frame_call("inv", out, pitch, y, cb, cr, h, w, sub, _host_table(q_luma), _host_table(q_chroma), flags,
                    stream)()
    return out


def bind_rgb_frame(direction: str, rgb, y, cb, cr, *, subsampling: str = "420", q_luma=None, q_chroma=None,
                   order: str = "zigzag", stream=None, transform: str = "hpappr"):
    """Pre-resolved forward_rgb_frame ("fwd") or inverse_rgb_frame ("inv")
    launch on the given buffers (rgb: the frame or view, read or written): a
    zero-argument callable like bind_rgb_blocks(), for timing."""
    if direction not in ("fwd", "inv"):
        raise ValueError('direction must be "fwd" or "inv"')
    sub, flags = _subsampling(subsampling), _frame_flags(order, transform)
    h, w, pitch = _rgb_frame_view(rgb, "rgb", None)
    _rgb_frame_blocks(rgb, (h - 1) * pitch + 3 * w, y, cb, cr, rgb_frame_geometry(h, w, subsampling))
    return _rgb_frame_call(direction, rgb, pitch, y, cb, cr, h, w, sub, _host_table(q_luma), _host_table(q_chroma),
                           flags, stream)


# ---------------------------------------------------------------------------
# Grey frames of any size and row pitch (hpdct_forward_grey_frame /
# hpdct_inverse_grey_frame): edge-replicated to whole tiles, cropped on the way
# back, the quant table per call
# ---------------------------------------------------------------------------
def grey_frame_geometry(height: int, width: int):
    """(padded_height, padded_width, blocks) of a height x width grey frame
    (hpdct_grey_frame_geometry): the sizes rounded up to 8 and the block count."""
    out = [ctypes.c_int64() for _ in range(3)]
    _check(load_library().hpdct_grey_frame_geometry(int(height), int(width), *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def _grey_frame_view(image, what: str, device):
    """(h, w, pitch_bytes) of an (H, W) uint8 device tensor whose pixels are
    dense (stride(1) == 1) and whose rows lie stride(0) >= W bytes apart: a whole
    frame, or a row- and column-sliced view of one."""
    torch = _torch()
    if not hasattr(image, "is_cuda") or not image.is_cuda:
        raise HpdctError(1, f"{what} must be a CUDA tensor")
    if device is not None and image.device != device:
        raise HpdctError(1, f"{what} is on {image.device}, the source on {device}")
    if image.dtype != torch.uint8:
        raise HpdctError(2, f"{what} dtype {image.dtype} not in {[torch.uint8]}")
    if image.dim() != 2:
        raise HpdctError(1, f"the {what} frame must be shaped (H, W)")
    h, w = int(image.shape[0]), int(image.shape[1])
    if h <= 0 or w <= 0:
        raise HpdctError(1, f"height and width must be positive (got {h}x{w})")
    s0, s1 = (int(s) for s in image.stride())
    if w > 1 and s1 != 1:
        raise HpdctError(1, f"{what} must hold dense pixels: stride(1) == 1 (got strides {(s0, s1)})")
    if h == 1:
        s0 = w              # a single row: its stride is never used
    if s0 < w:
        raise HpdctError(1, f"{what} rows must lie at least W = {w} bytes apart (stride(0) is {s0})")
    return h, w, s0


def _grey_frame_blocks(image, extent: int, blocks, geometry):
    """Buffer checks of the block array of a grey frame launch against the
    padded geometry, and the overlap with the pitched image extent."""
    torch = _torch()
    _device_plane(blocks, "blocks", image.device, 64 * geometry[2], (torch.int16,))
    _disjoint([(image.data_ptr(), image.data_ptr() + extent, "image"),
               (blocks.data_ptr(), blocks.data_ptr() + 128 * geometry[2], "blocks")])


def _grey_frame_call(direction, image, pitch, blocks, h, w, q, flags, stream):
    lib = load_library()
    vp = ctypes.c_void_p
    tail = (h, w, None if q is None else q.ctypes.data, flags, _stream_ptr(stream))
    if direction == "fwd":
        fn, args = lib.hpdct_forward_grey_frame, (vp(image.data_ptr()), pitch, vp(blocks.data_ptr())) + tail
    else:
        fn, args = lib.hpdct_inverse_grey_frame, (vp(blocks.data_ptr()), vp(image.data_ptr()), pitch) + tail
    return _bound(fn, args, keep=(q,))


def forward_grey_frame(image, *, q=None, order: str = "zigzag", out=None, stream=None, transform: str = "hpappr"):
    """forward_blocks for an (H, W) uint8 frame of any size, row pitch and
    alignment (a row- or column-sliced view of a larger frame works without a
    copy), quantised with q (64 floats; None: the library table at the time of
    the call): the frame is extended to whole tiles by repeating its last column
    and row, in the kernel.  Returns int16 blocks shaped (Hp/8, Wp/8, 64), Hp x
    Wp from grey_frame_geometry.  transform: "hpappr" (the reference's matrix)
    or "dct" (the exact DCT, HPDCT_FRAME_DCT: the blocks a standard JPEG decoder
    expects)."""
    torch = _torch()
    flags = _frame_flags(order, transform)
    h, w, pitch = _grey_frame_view(image, "image", None)
    geometry = grey_frame_geometry(h, w)
    if out is None:
        out = torch.empty((geometry[0] // 8, geometry[1] // 8, 64), dtype=torch.int16, device=image.device)
    _grey_frame_blocks(image, (h - 1) * pitch + w, out, geometry)
    _grey_frame_call("fwd", image, pitch, out, h, w, _host_table(q), flags, stream)()
    return out


def inverse_grey_frame(blocks, *, height: int, width: int, q=None, order: str = "zigzag", out=None, stream=None,
                       transform: str = "hpappr"):
    """inverse_blocks to uint8, cropped to height x width and dequantised with q
    (None: the library table): blocks hold the padded frame (grey_frame_geometry),
    out is a (height, width) uint8 tensor or view (any row pitch; bytes between
    the rows are left alone).  transform="dct": the exact inverse DCT with the
    pixels rounded (R + 128.5, clamp, truncate), as JPEG decoders do
    (HPDCT_FRAME_DCT)."""
    torch = _torch()
    flags = _frame_flags(order, transform)
    _device_plane(blocks, "blocks", None, 0, (torch.int16,))
    h, w = int(height), int(width)
    geometry = grey_frame_geometry(h, w)
    if out is None:
        out = torch.empty((h, w), dtype=torch.uint8, device=blocks.device)
    oh, ow, pitch = _grey_frame_view(out, "image", blocks.device)
    if (oh, ow) != (h, w):
        raise HpdctError(1, f"image is {oh}x{ow}, the frame {h}x{w}")
    _grey_frame_blocks(out, (h - 1) * pitch + w, blocks, geometry)
    _grey_frame_call("inv", out, pitch, blocks, h, w, _host_table(q), flags, stream)()
    return out


def bind_grey_frame(direction: str, image, blocks, *, q=None, order: str = "zigzag", stream=None,
                    transform: str = "hpappr"):
    """Pre-resolved forward_grey_frame ("fwd") or inverse_grey_frame ("inv")
    launch on the given buffers (image: the frame or view, read or written): a
    zero-argument callable like bind_blocks().  It keeps the host table alive
    and allocates nothing: one kernel launch, which can be captured into a graph."""
    if direction not in ("fwd", "inv"):
        raise ValueError('direction must be "fwd" or "inv"')
    flags = _frame_flags(order, transform)
    h, w, pitch = _grey_frame_view(image, "image", None)
    _grey_frame_blocks(image, (h - 1) * pitch + w, blocks, grey_frame_geometry(h, w))
    return _grey_frame_call(direction, image, pitch, blocks, h, w, _host_table(q), flags, stream)


# ---------------------------------------------------------------------------
# Baseline-JPEG entropy coding (hpdct_encode_scan) and the file around the scan
# ---------------------------------------------------------------------------
HUFFMAN_TABLES = {"dc_luma": 0, "ac_luma": 1, "dc_chroma": 2, "ac_chroma": 3}


def _scan_bound(entry: str, blocks: int, intervals: int) -> int:
    n = int(getattr(load_library(), entry)(int(blocks), int(intervals)))
    if n < 0:
        raise HpdctError(1, f"no scan bound for {blocks} blocks in {intervals} intervals")
    return n


def scan_bound(blocks: int, intervals: int) -> int:
    """Worst-case bytes of a scan of `blocks` blocks in `intervals` restart
    intervals (hpdct_scan_bound): 415 * blocks + 4 * intervals."""
    return _scan_bound("hpdct_scan_bound", blocks, intervals)


def huffman_table(kind):
    """(bits, vals) of an Annex K.3 table (hpdct_huffman_table): kind 0..3 or
    "dc_luma", "ac_luma", "dc_chroma", "ac_chroma"; bits[l-1] codes of length
    l, vals the symbols in code order."""
    k = HUFFMAN_TABLES.get(kind, kind)
    if k not in (0, 1, 2, 3):
        raise ValueError(f"kind must be 0..3 or one of {sorted(HUFFMAN_TABLES)}")
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), ctypes.c_int(0)
    load_library().hpdct_huffman_table(k, bits.ctypes.data, vals.ctypes.data, ctypes.addressof(n))
    return bits, vals[:n.value].copy()


class _HuffmanSpec(ctypes.Structure):  # hpdct_huffman_spec
    _fields_ = [("bits", ctypes.c_uint8 * 16), ("vals", ctypes.c_uint8 * 256), ("nvals", ctypes.c_int32)]


def _huffman_specs(specs):
    """Four (bits, vals) pairs (None: an empty table) as hpdct_huffman_spec[4].  nvals is the length of vals:
    whether it is the sum of bits is the library's to judge."""
    if len(specs) != 4:
        raise HpdctError(1, f"four Huffman tables are expected (DC luma, AC luma, DC chroma, AC chroma; got {len(specs)})")
    arr = (_HuffmanSpec * 4)()
    for k, sp in enumerate(specs):
        if sp is None:
            continue
        bits, vals = (np.asarray(a, np.int64).ravel() for a in sp)
        if bits.size != 16 or vals.size > 256 or bits.min(initial=0) < 0 or bits.max(initial=0) > 255 or \
                vals.min(initial=0) < 0 or vals.max(initial=0) > 255:
            raise HpdctError(1, f"table {k}: bits is 16 bytes and vals at most 256 bytes")
        arr[k].bits[:] = [int(b) for b in bits]
        arr[k].vals[:vals.size] = [int(v) for v in vals]
        arr[k].nvals = int(vals.size)
    return arr


def _specs_out(arr):
    return [(np.array(a.bits, np.uint8), np.array(a.vals, np.uint8)[:max(0, min(256, a.nvals))].copy()) for a in arr]


def huffman_prepare(specs) -> np.ndarray:
    """The table blob of four Huffman tables (hpdct_huffman_prepare, host only):
    specs, four (bits, vals) pairs as huffman_table gives them, in the order DC
    luma, AC luma, DC chroma, AC chroma (None: an empty table).  Returns a uint8
    array of hpdct_huffman_blob_bytes() bytes; copy it to the device and pass
    that tensor as tables= to encode_scan / decode_scan.  A table a DHT segment
    may not hold is refused with status 1, the message naming table and reason."""
    lib = load_library()
    blob = np.zeros(int(lib.hpdct_huffman_blob_bytes()), np.uint8)
    arr = _huffman_specs(specs)
    _check(lib.hpdct_huffman_prepare(ctypes.addressof(arr), blob.ctypes.data, blob.size))
    return blob


def huffman_optimal(counts):
    """(bits, vals) of the optimal table of T.81 K.2 for 256 symbol counts
    (hpdct_huffman_optimal): no code longer than 16 bits, none all ones."""
    c = np.ascontiguousarray(np.asarray(counts).astype(np.uint64).ravel())
    if c.size != 256:
        raise HpdctError(1, f"256 counts are expected (got {c.size})")
    out = _HuffmanSpec()
    _check(load_library().hpdct_huffman_optimal(c.ctypes.data, ctypes.addressof(out)))
    return _specs_out([out])[0]


def scan_bound_tables(blocks: int, intervals: int) -> int:
    """scan_bound under a caller's tables (hpdct_scan_bound_tables): 417 * blocks + 4 * intervals."""
    return _scan_bound("hpdct_scan_bound_tables", blocks, intervals)


def _tables_ptr(tables, device):
    """The device pointer of a table blob (a uint8 tensor of huffman_prepare's bytes), or None."""
    if tables is None:
        return None
    torch = _torch()
    _device_plane(tables, "tables", device, int(load_library().hpdct_huffman_blob_bytes()), (torch.uint8,))
    return ctypes.c_void_p(tables.data_ptr())


def jpeg_header(height: int, width: int, *, components: int = 3, subsampling: str = "420", q_luma=None,
                q_chroma=None, restart_interval: int = 0, tables=None) -> bytes:
    """SOI .. SOS of a baseline file for a scan of encode_scan (hpdct_jpeg_header):
    height and width are the TRUE frame size; append the scan and FF D9.
    tables: the four (bits, vals) pairs DHT is to carry (huffman_prepare's
    specs; hpdct_jpeg_header_tables), None: Annex K's."""
    ql, qc = _host_table(q_luma), _host_table(q_chroma)
    buf, n = np.zeros(2048, np.uint8), ctypes.c_int64(0)
    args = (buf.ctypes.data, buf.size, ctypes.addressof(n), int(height), int(width), int(components),
            _subsampling(subsampling), None if ql is None else ql.ctypes.data,
            None if qc is None else qc.ctypes.data, int(restart_interval))
    arr = None if tables is None else _huffman_specs(tables)
    _check(load_library().hpdct_jpeg_header_tables(*args, None if arr is None else ctypes.addressof(arr)))
    return buf[:n.value].tobytes()


def _scan_planes(y, cb, cr, height, width, sub: int, restart_interval: int):
    """Buffer checks of the block arrays of one scan (the C-ABI sees raw pointers
    only); returns (h, w, components, blocks, intervals, workspace_bytes)."""
    torch = _torch()
    _device_plane(y, "y blocks", None, 0, (torch.int16,))
    if (cb is None) != (cr is None):
        raise HpdctError(1, "cb and cr are both given or both None")
    components = 1 if cb is None else 3
    side = 16 if components == 3 and sub == 1 else 8
    h, w = _unit_hw(*_blocks_hw(y, height, width, "y blocks"), side)
    ri = int(restart_interval)
    if not 0 <= ri <= 65535:
        raise HpdctError(1, f"restart_interval must be 0..65535 (got {ri})")
    _device_plane(y, "y blocks", None, h * w, (torch.int16,))
    nmcu = (h // side) * (w // side)
    blocks = h * w // 64
    if components == 3:
        for t, what in ((cb, "cb blocks"), (cr, "cr blocks")):
            _device_plane(t, what, y.device, 64 * nmcu, (torch.int16,))
        blocks += 2 * nmcu
    intervals = 1 if ri == 0 else -(-nmcu // ri)
    ws = int(load_library().hpdct_scan_workspace_bytes(h, w, components, sub, ri))
    if ws < 0:
        _check(1)
    return h, w, components, blocks, intervals, ws


def bind_scan(y, cb, cr, scan, info, offsets, workspace, *, height=None, width=None, subsampling: str = "420",
              restart_interval: int = 0, order: str = "zigzag", capacity=None, stream=None, tables=None):
    """Pre-resolved hpdct_encode_scan launch on the given buffers: a
    zero-argument callable like the other bind_* functions (three kernel
    launches, no allocation: it can be captured into a graph).  scan: uint8,
    `capacity` bytes of it (default: all) may be written; info: 16 bytes (two
    int64); offsets: None or intervals + 1 int64; workspace: uint8.  tables: a
    uint8 device tensor holding huffman_prepare's blob (hpdct_encode_scan_tables),
    None: Annex K's tables."""
    torch = _torch()
    sub, flags = _subsampling(subsampling), _block_flags(order)
    h, w, components, _, intervals, ws = _scan_planes(y, cb, cr, height, width, sub, restart_interval)
    _device_plane(scan, "scan", y.device, 0, (torch.uint8,))
    cap = scan.numel() if capacity is None else int(capacity)
    if cap < 0 or cap > scan.numel():
        raise HpdctError(1, f"capacity {cap} is not within the scan buffer's {scan.numel()} bytes")
    _device_plane(info, "info", y.device, 2, (torch.int64,))
    if offsets is not None:
        _device_plane(offsets, "offsets", y.device, intervals + 1, (torch.int64,))
    _device_plane(workspace, "workspace", y.device, ws, (torch.uint8,))
    vp = ctypes.c_void_p
    args = (vp(y.data_ptr()), None if cb is None else vp(cb.data_ptr()), None if cr is None else vp(cr.data_ptr()),
            h, w, sub, int(restart_interval), flags, vp(scan.data_ptr()), cap, vp(info.data_ptr()),
            None if offsets is None else vp(offsets.data_ptr()), vp(workspace.data_ptr()), workspace.numel())
    return _bound(load_library().hpdct_encode_scan_tables, args + (_tables_ptr(tables, y.device), _stream_ptr(stream)))


def bind_scan_histogram(y, cb, cr, counts, *, height=None, width=None, subsampling: str = "420",
                        restart_interval: int = 0, order: str = "zigzag", stream=None):
    """Pre-resolved hpdct_scan_histogram launch: a zero-argument callable (a
    memset and one kernel launch, no allocation: it can be captured into a
    graph).  counts: 4 * 256 int64 on the blocks' device, overwritten."""
    torch = _torch()
    sub, flags = _subsampling(subsampling), _block_flags(order)
    h, w, _, _, _, _ = _scan_planes(y, cb, cr, height, width, sub, restart_interval)
    _device_plane(counts, "counts", y.device, 1024, (torch.int64,))
    vp = ctypes.c_void_p
    args = (vp(y.data_ptr()), None if cb is None else vp(cb.data_ptr()), None if cr is None else vp(cr.data_ptr()),
            h, w, sub, int(restart_interval), flags, vp(counts.data_ptr()), _stream_ptr(stream))
    return _bound(load_library().hpdct_scan_histogram, args)


def scan_histogram(y, cb=None, cr=None, *, height=None, width=None, subsampling: str = "420",
                   restart_interval: int = 0, order: str = "zigzag", stream=None):
    """How often encode_scan emits each symbol of each table for these blocks
    (hpdct_scan_histogram): a (4, 256) int64 device tensor, rows DC luma, AC
    luma, DC chroma, AC chroma.  The arguments are encode_scan's."""
    torch = _torch()
    counts = torch.empty((4, 256), dtype=torch.int64, device=y.device)
    bind_scan_histogram(y, cb, cr, counts, height=height, width=width, subsampling=subsampling,
                        restart_interval=restart_interval, order=order, stream=stream)()
    return counts


def scan_info(info) -> dict:
    """The hpdct_scan_info a bind_scan launch wrote (synchronises)."""
    raw = info.cpu().numpy().view(np.uint32)
    return {"bytes": int(raw[0]) | int(raw[1]) << 32, "truncated": int(raw[2]), "out_of_range": int(raw[3])}


def encode_scan(y, cb=None, cr=None, *, height=None, width=None, subsampling: str = "420",
                restart_interval: int = 0, order: str = "zigzag", out=None, stream=None, tables=None):
    """int16 blocks -> the bytes of one baseline Huffman scan, on the device.
    tables: as bind_scan takes them (a symbol without a code is counted in
    info["out_of_range"]).
    y alone: grey; y, cb, cr: the arrays of forward_rgb_blocks / forward_rgb_frame
    (height and width: the padded frame).  Returns (scan, info, offsets): the
    uint8 device tensor trimmed to its length, {"bytes", "truncated",
    "out_of_range"} and the int64 device tensor of intervals + 1 byte offsets.
    Synchronises to read the length.  out: a uint8 buffer to fill; if the scan
    does not fit it, info["truncated"] is 1, info["bytes"] the size needed and
    the returned scan is empty.  Without out, a buffer of the blocks' own size
    is tried first and the exact size after that."""
    torch = _torch()
    sub = _subsampling(subsampling)
    _, _, _, blocks, intervals, ws = _scan_planes(y, cb, cr, height, width, sub, restart_interval)
    info = torch.empty(2, dtype=torch.int64, device=y.device)
    offsets = torch.empty(intervals + 1, dtype=torch.int64, device=y.device)
    workspace = torch.empty(ws, dtype=torch.uint8, device=y.device)
    bound = scan_bound(blocks, intervals) if tables is None else scan_bound_tables(blocks, intervals)
    buf = out if out is not None else torch.empty(min(bound, 128 * blocks + 4 * intervals),
                                                  dtype=torch.uint8, device=y.device)
    while True:
        bind_scan(y, cb, cr, buf, info, offsets, workspace, height=height, width=width, subsampling=subsampling,
                  restart_interval=restart_interval, order=order, stream=stream, tables=tables)()
        if stream is not None:
            stream.synchronize()
        res = scan_info(info)
        if not res["truncated"]:
            return buf[:res["bytes"]], res, offsets
        if out is not None:
            return buf[:0], res, offsets
        buf = torch.empty(res["bytes"], dtype=torch.uint8, device=y.device)


def jpeg_encode(image, *, subsampling: str = "420", q_luma=None, q_chroma=None, restart_interval=None,
                optimize: bool = False, transform: str = "hpappr") -> bytes:
    """A whole baseline JPEG file from a device frame.  A 2-D uint8 tensor of any
    size and row stride is a grey frame: forward_grey_frame under q_luma (None:
    the library table, set_quant_table), then encode_scan.  An (H, W, 3) tensor
    of any size goes through forward_rgb_frame with the given tables and
    subsampling.
    restart_interval None: one MCU row per interval, what the coder is tuned
    for.  transform: "hpappr", the reference's matrix: a standard decoder inverts
    with the exact DCT, so the file decodes there to an approximation of this
    library's own inverse; "dct": the exact DCT, the file a
    standard decoder expects, and jpeg_decode(..., transform="dct") is its
    rounding.  The entropy stage does not know the transform.
    optimize: the file carries the optimal Huffman tables of its own symbols
    instead of Annex K's (scan_histogram, 8 KiB to the host, huffman_optimal for
    each table in use, huffman_prepare, the blob to the device, then encode_scan
    and jpeg_header under those tables): a smaller file for one more read of the
    blocks and one round trip to the host."""
    _frame_flags("zigzag", transform)
    if image.dim() == 2:
        if q_chroma is not None:
            raise HpdctError(2, "a grey frame has no chroma table")
        h, w, _ = _grey_frame_view(image, "image", None)
        blocks = (forward_grey_frame(image, q=q_luma, transform=transform),)
        hp, wp, _ = grey_frame_geometry(h, w)
        components, mcu = 1, 8
    else:
        h, w, _ = _rgb_frame_view(image, "image", None)
        blocks = forward_rgb_frame(image, subsampling=subsampling, q_luma=q_luma, q_chroma=q_chroma,
                                   transform=transform)
        hp, wp, _, _ = rgb_frame_geometry(h, w, subsampling)
        components, mcu = 3, 16 if subsampling == "420" else 8
    ri = wp // mcu if restart_interval is None else int(restart_interval)
    specs = blob = None
    if optimize:
        counts = scan_histogram(*blocks, height=hp, width=wp, subsampling=subsampling, restart_interval=ri)
        counts = counts.cpu().numpy()
        specs = [huffman_optimal(counts[k]) if k < 2 or components == 3 else None for k in range(4)]
        blob = _torch().from_numpy(huffman_prepare(specs)).to(image.device)
    head = jpeg_header(h, w, components=components, subsampling=subsampling, q_luma=q_luma, q_chroma=q_chroma,
                       restart_interval=ri, tables=specs)
    scan, info, _ = encode_scan(*blocks, height=hp, width=wp, subsampling=subsampling, restart_interval=ri,
                                tables=blob)
    if info["out_of_range"]:
        raise HpdctError(3, f"{info['out_of_range']} coefficients are beyond baseline JPEG's range "
                            "(DC difference +-2047, AC +-1023): use a coarser quant table")
    return head + scan.cpu().numpy().tobytes() + b"\xff\xd9"


# ---------------------------------------------------------------------------
# Baseline-JPEG entropy decoding (hpdct_decode_scan) and the file's header
# ---------------------------------------------------------------------------
DECODE_STATUS = ["OK", "RANGE", "MARKER", "END", "CODE", "INDEX", "DC", "TAIL", "MISSING"]


class _JpegLayout(ctypes.Structure):  # hpdct_jpeg_layout
    _fields_ = [("height", ctypes.c_int64), ("width", ctypes.c_int64), ("components", ctypes.c_int),
                ("sub", ctypes.c_int), ("restart_interval", ctypes.c_int64), ("scan_offset", ctypes.c_int64),
                ("scan_bytes", ctypes.c_int64), ("q_luma", ctypes.c_float * 64), ("q_chroma", ctypes.c_float * 64)]


def _jpeg_parse(data, specs) -> dict:
    """jpeg_parse (specs None) and jpeg_parse_tables (specs: the hpdct_huffman_spec[4] to fill): the layout as a
    dictionary."""
    buf = np.frombuffer(bytes(data), np.uint8)
    lay = _JpegLayout()
    args = (buf.ctypes.data if buf.size else ctypes.addressof(lay), buf.size, ctypes.addressof(lay))
    if specs is None:
        _check(load_library().hpdct_jpeg_parse(*args))
    else:
        _check(load_library().hpdct_jpeg_parse_tables(*args, ctypes.addressof(specs)))
    names = {v: k for k, v in SUBSAMPLINGS.items()}
    return {"height": lay.height, "width": lay.width, "components": lay.components, "subsampling": names[lay.sub],
            "restart_interval": lay.restart_interval, "scan_offset": lay.scan_offset, "scan_bytes": lay.scan_bytes,
            "q_luma": np.array(lay.q_luma, np.float32).reshape(8, 8),
            "q_chroma": np.array(lay.q_chroma, np.float32).reshape(8, 8) if lay.components == 3 else None}


def jpeg_parse(data) -> dict:
    """SOI .. SOS of a baseline file (hpdct_jpeg_parse, host only): {"height",
    "width" (the TRUE frame size), "components", "subsampling", "restart_interval",
    "scan_offset", "scan_bytes", "q_luma", "q_chroma" (8x8 float32, row-major;
    q_chroma None for one component)}.  HpdctError status 2 names why a file is
    not one decode_scan decodes, status 1 a truncated or malformed file."""
    return _jpeg_parse(data, None)


def jpeg_parse_tables(data) -> dict:
    """jpeg_parse for a file with any Huffman tables a baseline DHT can carry
    (hpdct_jpeg_parse_tables): the same dictionary and "tables", the four
    (bits, vals) pairs the scan's components select (DC luma, AC luma, DC
    chroma, AC chroma; the chroma pair empty for one component), as
    huffman_prepare takes them."""
    arr = (_HuffmanSpec * 4)()
    return dict(_jpeg_parse(data, arr), tables=_specs_out(arr))


def _decode_geometry(height, width, components, sub: int, restart_interval):
    """(h, w, components, side, nmcu, intervals) of a scan of the padded frame h x w."""
    components, ri = int(components), int(restart_interval)
    if components not in (1, 3):
        raise HpdctError(1, "components must be 1 or 3")
    side = 16 if components == 3 and sub == 1 else 8
    h, w = _unit_hw(int(height), int(width), side)
    if not 0 <= ri <= 65535:
        raise HpdctError(1, f"restart_interval must be 0..65535 (got {ri})")
    nmcu = (h // side) * (w // side)
    return h, w, components, side, nmcu, 1 if ri == 0 else -(-nmcu // ri)


def decode_workspace_bytes(height, width, *, components=1, subsampling="420", restart_interval=0, scan_bytes=0) -> int:
    """hpdct_decode_workspace_bytes: 8 bytes per interval and per 4096 bytes of scan."""
    n = int(load_library().hpdct_decode_workspace_bytes(int(height), int(width), int(components),
                                                        _subsampling(subsampling), int(restart_interval),
                                                        int(scan_bytes)))
    if n < 0:
        _check(1)
    return n


def _bind_decode(split_min_bytes, scan, offsets, y, cb, cr, info, status, workspace, height, width, subsampling,
                 restart_interval, order, stream, tables=None):
    """bind_decode_scan (split_min_bytes None) and bind_decode_scan_split: the same buffers and checks, the info
    and the workspace the call's own."""
    torch = _torch()
    split = split_min_bytes is not None
    sub, flags = _subsampling(subsampling), _block_flags(order)
    _device_plane(y, "y blocks", None, 0, (torch.int16,))
    if (cb is None) != (cr is None):
        raise HpdctError(1, "cb and cr are both given or both None")
    h, w = _blocks_hw(y, height, width, "y blocks")
    h, w, components, side, nmcu, intervals = _decode_geometry(h, w, 1 if cb is None else 3, sub, restart_interval)
    if split and int(split_min_bytes) < 0:
        raise HpdctError(1, f"split_min_bytes must not be negative (got {split_min_bytes})")
    _device_plane(scan, "scan", y.device, 0, (torch.uint8,))
    _device_plane(y, "y blocks", None, h * w, (torch.int16,))
    if components == 3:
        for t, what in ((cb, "cb blocks"), (cr, "cr blocks")):
            _device_plane(t, what, y.device, 64 * nmcu, (torch.int16,))
    ninfo = 4 if split else 2
    _device_plane(info, "info", y.device, ninfo, (torch.int64,))
    if offsets is not None:
        _device_plane(offsets, "offsets", y.device, intervals + 1, (torch.int64,))
    if status is not None:
        _device_plane(status, "status", y.device, intervals, (torch.int64,))
    ws = (decode_split_workspace_bytes if split else decode_workspace_bytes)(
        h, w, components=components, subsampling=subsampling, restart_interval=restart_interval,
        scan_bytes=scan.numel())
    _device_plane(workspace, "workspace", y.device, ws, (torch.uint8,))
    spans = [(t.data_ptr(), t.data_ptr() + n * t.element_size(), what)
             for t, n, what in ((y, h * w, "y"), (cb, 64 * nmcu, "cb"), (cr, 64 * nmcu, "cr"), (scan, scan.numel(), "scan"),
                                (info, ninfo, "info"), (offsets, intervals + 1, "offsets"), (status, intervals, "status"),
                                (workspace, ws, "workspace")) if t is not None and n]
    _disjoint(spans)
    vp = ctypes.c_void_p
    args = (vp(scan.data_ptr()), scan.numel(), None if offsets is None else vp(offsets.data_ptr()), vp(y.data_ptr()),
            None if cb is None else vp(cb.data_ptr()), None if cr is None else vp(cr.data_ptr()), h, w, sub,
            int(restart_interval), flags) + ((int(split_min_bytes),) if split else ()) + (
            vp(info.data_ptr()), None if status is None else vp(status.data_ptr()),
            vp(workspace.data_ptr()), workspace.numel())
    lib = load_library()
    return _bound(lib.hpdct_decode_scan_split_tables if split else lib.hpdct_decode_scan_tables,
                  args + (_tables_ptr(tables, y.device), _stream_ptr(stream)))


def bind_decode_scan(scan, offsets, y, cb, cr, info, status, workspace, *, height=None, width=None,
                     subsampling: str = "420", restart_interval: int = 0, order: str = "zigzag", stream=None,
                     tables=None):
    """Pre-resolved hpdct_decode_scan launch on the given buffers (tables: a
    uint8 device tensor holding huffman_prepare's blob, hpdct_decode_scan_tables;
    None: Annex K's): a
    zero-argument callable like the other bind_* functions (two kernel launches
    with offsets, four without, no allocation: it can be captured into a graph).
    scan: uint8, all of it is the scan; offsets: None (the markers are located)
    or intervals + 1 int64; y, cb, cr: int16 block arrays to fill (cb = cr = None:
    grey); info: 16 bytes (two int64); status: None or `intervals` int64;
    workspace: uint8."""
    return _bind_decode(None, scan, offsets, y, cb, cr, info, status, workspace, height, width, subsampling,
                        restart_interval, order, stream, tables)


def decode_split_geometry():
    """hpdct_decode_split_geometry: (bytes of a segment, segments of a group, launches between groups)."""
    v = [ctypes.c_int(0) for _ in range(3)]
    load_library().hpdct_decode_split_geometry(*(ctypes.byref(x) for x in v))
    return tuple(int(x.value) for x in v)


def decode_split_workspace_bytes(height, width, *, components=1, subsampling="420", restart_interval=0,
                                 scan_bytes=0) -> int:
    """hpdct_decode_split_workspace_bytes: decode_workspace_bytes and 16 bytes per interval and group, 64 per
    segment more."""
    n = int(load_library().hpdct_decode_split_workspace_bytes(int(height), int(width), int(components),
                                                              _subsampling(subsampling), int(restart_interval),
                                                              int(scan_bytes)))
    if n < 0:
        _check(1)
    return n


def bind_decode_scan_split(scan, offsets, y, cb, cr, info, status, workspace, *, height=None, width=None,
                           subsampling: str = "420", restart_interval: int = 0, order: str = "zigzag",
                           split_min_bytes: int = 0, stream=None, tables=None):
    """Pre-resolved hpdct_decode_scan_split launch: bind_decode_scan's buffers,
    but info of 32 bytes (four int64) and a workspace of
    decode_split_workspace_bytes(...) bytes.  split_min_bytes: intervals of at
    least this many bytes are split (0: the library's choice; 1: all but empty
    ones).  Eleven launches with offsets, thirteen without, none of which waits
    for the host: it can be captured into a graph.  tables: as bind_decode_scan
    takes them (hpdct_decode_scan_split_tables)."""
    return _bind_decode(int(split_min_bytes), scan, offsets, y, cb, cr, info, status, workspace, height, width,
                        subsampling, restart_interval, order, stream, tables)


def decode_split_info(info) -> dict:
    """The hpdct_decode_split_info a bind_decode_scan_split launch wrote (synchronises)."""
    raw = info.cpu().numpy().view(np.uint32)
    return {"bad_intervals": int(raw[0]), "markers_found": int(raw[1]), "marker_errors": int(raw[2]),
            "split_intervals": int(raw[4]), "serial_intervals": int(raw[5]), "unsettled_intervals": int(raw[6]),
            "rounds": int(raw[7])}


def decode_info(info) -> dict:
    """The hpdct_decode_info a bind_decode_scan launch wrote (synchronises)."""
    raw = info.cpu().numpy().view(np.uint32)
    return {"bad_intervals": int(raw[0]), "markers_found": int(raw[1]), "marker_errors": int(raw[2])}


def decode_scan(scan, *, height, width, components: int = 1, subsampling: str = "420", restart_interval: int = 0,
                offsets=None, order: str = "zigzag", out=None, stream=None, method: str = "serial",
                split_min_bytes: int = 0, tables=None):
    """The bytes of one baseline Huffman scan -> int16 blocks, on the device: the
    inverse of encode_scan.  scan: a uint8 device tensor, all of it the scan;
    height and width: the padded frame; offsets: encode_scan's table, or None
    and the restart markers are located.  Returns (blocks, info, status): the
    tuple (y,) or (y, cb, cr) shaped like forward_blocks / forward_rgb_blocks
    give them (out: such a tuple to fill), {"bad_intervals", "markers_found",
    "marker_errors"} and the int64 device tensor of one status per interval
    (code + 256 * failing block; DECODE_STATUS names the codes; 0: clean).
    Untrusted bytes are safe to pass: a damaged interval is reported, its
    failing block and the blocks after it are zero.  method: "serial"
    (hpdct_decode_scan, one lane per restart interval) or "split"
    (hpdct_decode_scan_split, parallel inside an interval of at least
    split_min_bytes bytes as well: the same blocks and status, and info has the
    four counters of decode_split_info besides).  tables: a uint8 device tensor
    holding huffman_prepare's blob, the tables the scan was coded with (None:
    Annex K's).  Synchronises to read info."""
    torch = _torch()
    sub = _subsampling(subsampling)
    if method not in ("serial", "split"):
        raise ValueError(f"method must be 'serial' or 'split' (got {method!r})")
    split = method == "split"
    _device_plane(scan, "scan", None, 0, (torch.uint8,))
    h, w, components, side, nmcu, intervals = _decode_geometry(height, width, components, sub, restart_interval)
    dev = scan.device
    if out is None:
        out = (torch.empty((h // 8, w // 8, 64), dtype=torch.int16, device=dev),)
        if components == 3:
            out += tuple(torch.empty((h // side, w // side, 64), dtype=torch.int16, device=dev) for _ in range(2))
    if len(out) != components:
        raise HpdctError(1, f"out holds {len(out)} block arrays, the scan {components} components")
    y, cb, cr = (out[0], None, None) if components == 1 else out
    info = torch.empty(4 if split else 2, dtype=torch.int64, device=dev)
    status = torch.empty(intervals, dtype=torch.int64, device=dev)
    ws = (decode_split_workspace_bytes if split else decode_workspace_bytes)(
        h, w, components=components, subsampling=subsampling, restart_interval=restart_interval,
        scan_bytes=scan.numel())
    workspace = torch.empty(ws, dtype=torch.uint8, device=dev)
    _bind_decode(int(split_min_bytes) if split else None, scan, offsets, y, cb, cr, info, status, workspace, h, w,
                 subsampling, restart_interval, order, stream, tables)()
    if stream is not None:
        stream.synchronize()
    return tuple(out), (decode_split_info if split else decode_info)(info), status


SPLIT_MIN_BYTES = 3328  # hpdct_policy.hpp's kUnsplitMinBytes: what split_min_bytes = 0 and method="auto" mean


def jpeg_decode(data, *, device=None, method: str = "auto", quant: str = "library", transform: str = "hpappr"):
    """A baseline JPEG file (bytes) of the kind jpeg_encode writes -> pixels on
    the device: jpeg_parse on the host, the scan uploaded, decode_scan, then
    inverse_rgb_frame with the file's tables ((H, W, 3) uint8) or, for a grey
    file, inverse_blocks ((H, W) uint8, cut from the padded frame).  quant:
    "library": the grey inverse runs under the library table, and a grey file
    whose table differs from get_quant_table() is refused (set_quant_table
    first, or pass quant="file"); "file": a grey file is inverted with its own
    table through inverse_grey_frame, whatever the library table is (no global
    state is read or written).  A colour file is always inverted with its own
    tables.  A damaged scan
    (bad_intervals != 0) raises.  method: "serial" or "split" as decode_scan
    takes them, or "auto": the split call when the scan has SPLIT_MIN_BYTES
    bytes per restart interval or more (a file without restart markers is one
    interval), the serial call below that.  A file with Huffman tables of its
    own (jpeg_parse_tables; an optimised file) is decoded under them.
    transform: "hpappr", this library's own inverse (the reference's matrix,
    truncated pixels), or "dct": the exact inverse DCT with rounded pixels,
    what a standard decoder computes for the file.  Under
    "dct" a grey file always goes through inverse_grey_frame: with its own
    table (quant="file") or, once the equality rule above holds, with the
    library table (quant="library")."""
    torch = _torch()
    data = bytes(data)
    _frame_flags("zigzag", transform)
    if method not in ("auto", "serial", "split"):
        raise ValueError(f"method must be 'auto', 'serial' or 'split' (got {method!r})")
    if quant not in ("library", "file"):
        raise ValueError(f"quant must be 'library' or 'file' (got {quant!r})")
    lay = jpeg_parse_tables(data)
    dev = torch.device(device if device is not None else "cuda")
    annex = all(sp is None or (np.array_equal(sp[0], t[0]) and np.array_equal(sp[1], t[1]))
                for sp, t in zip([huffman_table(k) if k < 2 or lay["components"] == 3 else None for k in range(4)],
                                 lay["tables"]))
    tables = None if annex else torch.from_numpy(huffman_prepare(lay["tables"])).to(dev)
    h, w, comps, sub = lay["height"], lay["width"], lay["components"], lay["subsampling"]
    if comps == 1:
        if quant == "library" and not np.array_equal(lay["q_luma"], get_quant_table().reshape(8, 8)):
            raise HpdctError(2, "the grey file's quant table is not the library table: pass it to set_quant_table() "
                                "first (inverse_blocks dequantises with the library table), or pass quant=\"file\"")
        hp_, wp_, _ = grey_frame_geometry(h, w)
    else:
        hp_, wp_, _, _ = rgb_frame_geometry(h, w, sub)
    raw = np.frombuffer(data, np.uint8, lay["scan_bytes"], lay["scan_offset"])
    scan = torch.from_numpy(raw.copy()).to(dev)
    if method == "auto":
        intervals = _decode_geometry(hp_, wp_, comps, _subsampling(sub), lay["restart_interval"])[5]
        method = "split" if lay["scan_bytes"] >= SPLIT_MIN_BYTES * intervals else "serial"
    blocks, info, status = decode_scan(scan, height=hp_, width=wp_, components=comps, subsampling=sub,
                                       restart_interval=lay["restart_interval"], method=method, tables=tables)
    if info["bad_intervals"]:
        first = int(torch.nonzero(status)[0])
        code = int(status[first]) & 255
        raise HpdctError(1, f"{info['bad_intervals']} damaged restart intervals; the first is interval {first}: "
                            f"{DECODE_STATUS[code] if code < len(DECODE_STATUS) else code}")
    if comps == 1 and quant == "file":
        return inverse_grey_frame(blocks[0], height=h, width=w, q=lay["q_luma"], transform=transform)
    if comps == 1 and transform != "hpappr":
        return inverse_grey_frame(blocks[0], height=h, width=w, q=None, transform=transform)
    if comps == 1:
        return inverse_blocks(blocks[0], out_dtype=torch.uint8)[:h, :w]
    return inverse_rgb_frame(*blocks, height=h, width=w, subsampling=sub, q_luma=lay["q_luma"],
                             q_chroma=lay["q_chroma"], transform=transform)


SSE_F32_UNIT = 1.0 / 65536.0  # HPDCT_SSE_F32_UNIT
SSE_F32_INVALID = 1 << 63     # HPDCT_SSE_F32_INVALID


def _roundtrip_args(image, coef, recon, sums_buf, height, width, stream):
    torch = _torch()
    _device_plane(image, "image", None, 0, (torch.uint8,))
    h, w = _hw(image, height, width)
    _device_plane(coef, "coefficients", image.device, h * w, (torch.float32,))
    if recon is not None:
        _device_plane(recon, "reconstruction", image.device, h * w, (torch.uint8, torch.float32))
    if sums_buf is not None:
        _device_plane(sums_buf, "sums buffer", image.device, 3, (torch.int64,))
    return (ctypes.c_void_p(image.data_ptr()), ctypes.c_void_p(coef.data_ptr()),
            None if recon is None else ctypes.c_void_p(recon.data_ptr()),
            F32 if recon is None else _dtype_code(recon),
            None if sums_buf is None else ctypes.c_void_p(sums_buf.data_ptr()), h, w, _stream_ptr(stream))


def sums_from_buffer(sums_buf) -> dict:
    """The 3 x uint64 device struct hpdct_roundtrip_sums (held in an int64
    tensor) as {"sse_f32", "sse_u8", "sum_x2"} (synchronises)."""
    v = [int(x) & ((1 << 64) - 1) for x in sums_buf.cpu().tolist()]
    # bit 63: some tile's fp32 error sum was non-finite or too large to add
    # (HPDCT_SSE_F32_INVALID): no finite sse_f32 exists for the frame
    sse_f32 = float("inf") if v[0] & SSE_F32_INVALID else v[0] * SSE_F32_UNIT
    return {"sse_f32": sse_f32, "sse_u8": v[1], "sum_x2": v[2]}


def quality_from_sums(sums: dict, pixels: int) -> dict:
    """PEEN (%) and MSE of both reconstructions from the round-trip sums
    (PEEN = 100 sqrt(sse / sum x^2), MSE = sse / pixels; hpdct_quality.py)."""
    sx = float(sums["sum_x2"])
    return {"mse_f32": sums["sse_f32"] / pixels, "peen_f32_pct": 100.0 * (sums["sse_f32"] / sx) ** 0.5,
            "mse_u8": sums["sse_u8"] / pixels, "peen_u8_pct": 100.0 * (sums["sse_u8"] / sx) ** 0.5}


def roundtrip(image, coef=None, recon=None, *, recon_dtype=None, sums=False, height=None, width=None,
              stream=None):
    """One-pass C3 round trip on the GPU (hpdct_roundtrip_u8): uint8 frame ->
    fp32 quantised coefficients, the reconstruction (uint8 clamp + truncate or
    fp32, when recon or recon_dtype is given) and, with sums=True, the quality
    sums.  Bit-identical to forward() followed by inverse().
    Returns (coef, recon or None, sums dict or None); reading the sums
    synchronises the stream."""
    torch = _torch()
    if coef is None:
        coef = torch.empty(image.shape, dtype=torch.float32, device=image.device)
    if recon is None and recon_dtype is not None:
        recon = torch.empty(image.shape, dtype=recon_dtype, device=image.device)
    sums_buf = torch.empty(3, dtype=torch.int64, device=image.device) if sums else None
    _check(load_library().hpdct_roundtrip_u8(*_roundtrip_args(image, coef, recon, sums_buf, height, width, stream)))
    return coef, recon, (sums_from_buffer(sums_buf) if sums else None)


def bind_roundtrip(image, coef, recon=None, sums_buf=None, *, stream=None, height=None, width=None,
                   accumulate=False):
    """Pre-resolved round-trip launch (like bind): a zero-argument callable.
    sums_buf: an int64 CUDA tensor of 3 elements, or None.  accumulate=True:
    the frame's sums are added to sums_buf, which the caller zeroes
    (hpdct_roundtrip_u8_accumulate: the same kernels, the finish adds)."""
    if accumulate and sums_buf is None:
        raise HpdctError(1, "accumulate=True needs a sums buffer")
    args = _roundtrip_args(image, coef, recon, sums_buf, height, width, stream)
    lib = load_library()
    return _bound(lib.hpdct_roundtrip_u8_accumulate if accumulate else lib.hpdct_roundtrip_u8, args)


def baseline_forward(kind: str, image, tmp, result, transform, stream=None) -> None:
    """A/B baselines (include/hpdct_baseline.h): the reference's 3-launch
    HpApprDCT structure or the fastApprDCT row-per-thread structure on the GPU.
    Mutates `image` to X-128 like the reference."""
    if kind not in BASELINES:
        raise ValueError(f"kind must be one of {sorted(BASELINES)}")
    torch = _torch()
    _device_plane(image, "image", None, 0, (torch.float32,))
    h, w = _hw(image, None, None)
    for t, what in ((tmp, "tmp"), (result, "result")):
        _device_plane(t, what, image.device, h * w, (torch.float32,))
    if _transform_ptr(transform, image.device) is None:
        raise HpdctError(1, "the baselines take the caller's transform (64 floats on the device)")
    st = load_library().hpdct_baseline_forward(BASELINES[kind], ctypes.c_void_p(image.data_ptr()),
                                               ctypes.c_void_p(tmp.data_ptr()), ctypes.c_void_p(result.data_ptr()),
                                               h, w, ctypes.c_void_p(transform.data_ptr()), _stream_ptr(stream))
    if st:
        raise HpdctError(st, "baseline launch failed")


def _frame_list(frames, outs, out_dtype):
    """Checks of one frame list (the C-ABI sees only the pointer tables):
    every frame a contiguous uint8 CUDA tensor of one shape on one device,
    every out a contiguous plane of h*w elements of one coefficient dtype."""
    torch = _torch()
    frames = list(frames)
    if not frames:
        return frames, [], 0, 0
    _device_plane(frames[0], "frame 0", None, 0, (torch.uint8,))
    h, w = _hw(frames[0], None, None)
    shape, dev = tuple(frames[0].shape), frames[0].device
    for i, f in enumerate(frames):
        _device_plane(f, f"frame {i}", dev, h * w, (torch.uint8,))
        if tuple(f.shape) != shape:
            raise HpdctError(1, f"frame {i}: shape {tuple(f.shape)}, frame 0 is {shape}")
    if outs is None:
        outs = [torch.empty(shape, dtype=out_dtype or torch.float32, device=dev) for _ in frames]
    outs = list(outs)
    if len(outs) != len(frames):
        raise HpdctError(1, f"{len(frames)} frames but {len(outs)} coefficient planes")
    odt = outs[0].dtype
    for i, o in enumerate(outs):
        _device_plane(o, f"out {i}", dev, h * w, (torch.float32, torch.int8))
        if o.dtype != odt:
            raise HpdctError(1, f"out {i}: dtype {o.dtype}, out 0 is {odt}")
    return frames, outs, h, w


def forward_frames(frames, outs=None, *, out_dtype=None, stream=None):
    """A list of independent uint8 frames (CUDA tensors of one shape, need not
    be contiguous with each other) -> their quantised coefficients, one kernel
    launch per 64 frames (hpdct_forward_frames).  Built-in T, library Q.
    Bit-identical to forward() per frame; returns the list of outs."""
    frames, outs, h, w = _frame_list(frames, outs, out_dtype)
    n = len(frames)
    if n == 0:
        return outs
    fp = (ctypes.c_void_p * n)(*[f.data_ptr() for f in frames])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    _check(load_library().hpdct_forward_frames(fp, op, _dtype_code(outs[0]), n, h, w, _stream_ptr(stream)))
    return outs


def bind_frames(frames, outs, *, stream=None):
    """forward_frames with every argument resolved once: a zero-argument
    callable (bench.py's timed loop)."""
    frames, outs, h, w = _frame_list(frames, outs, None)
    n = len(frames)
    fp = (ctypes.c_void_p * n)(*[f.data_ptr() for f in frames])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    return _bound(load_library().hpdct_forward_frames, (fp, op, _dtype_code(outs[0]), n, h, w, _stream_ptr(stream)))


def _stream_lists(frames, outs):
    """Checks of a C5 batch; returns (n, h, w, out dtype code, frame and out pointer arrays)."""
    torch = _torch()
    n = len(frames)
    if n != len(outs) or n == 0:
        raise HpdctError(1, "frames and outs must be non-empty lists of equal length")
    h, w = _hw(frames[0], None, None)
    # the library copies h*w bytes in and h*w coefficients out per frame from
    # these host pointers: every entry must be exactly that large
    shape, odt = tuple(frames[0].shape), outs[0].dtype
    if odt not in (torch.float32, torch.int8):
        raise HpdctError(2, f"coefficient planes must be float32 or int8, not {odt}")
    for i, (f, o) in enumerate(zip(frames, outs)):
        if f.is_cuda or o.is_cuda:
            raise HpdctError(1, f"frame {i}: frames and outs are host (pinned) tensors")
        if not (f.is_contiguous() and o.is_contiguous()):
            raise HpdctError(1, f"frame {i}: host tensors must be contiguous")
        if f.dtype != torch.uint8 or tuple(f.shape) != shape:
            raise HpdctError(1, f"frame {i}: expected a uint8 {shape} frame, got {f.dtype} {tuple(f.shape)}")
        if o.dtype != odt or o.numel() != h * w:
            raise HpdctError(1, f"out {i}: expected {h * w} {odt} elements, got {o.numel()} {o.dtype}")
    fp = (ctypes.c_void_p * n)(*[f.data_ptr() for f in frames])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    return n, h, w, _dtype_code(outs[0]), fp, op


def stream_forward(frames, outs, nstreams: int = 3) -> float:
    """Config C5: host-resident (pinned) uint8 frames -> host coefficient planes
    with H2D / kernel / D2H overlapped over `nstreams` HIP streams.  `frames`
    and `outs` are equal-length lists of CPU tensors (entries may repeat).
    Returns the device-timed milliseconds of the whole batch.  One-shot:
    streams and device buffers are made and freed per call (StreamContext
    keeps them)."""
    n, h, w, odt, fp, op = _stream_lists(frames, outs)
    ms = ctypes.c_float()
    _check(load_library().hpdct_stream_forward(fp, op, n, h, w, odt, int(nstreams), ctypes.byref(ms)))
    return ms.value


class StreamContext:
    """A persistent C5 pipeline (hpdct_stream_create / _run / _destroy): the
    HIP streams, the device ring (one input + one output frame per stream)
    and the timing events are created once, on the current device, for
    height x width frames and one coefficient dtype; run() streams a batch
    through them like stream_forward()."""

    def __init__(self, height: int, width: int, out_dtype, nstreams: int = 3):
        torch = _torch()
        if out_dtype not in (torch.float32, torch.int8):
            raise HpdctError(2, f"coefficient planes must be float32 or int8, not {out_dtype}")
        self.height, self.width, self.out_dtype = int(height), int(width), out_dtype
        self.handle = ctypes.c_void_p()
        _check(load_library().hpdct_stream_create(ctypes.byref(self.handle), self.height, self.width,
                                                  F32 if out_dtype == torch.float32 else I8, int(nstreams)))

    def run(self, frames, outs) -> float:
        if not self.handle:
            raise HpdctError(1, "stream context is closed")
        n, h, w, _, fp, op = _stream_lists(frames, outs)
        if (h, w) != (self.height, self.width) or outs[0].dtype != self.out_dtype:
            raise HpdctError(1, f"context is for {self.height}x{self.width} -> {self.out_dtype} frames")
        ms = ctypes.c_float()
        _check(load_library().hpdct_stream_run(self.handle, fp, op, n, ctypes.byref(ms)))
        return ms.value

    def close(self) -> None:
        if self.handle:
            _check(load_library().hpdct_stream_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_hash_u8(out, seed: int, first_index: int = 0, stream=None):
    """Device-side synthetic frame: out[i] = splitmix64(seed, first_index+i) & 255."""
    _device_plane(out, "out", None, 0, (_torch().uint8,))
    _check(load_library().hpdct_fill_hash_u8(ctypes.c_void_p(out.data_ptr()), out.numel(),
                                             ctypes.c_uint64(seed), first_index, _stream_ptr(stream)))
    return out


def decode_i8_f32(q, out=None, stream=None):
    """int8 wire coefficients -> the fp32 coefficient plane (HIP kernel,
    hpdct_decode_i8_f32): equal in value to the fp32 forward's output."""
    torch = _torch()
    _device_plane(q, "q", None, 0, (torch.int8,))
    if out is None:
        out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    _device_plane(out, "out", q.device, q.numel(), (torch.float32,))
    _check(load_library().hpdct_decode_i8_f32(ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                              q.numel(), _stream_ptr(stream)))
    return out


PROBE_EMPTY, PROBE_COPY = 0, 1


def bind_floor_probe(kind: int, img=None, out=None, height: int = 0, width: int = 0, stream=None):
    """Measurement floor of the uint8 -> fp32 forward of a height x width
    frame (hpdct_floor_probe), as a zero-argument callable like bind():
    PROBE_EMPTY an empty kernel on that forward's grid, PROBE_COPY the same
    grid copying img (uint8) to out as fp32."""
    torch = _torch()
    ip = op = None
    if kind == PROBE_COPY:
        _device_plane(img, "img", None, int(height) * int(width), (torch.uint8,))
        _device_plane(out, "out", img.device, int(height) * int(width), (torch.float32,))
        ip, op = ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(out.data_ptr())
    return _bound(load_library().hpdct_floor_probe,
                  (int(kind), ip, op, int(height), int(width), _stream_ptr(stream)))


def floor_probe(kind: int, img=None, out=None, height: int = 0, width: int = 0, stream=None) -> None:
    bind_floor_probe(kind, img, out, height, width, stream)()


def bind_copy_ceiling(src, out0, out1=None, *, cap_waves: int = 0, stream=None):
    """The copy ceiling of a kernel that reads src and writes out0 (and out1)
    (hpdct_copy_ceiling, include/hpdct_baseline.h): the same bytes per pixel,
    no arithmetic, at most cap_waves resident one-wave workgroups per CU
    (0: no cap).  A zero-argument callable like bind().  Measurement only."""
    _device_plane(src, "src", None, 0)
    n = src.numel()
    for name, t in (("out0", out0), ("out1", out1)):
        if t is not None:
            _device_plane(t, name, src.device, n)
    args = (ctypes.c_void_p(src.data_ptr()), _dtype_code(src), ctypes.c_void_p(out0.data_ptr()), _dtype_code(out0),
            None if out1 is None else ctypes.c_void_p(out1.data_ptr()), F32 if out1 is None else _dtype_code(out1),
            n, int(cap_waves), _stream_ptr(stream))
    return _bound(load_library().hpdct_copy_ceiling, args)


def release_sums(sums_buf) -> None:
    """Return the library's 16 KiB spread slot kept for this sums buffer
    (hpdct_roundtrip_release_sums); call when no round trip with it is in
    flight (e.g. before freeing a ring of sums buffers)."""
    _device_plane(sums_buf, "sums_buf", None, 3, (_torch().int64,))
    _check(load_library().hpdct_roundtrip_release_sums(ctypes.c_void_p(sums_buf.data_ptr())))


# ---------------------------------------------------------------------------
# the reference's own C++ entry points (compat layer, synchronous, prints)
# ---------------------------------------------------------------------------
def _compat_call(key, image_matrix, img_height, img_width, transform_matrix, result, *extra):
    """Buffer checks the C++ entry points cannot make (they see raw pointers):
    fp32 CUDA planes of >= h*w elements and a 64-float device T.  Shape
    errors the reference itself reports (W, H not multiples of 8) are left to
    the library, which prints and exits like CHECK_CUDA."""
    torch = _torch()
    h, w = int(img_height), int(img_width)
    need = max(h, 0) * max(w, 0)
    _device_plane(image_matrix, "image_matrix", None, need, (torch.float32,))
    _device_plane(result, "result", image_matrix.device, need, (torch.float32,))
    tptr = _transform_ptr(transform_matrix, image_matrix.device)
    if tptr is None:
        raise HpdctError(1, "transform_matrix: the reference entry points take the caller's device T")
    f = getattr(load_library(), COMPAT_SYMBOLS[key])
    f(ctypes.c_void_p(image_matrix.data_ptr()), h, w, tptr, ctypes.c_void_p(result.data_ptr()), *extra)


def dct_all_blocks_cuda(image_matrix, img_height: int, img_width: int, transform_matrix, result) -> None:
    """main_newAppr.cu:252-291 semantics: device fp32 buffers, caller's T,
    X-128 left in image_matrix, timing line on stdout, exits on error."""
    _compat_call("dct_all_blocks_cuda", image_matrix, img_height, img_width, transform_matrix, result)


def idct_all_blocks_cuda(image_matrix, img_height: int, img_width: int, transform_matrix, result) -> None:
    """main_newAppr.cu:293-332 semantics."""
    _compat_call("idct_all_blocks_cuda", image_matrix, img_height, img_width, transform_matrix, result)


def dct_all_blocks(image_matrix, img_height: int, img_width: int, transform_matrix, result, handle=None) -> None:
    """cublasDCTv2 surface (main_cublass_2.cu:197-252): row pass first, X-128
    left in image_matrix; the cuBLAS handle is accepted and ignored."""
    _compat_call("dct_all_blocks", image_matrix, img_height, img_width, transform_matrix, result, handle)


def idct_all_blocks(image_matrix, img_height: int, img_width: int, transform_matrix, result, handle=None) -> None:
    """main_cublass_2.cu:257-311: q*Q left in image_matrix, D.T first."""
    _compat_call("idct_all_blocks", image_matrix, img_height, img_width, transform_matrix, result, handle)


# ---------------------------------------------------------------------------
# host helpers (no device work)
# ---------------------------------------------------------------------------
def fill_rand_u8(n: int, seed: int = 42) -> np.ndarray:
    """srand(seed); rand() % 256, n values (benchmark_newAppr.cu:46-51)."""
    a = np.empty(int(n), np.uint8)
    load_library().hpdct_fill_rand_u8(a.ctypes.data, int(n), ctypes.c_uint32(seed))
    return a


def convert_to_float(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    o = np.empty(a.shape, np.float32)
    load_library().hpdct_u8_to_f32(a.ctypes.data, o.ctypes.data, a.size)
    return o


def convert_to_unsigned_char(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    o = np.empty(a.shape, np.uint8)
    load_library().hpdct_f32_to_u8(a.ctypes.data, o.ctypes.data, a.size)
    return o


# ---------------------------------------------------------------------------
# row-shard layer over RCCL (include/hpdct_dist.h, lib/libhpdct_dist.so):
# BASELINE config C4.  The reference has no multi-GPU code.
# ---------------------------------------------------------------------------
DIST_LIB_PATH = os.environ.get("HPDCT_DIST_LIB", os.path.join(_HERE, "lib", "libhpdct_dist.so"))
DIST_SYMBOLS = [
    "hpdct_shard_rows", "hpdct_comm_init_all", "hpdct_comm_unique_id", "hpdct_comm_init_rank",
    "hpdct_comm_destroy", "hpdct_comm_rank", "hpdct_comm_size", "hpdct_comm_device",
    "hpdct_group_start", "hpdct_group_end", "hpdct_forward_slab", "hpdct_gather_rows", "hpdct_forward_sharded",
    "hpdct_gather_decode_i8",
]
UNIQUE_ID_BYTES = 128
_dist = None


def load_dist_library() -> ctypes.CDLL:
    """Load (once) libhpdct_dist.so; it needs librccl.so.1 (inside a torch
    process that is torch's own RCCL, already loaded under the same soname)."""
    global _dist
    if _dist is not None:
        return _dist
    load_library()
    if not os.path.exists(DIST_LIB_PATH):
        raise HpdctLibraryError(f"{DIST_LIB_PATH} not found: build it with `make -C cuda-dct-idct_amd`")
    try:
        lib = ctypes.CDLL(DIST_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the loader
        raise HpdctLibraryError(f"cannot load {DIST_LIB_PATH}: {e}") from e
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hpdct_shard_rows.argtypes = [i64, ci, ci, vp, vp]
    lib.hpdct_comm_init_all.argtypes = [vp, ci, vp]
    lib.hpdct_comm_unique_id.argtypes = [vp]
    lib.hpdct_comm_init_rank.argtypes = [vp, ci, vp, ci, ci]
    lib.hpdct_comm_destroy.argtypes = [vp]
    for f in (lib.hpdct_comm_rank, lib.hpdct_comm_size, lib.hpdct_comm_device):
        f.argtypes = [vp]
        f.restype = ci
    lib.hpdct_group_start.argtypes = []
    lib.hpdct_group_end.argtypes = []
    lib.hpdct_forward_slab.argtypes = [vp, vp, vp, ci, i64, i64, vp]
    lib.hpdct_gather_rows.argtypes = [vp, vp, vp, ci, i64, i64, ci, vp]
    lib.hpdct_forward_sharded.argtypes = [vp, vp, vp, ci, vp, i64, i64, ci, vp]
    lib.hpdct_gather_decode_i8.argtypes = [vp, vp, vp, vp, i64, i64, ci, vp]
    for name in DIST_SYMBOLS:
        if name not in ("hpdct_comm_rank", "hpdct_comm_size", "hpdct_comm_device"):
            getattr(lib, name).restype = ci
    _dist = lib
    return lib


def shard_rows_native(height: int, world: int, rank: int):
    """(first_row, rows) of `rank` from the C-ABI (hpdct_shard_rows)."""
    first, rows = ctypes.c_int64(), ctypes.c_int64()
    _check(load_dist_library().hpdct_shard_rows(int(height), int(world), int(rank), ctypes.byref(first),
                                                ctypes.byref(rows)))
    return first.value, rows.value


def comm_unique_id() -> bytes:
    """ncclGetUniqueId (rank 0 creates it, the caller hands it to every rank)."""
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    _check(load_dist_library().hpdct_comm_unique_id(buf))
    return buf.raw


class Comm:
    """An RCCL communicator of the row-shard layer (hpdct_comm)."""

    def __init__(self, handle: int):
        self.handle = ctypes.c_void_p(handle)

    @classmethod
    def init_all(cls, devices):
        """One communicator per device of this process (ncclCommInitAll)."""
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        hs = (ctypes.c_void_p * len(devices))()
        _check(load_dist_library().hpdct_comm_init_all(hs, len(devices), devs))
        return [cls(h) for h in hs]

    @classmethod
    def init_rank(cls, nranks: int, unique_id: bytes, rank: int, device: int):
        """One communicator per process (ncclCommInitRank on `device`)."""
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise HpdctError(1, f"unique id must be {UNIQUE_ID_BYTES} bytes")
        h = ctypes.c_void_p()
        uid = ctypes.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        _check(load_dist_library().hpdct_comm_init_rank(ctypes.byref(h), int(nranks), uid, int(rank), int(device)))
        return cls(h.value)

    @property
    def rank(self) -> int:
        return load_dist_library().hpdct_comm_rank(self.handle)

    @property
    def size(self) -> int:
        return load_dist_library().hpdct_comm_size(self.handle)

    @property
    def device(self) -> int:
        return load_dist_library().hpdct_comm_device(self.handle)

    def destroy(self) -> None:
        if self.handle:
            _check(load_dist_library().hpdct_comm_destroy(self.handle))
            self.handle = ctypes.c_void_p()


def group_start() -> None:
    _check(load_dist_library().hpdct_group_start())


def group_end() -> None:
    _check(load_dist_library().hpdct_group_end())


def forward_slab(comm: Comm, slab, coef_slab, height: int, width: int, stream=None) -> None:
    """The fused forward kernel on this rank's slab (hpdct_forward_slab):
    slab = rows x width uint8 of the height x width frame, rows from
    shard_rows_native(height, comm.size, comm.rank)."""
    torch = _torch()
    _, rows = shard_rows_native(height, comm.size, comm.rank)
    _device_plane(slab, "slab", None, rows * width, (torch.uint8,))
    _device_plane(coef_slab, "coefficient slab", slab.device, rows * width, (torch.float32, torch.int8))
    _check(load_dist_library().hpdct_forward_slab(comm.handle, ctypes.c_void_p(slab.data_ptr()),
                                                  ctypes.c_void_p(coef_slab.data_ptr()), _dtype_code(coef_slab),
                                                  int(height), int(width), _stream_ptr(stream)))


def gather_rows(comm: Comm, slab, frame, height: int, width: int, root: int = 0, stream=None) -> None:
    """Every rank's slab to the root's height x width `frame` over RCCL
    (hpdct_gather_rows); `frame` is ignored (may be None) off the root."""
    _, rows = shard_rows_native(height, comm.size, comm.rank)
    _device_plane(slab, "slab", None, rows * width)
    fp = None
    if comm.rank == root:
        _device_plane(frame, "frame", slab.device, int(height) * int(width), (slab.dtype,))
        fp = ctypes.c_void_p(frame.data_ptr())
    _check(load_dist_library().hpdct_gather_rows(comm.handle, ctypes.c_void_p(slab.data_ptr()), fp,
                                                 _dtype_code(slab), int(height), int(width), int(root),
                                                 _stream_ptr(stream)))


def gather_decode_i8(comm: Comm, slab8, frame8, frame, height: int, width: int, root: int = 0,
                     stream=None) -> None:
    """The int8 wire format's gather (hpdct_gather_decode_i8): every rank but
    the root sends its int8 slab; the root, whose own slab is already fp32 at
    its rows of `frame` (pass slab8=None there), receives the peers' slabs
    into the int8 scratch `frame8` and decodes them into `frame`.  frame8 and
    frame are ignored (may be None) off the root."""
    torch = _torch()
    n = int(height) * int(width)
    sp = f8 = ff = None
    if comm.rank != root:
        _, rows = shard_rows_native(height, comm.size, comm.rank)
        _device_plane(slab8, "slab", None, rows * int(width), (torch.int8,))
        sp = ctypes.c_void_p(slab8.data_ptr())
    else:
        _device_plane(frame8, "frame8", None, n, (torch.int8,))
        _device_plane(frame, "frame", frame8.device, n, (torch.float32,))
        f8, ff = ctypes.c_void_p(frame8.data_ptr()), ctypes.c_void_p(frame.data_ptr())
    _check(load_dist_library().hpdct_gather_decode_i8(comm.handle, sp, f8, ff, int(height), int(width), int(root),
                                                      _stream_ptr(stream)))
