/*
 * hpdct.h -- native C-ABI of the MI355X (gfx950) 8x8 block DCT/IDCT +
 * quantisation path (HpApprDCT arithmetic).  Library: libhpdct.so
 * (cuda-dct-idct_amd/lib/).
 *
 * Every entry point takes plain device pointers, 64-bit sizes and an optional
 * HIP stream (hipStream_t passed as void*; NULL = the null stream), returns a
 * status code and never exits the process.  The reference's own C++ entry
 * points (dct_all_blocks_cuda / idct_all_blocks_cuda, with their
 * print-and-exit semantics) are in hpdct_compat.h and are implemented on top
 * of these.
 *
 * Reference interface each function replaces (file:line into the reference,
 * GerryDps/CUDA-DCT-IDCT):
 *   hpdct_forward          dct_all_blocks_cuda      main_newAppr.cu:252-291
 *                          (sub_matrix_scalar -> cuda_matrix_dct ->
 *                          divide_matrices fused into one pass)
 *   hpdct_inverse          idct_all_blocks_cuda     main_newAppr.cu:293-332
 *                          (multiply_matrices -> cuda_matrix_idct ->
 *                          add_matrix_scalar fused into one pass)
 *   hpdct_roundtrip_u8     dct_all_blocks_cuda then idct_all_blocks_cuda
 *                          (main_newAppr.cu:99,120) and the host-side
 *                          PEEN/MSE of README.md:62-69, in one pass
 *   hpdct_forward(..., HPDCT_FLAG_ROW_FIRST)  dct_all_blocks  main_cublass_2.cu:197-252
 *   hpdct_inverse(..., HPDCT_FLAG_ROW_FIRST)  idct_all_blocks main_cublass_2.cu:257-311
 *   hpdct_set_quant_table  cudaMemcpyToSymbol(const_quant_matrix, ...)
 *                          main_newAppr.cu:19,70 (Q is library-owned here)
 *   hpdct_default_*        the Q and T tables of main_newAppr.cu:60-81
 *   hpdct_fill_rand_u8     not a device op in the reference: the synthetic
 *   (host)                 input of benchmark_newAppr.cu:46-51
 *                          (srand(42); rand()%256), restated
 *   hpdct_u8_from_f32 ... host conversions utils.cu:10-24
 *
 * Layout: an image is `height` rows of `width` elements, row-major, densely
 * packed (row pitch == width elements).  Coefficients are written in the
 * reference's spatial layout: coefficient (v,u) of tile (by,bx) sits at
 * [(8*by + v) * width + 8*bx + u].  A batch of F frames of HxW stacked in
 * memory is the single image (F*H) x W: tiles never cross a frame boundary
 * when H is a multiple of 8.  height and width must be positive multiples of
 * 8 (the reference silently produces garbage otherwise; we refuse).
 */
#ifndef HPDCT_H
#define HPDCT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum hpdct_status {
    HPDCT_SUCCESS = 0,
    HPDCT_ERROR_INVALID_VALUE = 1, /* NULL pointer, size not a positive multiple of 8, too many tiles */
    HPDCT_ERROR_UNSUPPORTED = 2,   /* dtype / flag combination not provided */
    HPDCT_ERROR_RANGE = 3,         /* int8 coefficients requested but the quant table can overflow int8 */
    HPDCT_ERROR_DEVICE = 4         /* a HIP runtime call failed: see hpdct_last_error_string() */
} hpdct_status;

typedef enum hpdct_dtype {
    HPDCT_U8 = 0,  /* uint8 pixels (0..255)                                   */
    HPDCT_I8 = 1,  /* int8 quantised coefficients (wire format, |q| <= 127)   */
    HPDCT_F32 = 2  /* fp32 pixels or coefficients (the reference's only type) */
} hpdct_dtype;

/* Flags for hpdct_forward / hpdct_inverse. */
#define HPDCT_FLAG_NO_QUANT 0x1u       /* forward: skip /Q+round; inverse: skip xQ (raw coefficients) */
#define HPDCT_FLAG_WRITEBACK_SHIFT 0x2u /* forward, f32 input only: also store X-128 back into the
                                           input buffer, as the reference's in-place sub_matrix_scalar
                                           does (main_newAppr.cu:273) */
#define HPDCT_FLAG_NO_SHIFT 0x4u       /* skip the -128 / +128 level shift (diagnostics, round trips) */
#define HPDCT_FLAG_ROW_FIRST 0x8u      /* fp32 -> fp32 only: cublasDCTv2 pass order (main_cublass_2.cu:228-235,
                                          288-295): the row pass X.T^T (D.T) before the column pass */
#define HPDCT_FLAG_WRITEBACK_DEQUANT 0x10u /* inverse, fp32 -> fp32 with dequantisation: also store q*Q back
                                              into the coefficient buffer, as the cublasDCTv2 inverse's in-place
                                              multiply_matrices does (main_cublass_2.cu:285) */

/* Library / error information. */
const char* hpdct_version(void);
/* Build provenance: "src=<sha256 of csrc/ + include/> git=<rev> arch=gfx950"
 * (cuda-dct-idct_amd/src_digest.py defines the digest; bench.py recomputes it
 * from the tree it runs in).  No reference counterpart. */
const char* hpdct_build_info(void);
const char* hpdct_status_string(hpdct_status status);
const char* hpdct_last_error_string(void); /* thread-local, last failing call */

/* Built-in tables (main_newAppr.cu:60-68 Q, :73-81 T), copied into caller memory. */
void hpdct_default_quant_table(float* q64);
void hpdct_default_transform(float* t64);
/* The exact 8x8 DCT-II matrix of HPDCT_FRAME_DCT, row-major [v][i]: the fp32
 * value nearest sqrt(1/8) for v == 0 and nearest 0.5 * cos((2i+1) v pi / 16)
 * otherwise, the formula evaluated in double.  No reference counterpart. */
void hpdct_dct_transform(float* t64);

/* Library-owned quantisation table used by every subsequent forward/inverse
 * call (process-wide).  q64: HOST pointer to 64 floats, row-major [v][u];
 * NULL restores the default JPEG luminance table.  Entries must be finite and
 * non-zero; negative entries are legal.
 * The inverses agree with the reference bit for bit under any such table,
 * also one so large that q*Q or a partial sum overflows (the reference then
 * gives Inf, and NaN where an Inf meets a zero entry of T).  The integer-input
 * inverses (HPDCT_I8 coefficients, int16 blocks, the colour calls; built-in T)
 * skip the zero entries of T only while that cannot happen:
 *     max|Q| * qmax * c^2 < FLT_MAX,
 * c = 2.378 the largest column abs-sum of T, qmax = 128 for HPDCT_I8 and 32768
 * for int16 blocks (max|Q| below 4.7e35 and 1.8e33; a colour call tests both
 * of its tables).  A table beyond that runs kernels that keep every term:
 * the same result by the same rule, at a lower speed. */
hpdct_status hpdct_set_quant_table(const float* q64);
hpdct_status hpdct_get_quant_table(float* q64);

/* Forward 8x8 block transform.
 *   d_image    : device, height*width elements of in_type (HPDCT_U8 or HPDCT_F32)
 *   d_coef     : device, height*width elements of out_type (HPDCT_F32, or
 *                HPDCT_I8 with quantisation on)
 *   d_transform: device pointer to 64 floats T[v][i], or NULL for the
 *                built-in HpApprDCT matrix
 *   flags      : HPDCT_FLAG_*
 *   stream     : hipStream_t or NULL
 * Computes, per tile, q = round((T . (X-128) . T^T) / Q) with the reference's
 * fp32 fused-multiply-add order and IEEE division.  Asynchronous w.r.t. the
 * host.  d_image and d_coef must not overlap (except that d_image is written
 * with X-128 under HPDCT_FLAG_WRITEBACK_SHIFT). */
hpdct_status hpdct_forward(const void* d_image, hpdct_dtype in_type, void* d_coef, hpdct_dtype out_type,
                           int64_t height, int64_t width, const float* d_transform, unsigned flags,
                           void* stream);

/* Inverse 8x8 block transform.
 *   d_coef : device, height*width elements of in_type (HPDCT_F32 or HPDCT_I8)
 *   d_image: device, height*width elements of out_type: HPDCT_F32 (R+128, no
 *            clamp, as the reference) or HPDCT_U8 (then clamped to [0,255] and
 *            truncated, as convertToUnsignedChar, utils.cu:18-24)
 * Computes R = T^T . (q*Q) . T + 128 per tile. */
hpdct_status hpdct_inverse(const void* d_coef, hpdct_dtype in_type, void* d_image, hpdct_dtype out_type,
                           int64_t height, int64_t width, const float* d_transform, unsigned flags,
                           void* stream);

/* Typed shorthands for the common cases (built-in T, library Q). */
hpdct_status hpdct_forward_u8_f32(const uint8_t* d_image, float* d_coef, int64_t height, int64_t width,
                                  void* stream);
hpdct_status hpdct_forward_u8_i8(const uint8_t* d_image, int8_t* d_coef, int64_t height, int64_t width,
                                 void* stream);
hpdct_status hpdct_inverse_f32_f32(const float* d_coef, float* d_image, int64_t height, int64_t width,
                                   void* stream);

/* One-pass round trip (BASELINE config C3: forward DCT + IDCT with the
 * PEEN/MSE check).  The reference runs dct_all_blocks_cuda then
 * idct_all_blocks_cuda (main_newAppr.cu:99,120; benchmark_newAppr.cu:93,105)
 * and measures quality on the host (README.md:62-69).  Here one kernel reads
 * the uint8 frame once and writes
 *   d_coef   fp32 quantised coefficients (required; as hpdct_forward U8 -> F32)
 *   d_recon  the reconstruction R+128 as recon_type HPDCT_U8 (clamp +
 *            truncate) or HPDCT_F32 (no clamp), or NULL for none (as
 *            hpdct_inverse F32 -> recon_type on d_coef)
 *   d_sums   device struct, or NULL: the quality sums below (overwritten).  The
 *            kernel adds into a 16 KiB library "spread slot" kept per d_sums
 *            pointer (64 sub-slots on separate 256-B lines, so the atomics of
 *            many waves do not queue on one line; allocated zeroed on first
 *            use, 256 = 4 MiB at a time) and a one-wave kernel then folds it
 *            into *d_sums and zeroes it: no memset before the kernel.  A slot
 *            stays with its pointer until hpdct_roundtrip_release_sums.
 *            Without a slot (an allocation would be needed inside a stream
 *            capture, or 4096 pointers = 64 MiB of slots are live on the
 *            device) the launch memsets *d_sums and takes the tile-per-lane
 *            kernel.  Two overwriting launches in flight at once with the
 *            same d_sums on different streams race, as they would on the
 *            struct itself (accumulating ones do not: see below).
 * Built-in T, the library Q, level shift 128; coefficients and reconstruction
 * are bit-identical to the two separate calls.  HBM traffic per pixel: 1 B
 * read, 4 B (+1 or 4 B) written, against 10 B for the two calls.
 * PEEN = 100 sqrt(sse / sum_x2) %, MSE = sse / (height*width) (the
 * definitions of the README table). */
typedef struct hpdct_roundtrip_sums {
    uint64_t sse_f32_fx; /* sum (x - (R+128))^2 in units of 2^-16 (HPDCT_SSE_F32_UNIT): per tile four
                            fp32 partial sums, one per (row parity, column parity) class of its
                            pixels (an fma chain over the class's 16 pixels in row-major order, so
                            NOT the exact sum: relative error ~1e-10 on a 8192^2 frame), each
                            rounded to the unit, then all added exactly in any order.  Bit 63
                            (HPDCT_SSE_F32_INVALID) is set, sticky, when some partial sum is
                            non-finite or >= 2^24 (an extreme caller table on the IEEE path): the
                            field then holds no sum */
    uint64_t sse_u8;     /* sum (x - u8(R+128))^2, exact */
    uint64_t sum_x2;     /* sum x^2, exact */
} hpdct_roundtrip_sums;
#define HPDCT_SSE_F32_UNIT (1.0 / 65536.0)
#define HPDCT_SSE_F32_INVALID (1ull << 63)
hpdct_status hpdct_roundtrip_u8(const uint8_t* d_image, float* d_coef, void* d_recon, hpdct_dtype recon_type,
                                hpdct_roundtrip_sums* d_sums, int64_t height, int64_t width, void* stream);

/* The same round trip, but the frame's quality sums are ADDED to *d_sums,
 * which the caller has zeroed (d_sums required; the same spread slot and fold
 * kernel, which adds instead of overwriting).  A pipeline that owns a ring of
 * per-frame sums slots zeroes the ring once, with one memset for many frames,
 * and gets the same per-frame sums (or a batch total, if frames share a
 * slot).  The fold takes the slot with atomic exchanges and adds with atomic
 * adds, so frames that share d_sums may run on different streams at once. */
hpdct_status hpdct_roundtrip_u8_accumulate(const uint8_t* d_image, float* d_coef, void* d_recon,
                                           hpdct_dtype recon_type, hpdct_roundtrip_sums* d_sums, int64_t height,
                                           int64_t width, void* stream);

/* Return the spread slot kept for d_sums (16 KiB of device memory) to the
 * library, e.g. before freeing a ring of per-frame sums structs.  Call it when
 * no round trip with d_sums is in flight and no captured HIP graph that uses
 * d_sums will be replayed (the slot may go to another pointer); a later round
 * trip with the same pointer takes a slot again.  A pointer without a slot (or
 * NULL) is a no-op.  No reference counterpart. */
hpdct_status hpdct_roundtrip_release_sums(const hpdct_roundtrip_sums* d_sums);

/* A list of independent device frames in as few launches as possible (config
 * C2's small frames: one 1024^2 frame per launch is dispatch-bound, ~3.6 us for
 * ~0.9 us of work).  d_images / d_coefs: HOST arrays of n_frames DEVICE
 * pointers; frame f is height x width uint8 at d_images[f] (8-byte aligned),
 * its coefficients go to d_coefs[f] as out_type HPDCT_F32 (16-byte aligned) or
 * HPDCT_I8 (8-byte aligned).  Frames need not be contiguous or distinct inputs
 * (a pool may repeat), but no coefficient plane may overlap another plane or
 * any input.  Built-in T, the library Q, level shift 128: the result is
 * bit-identical to n_frames calls of hpdct_forward.  One kernel launch per 64
 * frames (the pointer table travels in the kernel arguments); asynchronous on
 * `stream`; n_frames == 0 is a no-op.  The reference has no batch entry
 * (dct_all_blocks_cuda takes one image, main_newAppr.cu:252). */
hpdct_status hpdct_forward_frames(const uint8_t* const* d_images, void* const* d_coefs, hpdct_dtype out_type,
                                  int64_t n_frames, int64_t height, int64_t width, void* stream);

/* Host-resident batch (BASELINE config C5): frame f (height x width uint8 at
 * h_frames[f]) -> coefficients at h_coef[f] (out_type HPDCT_F32 or HPDCT_I8),
 * pipelined over nstreams (1..16) HIP streams, each with one device input and
 * one output buffer: H2D copy, fused forward kernel and D2H copy of different
 * frames overlap (2 streams keep both DMA directions busy: 0.90-0.97 of the
 * copy-only duplex ceiling on MI355X).  HPDCT_STREAM_PIPELINE=engines selects
 * a rejected A/B layout (one stream per engine over nstreams device slots).
 * Pointers may repeat (a pool cycled over the batch).  Host
 * buffers should be pinned for the copies to overlap.  Synchronous: returns
 * when every coefficient plane is in host memory; *elapsed_ms (may be NULL)
 * receives the device-timed span of the batch.  Replaces the reference's
 * one-image blocking H2D/compute/D2H sequence (benchmark_newAppr.cu:88-109). */
hpdct_status hpdct_stream_forward(const uint8_t* const* h_frames, void* const* h_coef, int64_t n_frames,
                                  int64_t height, int64_t width, hpdct_dtype out_type, int nstreams,
                                  float* elapsed_ms);

/* The same pipeline with its resources kept across calls: hpdct_stream_create
 * makes the nstreams HIP streams, their device input/output buffers (one
 * height x width frame each) and the timing events on the current device;
 * hpdct_stream_run streams one batch through them (semantics and timing as
 * hpdct_stream_forward, on the context's device); hpdct_stream_destroy frees
 * them.  hpdct_stream_forward is create + run + destroy.  A context is not
 * thread-safe: one run at a time. */
typedef struct hpdct_stream_ctx_s* hpdct_stream_ctx;
hpdct_status hpdct_stream_create(hpdct_stream_ctx* ctx, int64_t height, int64_t width, hpdct_dtype out_type,
                                 int nstreams);
hpdct_status hpdct_stream_run(hpdct_stream_ctx ctx, const uint8_t* const* h_frames, void* const* h_coef,
                              int64_t n_frames, float* elapsed_ms);
hpdct_status hpdct_stream_destroy(hpdct_stream_ctx ctx);

/* Synthetic frames generated on the device (BASELINE config C4): pixel
 * i of the frame = splitmix64(seed, first_index + i) & 255 (the oracle's
 * oracle_fill_hash_u8 restates it). */
hpdct_status hpdct_fill_hash_u8(uint8_t* d_out, int64_t n, uint64_t seed, int64_t first_index, void* stream);

/* Decode n int8 wire coefficients (hpdct_forward's HPDCT_I8 output, e.g. a
 * root's gathered C4 frame) into the fp32 coefficient plane
 * dct_all_blocks_cuda produces (main_newAppr.cu:252-291): out[i] = (float)q[i].
 * Equal in value to the fp32 forward's output; a -0.0 of that output decodes
 * as +0.0.  Device pointers: d_q 4-byte, d_out 16-byte aligned.  Async on
 * `stream`.  No reference counterpart (the reference has no int8 format). */
hpdct_status hpdct_decode_i8_f32(const int8_t* d_q, float* d_out, int64_t n, void* stream);

/* JPEG-style coefficient blocks (no reference counterpart: the reference keeps
 * its coefficients in the spatial layout).  What an entropy coder or libjpeg's
 * jpeg_write_coefficients takes: one block of 64 int16 per 8x8 tile, block
 * after block.
 *   layout  block t = tile t in row-major tile order, t = by * (width/8) + bx,
 *           at d_blocks + 64 * t; element n of a block = the quantised
 *           coefficient at row-major position zigzag[n] (hpdct_zigzag_order),
 *           or at n with HPDCT_BLOCKS_NATURAL (row-major (v,u): what libjpeg's
 *           coefficient arrays hold).  A stack of F frames, (F*height) x width,
 *           gives each frame's blocks contiguously, frame after frame.
 *   forward uint8 frame -> blocks.  Built-in T, the library Q, level shift 128.
 *           The values equal hpdct_forward U8 -> F32 on the same frame, cast
 *           to int16 (a -0.0 becomes 0); the quotient is chosen as
 *           hpdct_forward chooses it.  int16 holds every |q| <= 32767, i.e.
 *           every table with |Q| >= 1/31 everywhere (|C| <= 1024 with the
 *           built-in T), so also the tables HPDCT_I8 refuses (any DC entry
 *           below ~8.06, e.g. libjpeg's quality-75 luminance table); a table
 *           that can exceed it returns HPDCT_ERROR_RANGE.
 *   inverse blocks -> out_type HPDCT_F32 (R+128, no clamp) or HPDCT_U8 (clamp
 *           + truncate) pixels: equal, bit for bit, to hpdct_inverse F32 ->
 *           out_type on the spatial fp32 plane that holds (float)block value.
 *   d_blocks 16-byte aligned, height*width int16; d_image 8-byte (HPDCT_U8) or
 *   16-byte (HPDCT_F32) aligned; the two must not overlap.  flags:
 *   HPDCT_BLOCKS_NATURAL or 0, anything else HPDCT_ERROR_UNSUPPORTED.
 *   Asynchronous on `stream`.  hpdct_set_mapping does not affect these calls:
 *   only the one-lane-per-tile mapping exists for them. */
#define HPDCT_BLOCKS_NATURAL 0x1u /* within a block: row-major (v,u) order instead of zig-zag */
hpdct_status hpdct_forward_blocks(const uint8_t* d_image, int16_t* d_blocks, int64_t height, int64_t width,
                                  unsigned flags, void* stream);
hpdct_status hpdct_inverse_blocks(const int16_t* d_blocks, void* d_image, hpdct_dtype out_type, int64_t height,
                                  int64_t width, unsigned flags, void* stream);
void hpdct_zigzag_order(uint8_t* z64); /* z64[n] = 8*v+u of the n-th zig-zag coefficient (host memory) */

/* Colour frames: interleaved uint8 RGB <-> three arrays of int16 blocks (Y, Cb,
 * Cr), 4:4:4 or 4:2:0, one kernel launch per direction (no reference
 * counterpart: the reference is grey-scale).  Everything is integer arithmetic
 * around the block transform above, so every result is exact; these formulas
 * are the specification.
 *   input   d_rgb: height rows of width pixels, dense: the row pitch is
 *           3*width bytes and byte 3*x + c of a row is channel c (R, G, B) of
 *           pixel x.  HPDCT_SUBSAMPLING_444: height and width positive
 *           multiples of 8; HPDCT_SUBSAMPLING_420: of 16.  A stack of F frames
 *           is the one image (F*height) x width.  The tile-count limit is
 *           hpdct_forward_blocks' ((height/8)*(width/8) < 2^32).
 *   convert per pixel, in int32 (every result is 0..255 without a clamp):
 *             Y  = ( 19595*R + 38470*G +  7471*B + 32768) >> 16
 *             Cb = (-11059*R - 21709*G + 32768*B + (128<<16) + 32767) >> 16
 *             Cr = ( 32768*R - 27439*G -  5329*B + (128<<16) + 32767) >> 16
 *   4:2:0   each chroma sample is (a + b + c + d + 2) >> 2 over the 2x2 quad of
 *           the converted per-pixel Cb (Cr) values: convert, then average.
 *   forward each component plane (Y: height x width; Cb, Cr: the same for
 *           4:4:4, height/2 x width/2 for 4:2:0) goes through exactly
 *           hpdct_forward_blocks' arithmetic: built-in T, level shift 128, the
 *           quotient, the cast to int16 (-0.0 becomes 0).  Y is quantised with
 *           the luma table, Cb and Cr with the chroma table.  d_y, d_cb, d_cr
 *           are three separate block arrays, each laid out as
 *           hpdct_forward_blocks lays out that plane (block t = tile t of the
 *           component plane in row-major tile order; zig-zag inside, or
 *           row-major with HPDCT_BLOCKS_NATURAL): d_y is bit for bit what
 *           hpdct_forward_blocks writes for the Y plane under the luma table,
 *           and each array can go straight into hpdct_inverse_blocks.
 *   tables  q_luma64, q_chroma64: HOST pointers to 64 floats, read during the
 *           call and passed to the kernel with its arguments: no process-wide
 *           state, so calls with different tables may run on different streams
 *           at once.  q_luma64 NULL: the library-owned table
 *           (hpdct_set_quant_table).  q_chroma64 NULL: the JPEG Annex K
 *           chrominance table (hpdct_default_chroma_quant_table).  Entries
 *           must be finite and non-zero (HPDCT_ERROR_INVALID_VALUE); a table
 *           that can give |q| > 32767 returns HPDCT_ERROR_RANGE.  The result
 *           does not depend on which quotient form the library picks.
 *   inverse each component's blocks through hpdct_inverse_blocks' arithmetic to
 *           uint8 (clamp + truncate): Y, Cb, Cr.  4:2:0 chroma is replicated:
 *           chroma sample (i, j) serves pixels (2i..2i+1, 2j..2j+1).  Then, in
 *           int32 with arithmetic (flooring) right shifts,
 *             R = clamp255(Y + (( 91881*(Cr-128) + 32768) >> 16))
 *             G = clamp255(Y + ((-22554*(Cb-128) - 46802*(Cr-128) + 32768) >> 16))
 *             B = clamp255(Y + ((116130*(Cb-128) + 32768) >> 16))
 *           written as interleaved uint8 RGB in the input layout.  Without
 *           quantisation loss the pair is the identity to within +-1 a channel.
 *   All four device pointers 16-byte aligned; no buffer may overlap another.
 *   flags: HPDCT_BLOCKS_NATURAL or 0, anything else HPDCT_ERROR_UNSUPPORTED; an
 *   unknown subsampling HPDCT_ERROR_INVALID_VALUE.  Asynchronous on `stream`;
 *   every argument is checked before any device call.  hpdct_set_mapping does
 *   not affect these calls. */
typedef enum hpdct_subsampling { HPDCT_SUBSAMPLING_444 = 0, HPDCT_SUBSAMPLING_420 = 1 } hpdct_subsampling;
void hpdct_default_chroma_quant_table(float* q64); /* 64 floats, row-major (host memory) */
hpdct_status hpdct_forward_rgb_blocks(const uint8_t* d_rgb, int16_t* d_y, int16_t* d_cb, int16_t* d_cr,
                                      int64_t height, int64_t width, hpdct_subsampling sub,
                                      const float* q_luma64, const float* q_chroma64, unsigned flags, void* stream);
hpdct_status hpdct_inverse_rgb_blocks(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, uint8_t* d_rgb,
                                      int64_t height, int64_t width, hpdct_subsampling sub,
                                      const float* q_luma64, const float* q_chroma64, unsigned flags, void* stream);

/* Colour frames of any size and row pitch: the two calls above for a frame
 * that is not whole units, is a region of a larger frame, or has padded rows.
 * As every JPEG codec defines it, the frame is extended to whole units (8x8
 * tiles for 4:4:4, 16x16 MCUs for 4:2:0) by repeating its last column and its
 * last row; the padded blocks are coded and the inverse crops.  Still one
 * kernel launch per direction, no copy of the frame.
 *   sizes   height, width >= 1, any value.  pitch_bytes >= 3*width, any value;
 *           d_rgb has any alignment.  Row r starts at d_rgb + r*pitch_bytes;
 *           byte 3*x + c of the row is channel c of pixel x.  The RGB extent,
 *           for the overlap check, is (height-1)*pitch_bytes + 3*width bytes.
 *   padded  Hp, Wp: height, width rounded up to a multiple of 8 (4:4:4) or 16
 *           (4:2:0); (Hp/8)*(Wp/8) < 2^32.  The three block arrays are sized
 *           and laid out for the Hp x Wp frame exactly as
 *           hpdct_forward_rgb_blocks lays them out: Hp*Wp int16 for d_y, the
 *           same (4:4:4) or a quarter (4:2:0) for d_cb and d_cr each; 16-byte
 *           aligned.  hpdct_rgb_frame_geometry (host only) returns Hp, Wp and
 *           the block counts Hp*Wp/64 and (4:2:0) Hp*Wp/256; each output
 *           pointer may be NULL.
 *   forward bit for bit what hpdct_forward_rgb_blocks writes for the Hp x Wp
 *           frame P with P[r][x] = frame[min(r, height-1)][min(x, width-1)]:
 *           replication first, then the conversion, then the 2x2 average (a
 *           4:2:0 quad that straddles the edge averages replicated pixels).
 *   inverse bit for bit the top-left height x width pixels of what
 *           hpdct_inverse_rgb_blocks writes for the Hp x Wp block arrays.
 *           Bytes 3*width .. pitch_bytes-1 of a row are not written, and
 *           nothing past the last row's 3*width bytes is.
 *   Tables, flags, subsampling, the quotient forms and the independence from
 *   hpdct_set_mapping are those of the two calls above; these two also take
 *   HPDCT_FRAME_DCT (below, after the grey frame calls).  Refused with
 *   HPDCT_ERROR_INVALID_VALUE: pitch_bytes < 3*width; a height or width below
 *   1; the padded tile-count limit; a null pointer; a block pointer that is
 *   not 16-byte aligned; buffers that overlap (the RGB buffer with its pitched
 *   extent).  With Hp == height, Wp == width and pitch_bytes == 3*width the
 *   call is hpdct_forward_rgb_blocks / hpdct_inverse_rgb_blocks without their
 *   size and d_rgb alignment rules.
 *   Speed: a frame of whole units whose d_rgb and pitch_bytes are multiples of
 *   8 runs the same kernel as the calls above.  Other frames run a general
 *   kernel: only the units cut by the frame's edge pay for it while d_rgb and
 *   pitch_bytes are multiples of 8; with an unaligned base or pitch every unit
 *   moves its RGB bytes one at a time: pad the pitch to a
 *   multiple of 8 where the producer allows it. */
hpdct_status hpdct_rgb_frame_geometry(int64_t height, int64_t width, hpdct_subsampling sub, int64_t* padded_height,
                                      int64_t* padded_width, int64_t* y_blocks, int64_t* chroma_blocks);
hpdct_status hpdct_forward_rgb_frame(const uint8_t* d_rgb, int64_t pitch_bytes, int16_t* d_y, int16_t* d_cb,
                                     int16_t* d_cr, int64_t height, int64_t width, hpdct_subsampling sub,
                                     const float* q_luma64, const float* q_chroma64, unsigned flags, void* stream);
hpdct_status hpdct_inverse_rgb_frame(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, uint8_t* d_rgb,
                                     int64_t pitch_bytes, int64_t height, int64_t width, hpdct_subsampling sub,
                                     const float* q_luma64, const float* q_chroma64, unsigned flags, void* stream);

/* Grey frames of any size, row pitch and quant table: hpdct_forward_blocks and
 * hpdct_inverse_blocks (to uint8) for a frame that is not whole tiles, is a
 * region of a larger frame or has padded rows, quantised with a table that is
 * passed with the call.  As for the colour frames above, the frame is extended
 * to whole 8x8 tiles by repeating its last column and its last row; the padded
 * blocks are coded and the inverse crops.  One kernel launch per direction, no
 * copy of the frame, no process-wide state.
 *   sizes   height, width >= 1, any value.  pitch_bytes >= width, any value;
 *           d_image has any alignment.  Row r starts at d_image + r*pitch_bytes;
 *           byte x of the row is pixel x.  The image extent, for the overlap
 *           check, is (height-1)*pitch_bytes + width bytes.
 *   padded  Hp, Wp: height, width rounded up to a multiple of 8;
 *           (Hp/8)*(Wp/8) < 2^32.  d_blocks is 16-byte aligned and holds Hp*Wp
 *           int16, laid out exactly as hpdct_forward_blocks lays out the
 *           Hp x Wp plane (block t = tile t in row-major tile order; zig-zag
 *           inside, or row-major with HPDCT_BLOCKS_NATURAL), so it can go
 *           straight into hpdct_encode_scan or hpdct_inverse_blocks.
 *           hpdct_grey_frame_geometry (host only) returns Hp, Wp and the block
 *           count Hp*Wp/64; each output pointer may be NULL.
 *   table   q64: a HOST pointer to 64 floats (row-major), read during the call
 *           and passed to the kernel with its arguments: no process-wide state,
 *           so calls with different tables may run on different streams at
 *           once.  NULL: the library-owned table (hpdct_set_quant_table) at the
 *           time of the call.  The rules are those of the colour calls' luma
 *           table: entries must be finite and non-zero
 *           (HPDCT_ERROR_INVALID_VALUE); a table that can give |q| > 32767
 *           returns HPDCT_ERROR_RANGE.  The result does not depend on which
 *           quotient form the library picks.
 *   forward bit for bit what hpdct_forward_blocks writes for the Hp x Wp plane P
 *           with P[r][x] = frame[min(r, height-1)][min(x, width-1)] while the
 *           library table equals q64.
 *   inverse bit for bit the top-left height x width pixels of what
 *           hpdct_inverse_blocks(..., HPDCT_U8, ...) writes for the Hp x Wp
 *           blocks while the library table equals q64 (a table so large that
 *           q*Q or a partial sum may overflow runs every term of T, as there).
 *           Bytes width .. pitch_bytes-1 of a row are not written, and nothing
 *           past the last row's width bytes is.  uint8 output only: fp32 pixels
 *           stay with hpdct_inverse_blocks.
 *   flags: HPDCT_BLOCKS_NATURAL, HPDCT_FRAME_DCT (below), both or 0, anything
 *   else HPDCT_ERROR_UNSUPPORTED.
 *   Asynchronous on `stream`; every argument is checked before any device
 *   call; hpdct_set_mapping does not affect these calls.  Refused with
 *   HPDCT_ERROR_INVALID_VALUE: pitch_bytes < width; a height or width below 1;
 *   the padded tile-count limit; an image extent that overflows; a null
 *   pointer; a block pointer that is not 16-byte aligned; buffers that overlap
 *   (the image with its pitched extent).  With Hp == height, Wp == width,
 *   pitch_bytes == width and q64 == NULL the calls are hpdct_forward_blocks /
 *   hpdct_inverse_blocks to HPDCT_U8 without their size and d_image alignment
 *   rules.
 *   Speed: a frame of whole tiles whose d_image and pitch_bytes are multiples
 *   of 8 runs at the speed of the two calls above.  Other frames run a general
 *   kernel: only the tiles cut by the frame's edge pay for it while d_image and
 *   pitch_bytes are multiples of 8; with an unaligned base or pitch every tile
 *   moves its pixels one byte at a time: pad the pitch to a
 *   multiple of 8 where the producer allows it. */
hpdct_status hpdct_grey_frame_geometry(int64_t height, int64_t width, int64_t* padded_height, int64_t* padded_width,
                                       int64_t* blocks);
hpdct_status hpdct_forward_grey_frame(const uint8_t* d_image, int64_t pitch_bytes, int16_t* d_blocks, int64_t height,
                                      int64_t width, const float* q64, unsigned flags, void* stream);
hpdct_status hpdct_inverse_grey_frame(const int16_t* d_blocks, uint8_t* d_image, int64_t pitch_bytes, int64_t height,
                                      int64_t width, const float* q64, unsigned flags, void* stream);

/* The exact DCT on the four frame calls above (hpdct_forward_grey_frame,
 * hpdct_inverse_grey_frame, hpdct_forward_rgb_frame, hpdct_inverse_rgb_frame):
 * with HPDCT_FRAME_DCT in `flags` (alone or with HPDCT_BLOCKS_NATURAL) the call
 * transforms with the matrix of hpdct_dct_transform instead of HpApprDCT's, so
 * the blocks are what a standard JPEG decoder expects and a standard file's
 * blocks invert to its picture.  Every other entry point
 * refuses the bit with HPDCT_ERROR_UNSUPPORTED; without it nothing changes.
 *   forward the arithmetic contract of the unflagged call with T replaced: the
 *           level shift X - 128, P = T.X and C = P.T^T as fp32 FMA chains over
 *           i = 0..7 from +0, q = roundf(C / Q) (half away from zero), on the
 *           edge-replicated padded plane (each component plane for colour); the
 *           same block layout.  Every quotient form the library may pick gives
 *           that integer: the verified 3-op quotient covers |C| <= 4096 and
 *           the DCT's rows have L1 norm <= 2.8284272, so |C| < 1025; the
 *           default table's per-position forms are never used here.
 *   inverse D = q * Q as today, P = T^T.D and R = P.T as FMA chains with every
 *           term kept (the matrix has no zero entry: a table of any size takes
 *           the same path, and 0 * inf cannot arise from T), then each pixel
 *           is (R + 128.5f) in one fp32 add, clamped to [0, 255] and
 *           truncated: round half up, what JPEG decoders do, where the
 *           unflagged call truncates R + 128.  For colour the three component
 *           planes are made this way and the fixed-point conversion above is
 *           unchanged.
 *   table   the rules of the unflagged call; the |q| <= 32767 range rule is
 *           judged with the DCT's row norms (HPDCT_ERROR_RANGE).
 *   Sizes, pitches, alignment, padding, cropping, refusals, streams and the
 *   independence from hpdct_set_mapping are those of the unflagged call.  One
 *   kernel launch per direction, the general kernel of the unflagged call for
 *   every frame (DESIGN.md 4.13 has the cost). */
#define HPDCT_FRAME_DCT 0x100u

/* Baseline-JPEG entropy coding on the device: the block arrays above -> the
 * bytes of one interleaved Huffman scan (ITU-T T.81, baseline sequential), and
 * on the host the file header that goes in front of them (no reference
 * counterpart).
 *   input   d_y, d_cb, d_cr: exactly what hpdct_forward_blocks,
 *           hpdct_forward_rgb_blocks and hpdct_forward_rgb_frame write; height
 *           and width are those of the padded frame (Hp x Wp).  d_cb == d_cr ==
 *           NULL: one component (grey), MCU = one block, sizes multiples of 8,
 *           `sub` not read.  Else three components: sizes multiples of 8
 *           (4:4:4, MCU = Y Cb Cr) or 16 (4:2:0, MCU = Y(0,0) Y(0,1) Y(1,0)
 *           Y(1,1) Cb Cr, Y(dy,dx) = tile (2 my + dy, 2 mx + dx) of the Y plane).
 *           MCUs in row-major order.  flags: 0 (zig-zag blocks) or
 *           HPDCT_BLOCKS_NATURAL (permuted on load).
 *   coding  the four typical tables of Annex K.3 (hpdct_huffman_table):
 *           luminance DC / AC for Y, chrominance DC / AC for Cb and Cr.  DC
 *           difference against the previous block of the same component,
 *           magnitude category + extra bits (a negative v as v + 2^n - 1), AC
 *           (run, size) symbols with ZRL for runs of 16 or more, EOB unless
 *           coefficient 63 is non-zero; bits MSB first, every 0xFF byte
 *           followed by 0x00.
 *   restart restart_interval: 0 (the scan is one interval) or 1..65535 MCUs.
 *           Each interval ends padded with 1 bits to a whole byte; every
 *           interval but the last is followed by FF D0+(i mod 8), i its 0-based
 *           index; the DC predictors are 0 at each interval's start.
 *           d_interval_offsets (optional, intervals + 1 uint64): entry i is the
 *           byte offset of interval i's first byte, entry `intervals` equals
 *           info.bytes.  intervals = ceil(MCUs / restart_interval), or 1.
 *   output  d_scan[0 .. info.bytes), any alignment; no byte at or beyond
 *           d_scan + capacity is written, whatever the input.  If the scan does
 *           not fit, info.truncated = 1, info.bytes = the size it needs and the
 *           buffer holds nothing usable.  *d_info is written by the device.
 *   range   a DC difference beyond +-2047 or an AC value beyond +-1023 has no
 *           baseline code: each such coefficient is counted in
 *           info.out_of_range and the bytes are then unspecified; the call is
 *           still memory-safe and info.bytes <= hpdct_scan_bound.
 *   bound   hpdct_scan_bound(blocks, intervals) = 415 * blocks + 4 * intervals
 *           (-1 for a negative argument or an overflow): a block is at most
 *           (11 + 11) + 63 * (16 + 10) = 1660 bits (longest DC code + 11 extra
 *           bits, 63 times the longest AC code + 10), 207.5 bytes, twice that
 *           when every byte is stuffed; an interval adds at most one padded,
 *           stuffed byte (2) and its marker (2).
 *   scratch no allocation, no process-wide state: d_workspace, at least
 *           hpdct_scan_workspace_bytes(...) bytes (16 per interval at most; -1
 *           for arguments the call would refuse), is all the call uses, so it
 *           can be captured into a graph.  Three kernel launches in one chain,
 *           asynchronous on `stream`.
 *   speed   one wave codes one restart interval, so the call is parallel across
 *           intervals only: tuned for one MCU row per interval;
 *           restart_interval = 0 serialises the whole frame on one wave.
 *   Every argument is checked before any device call.
 *   HPDCT_ERROR_INVALID_VALUE: a null d_y, d_scan, d_info or d_workspace, only
 *   one of d_cb / d_cr null; sizes that are not positive multiples of the MCU
 *   or past the tile-count limit; an unknown subsampling (three components);
 *   restart_interval outside 0..65535; a negative capacity; a block, workspace
 *   or offsets pointer that is not 16-byte aligned, d_info not 8-byte aligned;
 *   workspace_bytes too small; any two buffers overlapping.
 *   HPDCT_ERROR_UNSUPPORTED: unknown flag bits. */
typedef struct hpdct_scan_info {
    uint64_t bytes;        /* length of the scan data; if truncated, the length it needs */
    uint32_t truncated;    /* 1: bytes > capacity, the output holds nothing usable */
    uint32_t out_of_range; /* number of coefficients baseline Huffman cannot code */
} hpdct_scan_info;
hpdct_status hpdct_encode_scan(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, int64_t height,
                               int64_t width, hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                               uint8_t* d_scan, int64_t capacity, hpdct_scan_info* d_info,
                               uint64_t* d_interval_offsets, void* d_workspace, int64_t workspace_bytes,
                               void* stream);
int64_t hpdct_scan_bound(int64_t blocks, int64_t intervals); /* host: worst-case bytes */
int64_t hpdct_scan_workspace_bytes(int64_t height, int64_t width, int components, hpdct_subsampling sub,
                                   int64_t restart_interval); /* host */
/* The file around the scan (host only): SOI, JFIF APP0, DQT (8-bit, zig-zag
 * order), SOF0, DHT, DRI when restart_interval > 0, SOS (Ss = 0, Se = 63, Ah/Al =
 * 0) into h_out; *bytes = the header's length (also when capacity is too small:
 * HPDCT_ERROR_INVALID_VALUE, nothing written).  The caller appends the scan and
 * FF D9.  height, width: the TRUE frame size, each 1..65535 (the scan holds the
 * padded MCUs, which is what hpdct_forward_rgb_frame's edge replication
 * produces).  components 1 (one DQT, two DHT tables) or 3 (two and four;
 * sampling 1x1 for 4:4:4, 2x2 / 1x1 / 1x1 for 4:2:0; `sub` not read for 1).
 * q_luma64 NULL: the library table; q_chroma64 NULL: the Annex K table (not
 * read for 1 component); an entry that is not an integer in 1..255 returns
 * HPDCT_ERROR_RANGE.
 * A standard decoder inverts with the exact DCT, while this library's T is the
 * HpApprDCT approximation: such a file decodes to an approximation of what
 * hpdct_inverse_* gives for the same blocks (DESIGN.md 4.8 records how close).
 * hpdct_huffman_table: bits16[l-1] = number of codes of length l, vals[0 ..
 * *nvals) the symbols in code order (12 for a DC table, 162 for an AC table);
 * an unknown kind sets *nvals = 0.  Any output pointer may be NULL. */
hpdct_status hpdct_jpeg_header(uint8_t* h_out, int64_t capacity, int64_t* bytes, int64_t height, int64_t width,
                               int components, hpdct_subsampling sub, const float* q_luma64,
                               const float* q_chroma64, int64_t restart_interval);
void hpdct_huffman_table(int kind /* 0 DC-luma, 1 AC-luma, 2 DC-chroma, 3 AC-chroma */, uint8_t* bits16, uint8_t* vals,
                         int* nvals);

/* Baseline-JPEG entropy DEcoding on the device: the inverse of hpdct_encode_scan
 * (no reference counterpart).  The bytes of one interleaved Huffman scan -> the
 * int16 block arrays hpdct_inverse_blocks, hpdct_inverse_rgb_blocks and
 * hpdct_inverse_rgb_frame take.  The geometry (height and width of the padded
 * frame, d_cb == d_cr == NULL for one component, the MCU order), `flags` (0 or
 * HPDCT_BLOCKS_NATURAL, permuted on store), the four Annex K.3 tables and the
 * restart rules are those of hpdct_encode_scan.
 *   input   d_scan[0 .. bytes), bytes >= 0, any alignment: the scan data alone
 *           (what hpdct_encode_scan writes; hpdct_jpeg_parse finds it in a
 *           file).  The bytes are untrusted: whatever they and the offsets
 *           hold, nothing outside d_scan[0, bytes) is read and nothing outside
 *           the block arrays, *d_info, d_interval_status and the workspace is
 *           written; every block of the frame is written exactly once per call.
 *   where an interval's bytes are
 *           d_interval_offsets given (the table hpdct_encode_scan writes,
 *           intervals + 1 uint64, device data and untrusted too): interval i is
 *           [offs[i], offs[i+1] - 2), the last one [offs[i], offs[i+1]); an
 *           interval whose bounds are not 0 <= lo <= hi <= bytes has status
 *           RANGE and reads nothing.
 *           NULL: the call locates the markers itself.  A marker is any
 *           position p with scan[p] == 0xFF, 0xD0 <= scan[p+1] <= 0xD7 and
 *           p + 1 < bytes (stuffing guarantees that no such pair occurs inside
 *           coded data).  Interval 0 starts at 0, interval i two bytes after the
 *           i-th marker in byte order, whatever its number; an interval ends at
 *           the next marker, or at `bytes`.  Intervals with no marker have
 *           status MISSING; markers beyond intervals - 1 are only counted.  FF
 *           fill bytes before a marker are not supported: they show as a MARKER
 *           or TAIL status.
 *   status  per interval, uint64 = code + 256 * index of the failing block
 *           within the interval; 0 for a clean interval:
 *             1 RANGE    bad offsets, as above; block 0
 *             2 MARKER   an FF inside the interval followed by anything but 00
 *             3 END      a bit is needed and the interval has no byte left
 *                        (also an FF as its last byte)
 *             4 CODE     16 bits read and no code of the component's table matches
 *             5 INDEX    a (run, size) symbol places a coefficient beyond index
 *                        63 (judged before its extra bits are read), or a ZRL
 *                        moves past 64
 *             6 DC       predictor + difference does not fit int16
 *             7 TAIL     all blocks decoded, but the rest of the current byte is
 *                        not all 1 bits, or bytes remain; the blocks stay as
 *                        decoded, block index 0
 *             8 MISSING  no marker for this interval; block 0
 *           MARKER and END are raised when a bit of the byte in question is
 *           needed, not before.  The predictors are 0 at each interval's start,
 *           bits are MSB first, extra bits v of size n below 2^(n-1) stand for
 *           v - 2^n + 1.  For the codes 1-6 and 8 the failing block and every
 *           later block of that interval are written as 64 zeros; the blocks
 *           before it keep what was decoded.
 *   output  *d_info (written by the device) and, when given, d_interval_status
 *           (`intervals` entries).
 *   scratch no allocation, no process-wide state: d_workspace, at least
 *           hpdct_decode_workspace_bytes(...) bytes (8 per interval and 8 per
 *           4096 bytes of scan; -1 for arguments the call would refuse), is all
 *           the call uses, so it can be captured into a graph.  Two launches in
 *           one chain with offsets, four without, asynchronous on `stream`.
 *   speed   one LANE walks one restart interval, so the call is parallel
 *           across intervals only; hpdct_decode_scan_split
 *           below is parallel inside an interval as well: 12 times faster at
 *           one MCU row of noise per interval at 8192^2, slower below some
 *           3 KB an interval.
 *   Every argument is checked before any device call.
 *   HPDCT_ERROR_INVALID_VALUE: a null d_scan, d_y, d_info or d_workspace, only
 *   one of d_cb / d_cr null; sizes that are not positive multiples of the MCU
 *   or past the tile-count limit; an unknown subsampling (three components);
 *   restart_interval outside 0..65535; negative bytes; a block, workspace,
 *   offsets or status pointer that is not 16-byte aligned, d_info not 8-byte
 *   aligned; workspace_bytes too small; any two buffers overlapping.
 *   HPDCT_ERROR_UNSUPPORTED: unknown flag bits. */
typedef struct hpdct_decode_info { /* written by the device; 8-byte aligned */
    uint32_t bad_intervals;  /* intervals whose status is not 0 */
    uint32_t markers_found;  /* RSTn markers located (0 when offsets were given) */
    uint32_t marker_errors;  /* located markers among the first intervals-1 whose number is not i mod 8 */
    uint32_t reserved;       /* 0 */
} hpdct_decode_info;
hpdct_status hpdct_decode_scan(const uint8_t* d_scan, int64_t bytes, const uint64_t* d_interval_offsets /* or NULL */,
                               int16_t* d_y, int16_t* d_cb, int16_t* d_cr, int64_t height, int64_t width,
                               hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                               hpdct_decode_info* d_info, uint64_t* d_interval_status /* or NULL */,
                               void* d_workspace, int64_t workspace_bytes, void* stream);
int64_t hpdct_decode_workspace_bytes(int64_t height, int64_t width, int components, hpdct_subsampling sub,
                                     int64_t restart_interval, int64_t scan_bytes); /* host; -1 if refused */
/* hpdct_decode_scan, parallel INSIDE a restart interval as well (DESIGN.md
 * 4.10): the arguments of hpdct_decode_scan and split_min_bytes.  An interval of
 * at least split_min_bytes bytes is split into segments, one lane each; 0: the
 * library's choice (3328); 1: every interval that is not empty; negative:
 * HPDCT_ERROR_INVALID_VALUE.
 *   contract  the block arrays, the status array and the first 16 bytes of
 *           *d_info are, for every input whatever, bit for bit what
 *           hpdct_decode_scan writes.  Everything its paragraph says about
 *           untrusted bytes and offsets holds unchanged, except that a block
 *           may be stored more than once.
 *   method  a lane walks a 256-byte segment from its first byte as if a block
 *           began there; Huffman codes fall into step, so most walks end where
 *           the true decode stands there.  Each lane then walks again from its
 *           predecessor's exit until nothing changes: inside a group of 256
 *           segments in one launch, between groups in 4 launches more.  The
 *           blocks of an interval are taken from the split walks only when every
 *           segment entered at its predecessor's exit (segment 0 at the true
 *           start), no walk met an error, the blocks number what the geometry
 *           says, the interval ends as TAIL demands and every DC fits int16.
 *           Every other interval is decoded as hpdct_decode_scan decodes it, by
 *           one lane, which also gives the exact status.  An interval of at most
 *           5 groups (320 KiB) always reaches the fixed point.
 *   info    hpdct_decode_split_info, 8-byte aligned: hpdct_decode_info's four
 *           words, then the intervals that were split, those walked by one lane
 *           (never split, or split and decoded again), those split but not at a
 *           fixed point after the last launch, and the last of the 4 launches
 *           between groups in which a group changed (0: none did).
 *   scratch d_workspace, at least hpdct_decode_split_workspace_bytes(...)
 *           bytes (hpdct_decode_scan's, 16 per interval and group and 64 per
 *           segment more; -1 for arguments the call would refuse).  Eleven
 *           launches in one chain with offsets, thirteen without; none depends
 *           on a value the host reads, so the call can be captured into a graph.
 *   speed   8192^2 noise at one MCU row per interval: 3.0 ms against
 *           hpdct_decode_scan's 35.7; a 1080p noise frame without restart
 *           markers 2.6 ms against 781.  The chain costs 2 ms whatever it
 *           decodes, and short intervals run mostly idle workgroups: at 8 MCUs
 *           per interval it is 60 times slower when every interval is split
 *           (DESIGN.md 4.10), hence the threshold.
 * The checks and their errors are hpdct_decode_scan's. */
typedef struct hpdct_decode_split_info { /* written by the device; 8-byte aligned */
    uint32_t bad_intervals, markers_found, marker_errors, reserved; /* as hpdct_decode_info */
    uint32_t split_intervals;     /* intervals cut into segments */
    uint32_t serial_intervals;    /* intervals walked by one lane: never split, or decoded again */
    uint32_t unsettled_intervals; /* split, but not at a fixed point after the last launch */
    uint32_t rounds;              /* the last launch between groups that changed a group's entry */
} hpdct_decode_split_info;
hpdct_status hpdct_decode_scan_split(const uint8_t* d_scan, int64_t bytes,
                                     const uint64_t* d_interval_offsets /* or NULL */, int16_t* d_y, int16_t* d_cb,
                                     int16_t* d_cr, int64_t height, int64_t width, hpdct_subsampling sub,
                                     int64_t restart_interval, unsigned flags, int64_t split_min_bytes,
                                     hpdct_decode_split_info* d_info, uint64_t* d_interval_status /* or NULL */,
                                     void* d_workspace, int64_t workspace_bytes, void* stream);
int64_t hpdct_decode_split_workspace_bytes(int64_t height, int64_t width, int components, hpdct_subsampling sub,
                                           int64_t restart_interval, int64_t scan_bytes); /* host; -1 if refused */
/* the bytes of a segment, the segments of a group, the launches between groups (host) */
void hpdct_decode_split_geometry(int* segment_bytes, int* group_segments, int* rounds);
/* The header of a baseline file (host only), the inverse of hpdct_jpeg_header:
 * walks SOI .. SOS of h_file[0 .. bytes) and never reads outside it.  APPn and
 * COM segments are skipped; a DQT or DHT segment may hold one table or several.
 * scan_offset: the first byte after the SOS header; scan_bytes runs to the
 * first marker after it that is neither FF 00 nor RSTn, which must be EOI.
 * height, width: the TRUE frame size; q_luma, q_chroma: row-major, as the
 * library's own tables (q_chroma is not written for one component).
 * HPDCT_ERROR_UNSUPPORTED, the message naming the reason, for what
 * hpdct_decode_scan cannot decode: a frame that is not SOF0 with 8-bit samples;
 * a 16-bit DQT; component counts other than 1 or 3; sampling other than 1x1
 * (grey), 1x1 / 1x1 / 1x1 or 2x2 / 1x1 / 1x1; Cb and Cr on different quant
 * tables; a Huffman table selected by a component whose contents differ from
 * the Annex K luminance table (component 0) or chrominance table (the others);
 * more than one scan; Ss / Se / Ah / Al other than 0 / 63 / 0 / 0.
 * HPDCT_ERROR_INVALID_VALUE: a null pointer, a truncated or malformed file. */
typedef struct hpdct_jpeg_layout {
    int64_t height, width;
    int components;
    hpdct_subsampling sub;
    int64_t restart_interval, scan_offset, scan_bytes;
    float q_luma[64], q_chroma[64];
} hpdct_jpeg_layout;
hpdct_status hpdct_jpeg_parse(const uint8_t* h_file, int64_t bytes, hpdct_jpeg_layout* out);

/* Huffman tables from the caller: the entropy coder and the
 * entropy decoders under any four tables a baseline DHT can carry, the
 * statistics of a frame's symbols, and the optimal tables for them.
 *
 * A table as a DHT segment holds it: bits[l-1] = the number of codes of length
 * l, vals[0 .. nvals) the symbols in order of increasing code length.  Kinds as
 * hpdct_huffman_table: 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma.  An
 * empty table (nvals == 0) is legal and codes nothing.
 *
 * hpdct_huffman_prepare (host only, no allocation, no process-wide state)
 * judges four specs and writes one POD blob of hpdct_huffman_blob_bytes()
 * bytes into h_blob: the coder's (length << 16) | code entries per symbol, then
 * the decoder's 8-bit lookup, maxcode, valoff and vals (256 symbols a table).
 * The caller copies the blob to device memory (16-byte aligned) and passes that
 * pointer as d_tables below.  HPDCT_ERROR_INVALID_VALUE, the message naming the
 * table and the reason: nvals is not the sum of bits or is above 256; the code
 * is over-subscribed (Kraft sum above 1 with the lengths assigned canonically);
 * a symbol appears twice; a DC symbol is above 15; a null pointer; capacity
 * below the blob's size.  The blob is the caller's data: the kernels mask every
 * index they form from it and clamp its code lengths to 16, so they stay
 * memory-safe whatever it holds, but only a blob prepare wrote gives a JPEG scan.
 *
 * hpdct_huffman_optimal (host only): the table of T.81 K.2 (figures K.1 - K.4)
 * for the symbol counts counts[0 .. 256): a pseudo-symbol 256 of count 1, so
 * that no symbol gets the all-ones code; the two smallest non-zero counts are
 * merged until one is left, on ties the larger symbol index for the first and
 * for the second choice; the lengths above 16 are adjusted as figure K.3 does;
 * the pseudo-symbol leaves the longest length; vals by length, then by symbol
 * value.  All-zero counts give nvals == 0, one non-zero count one code of
 * length 1.  A count above 2^54 is refused with HPDCT_ERROR_INVALID_VALUE (the
 * sum of all of them must stay below 2^63); a frame's counts stay below 2^38.
 *
 * hpdct_scan_histogram (device, one memset and one launch, no allocation, can
 * be captured into a graph): d_counts[kind * 256 + s], 4 * 256 uint64, 16-byte
 * aligned, overwritten, = exactly the number of times hpdct_encode_scan emits
 * symbol s of table kind for the same arguments: a DC category of the
 * difference hpdct_encode_scan codes (0 at an interval's start), a ZRL per 16
 * zeros, an EOB unless coefficient 63 is non-zero, the categories clamped to
 * 11 (DC) and 10 (AC) as the coder clamps them.  The pass is parallel over
 * blocks and does not depend on restart_interval.  Checks and errors:
 * hpdct_encode_scan's for the blocks, the geometry and the flags. */
typedef struct hpdct_huffman_spec {
    uint8_t bits[16];
    uint8_t vals[256];
    int32_t nvals;
} hpdct_huffman_spec;
int64_t hpdct_huffman_blob_bytes(void);
hpdct_status hpdct_huffman_prepare(const hpdct_huffman_spec specs[4], void* h_blob, int64_t capacity);
hpdct_status hpdct_huffman_optimal(const uint64_t counts[256], hpdct_huffman_spec* out);
hpdct_status hpdct_scan_histogram(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, int64_t height,
                                  int64_t width, hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                                  uint64_t* d_counts, void* stream);
/* hpdct_encode_scan, hpdct_decode_scan and hpdct_decode_scan_split with a table blob: d_tables NULL
 * means Annex K, bit for bit the calls without it.  Every documented contract
 * of those calls carries over.  With a 16-bit DC code a block reaches 27 + 63 *
 * 26 = 1665 bits, so the bound is hpdct_scan_bound_tables(blocks, intervals) =
 * 417 * blocks + 4 * intervals.  A symbol the caller's table has no code for is
 * counted in info.out_of_range; the bytes are then unspecified, the call still
 * memory-safe and info.bytes within the bound.  The decoder takes DC symbols up
 * to 15 (the int16 check of the DC stands); a code of an empty or incomplete
 * table ends the interval with status code 4 (CODE). */
int64_t hpdct_scan_bound_tables(int64_t blocks, int64_t intervals); /* host: worst-case bytes */
hpdct_status hpdct_encode_scan_tables(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, int64_t height,
                                      int64_t width, hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                                      uint8_t* d_scan, int64_t capacity, hpdct_scan_info* d_info,
                                      uint64_t* d_interval_offsets /* or NULL */, void* d_workspace,
                                      int64_t workspace_bytes, const void* d_tables /* or NULL */, void* stream);
hpdct_status hpdct_decode_scan_tables(const uint8_t* d_scan, int64_t bytes,
                                      const uint64_t* d_interval_offsets /* or NULL */, int16_t* d_y, int16_t* d_cb,
                                      int16_t* d_cr, int64_t height, int64_t width, hpdct_subsampling sub,
                                      int64_t restart_interval, unsigned flags, hpdct_decode_info* d_info,
                                      uint64_t* d_interval_status /* or NULL */, void* d_workspace,
                                      int64_t workspace_bytes, const void* d_tables /* or NULL */, void* stream);
/* hpdct_decode_scan_split under the caller's tables: bit for bit
 * hpdct_decode_scan_tables in blocks, status and the info's first three words. */
hpdct_status hpdct_decode_scan_split_tables(const uint8_t* d_scan, int64_t bytes,
                                            const uint64_t* d_interval_offsets /* or NULL */, int16_t* d_y,
                                            int16_t* d_cb, int16_t* d_cr, int64_t height, int64_t width,
                                            hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                                            int64_t split_min_bytes, hpdct_decode_split_info* d_info,
                                            uint64_t* d_interval_status /* or NULL */, void* d_workspace,
                                            int64_t workspace_bytes, const void* d_tables /* or NULL */,
                                            void* stream);
/* hpdct_jpeg_header with the tables to write into DHT (kinds 0, 1 alone for
 * one component): specs NULL means Annex K, byte for byte hpdct_jpeg_header;
 * specs that hpdct_huffman_prepare refuses are refused alike.
 * hpdct_jpeg_parse_tables: the walk and the refusals of hpdct_jpeg_parse,
 * except that any DHT hpdct_huffman_prepare accepts is accepted and returned
 * in specs[4]: Y selects kinds 0 / 1; Cb and Cr must select tables of equal
 * contents (kinds 2 / 3; one component: both empty), else
 * HPDCT_ERROR_UNSUPPORTED "Cb and Cr on different Huffman tables"; a table that
 * fails the validation gives HPDCT_ERROR_INVALID_VALUE with prepare's reason. */
hpdct_status hpdct_jpeg_header_tables(uint8_t* h_out, int64_t capacity, int64_t* bytes, int64_t height,
                                      int64_t width, int components, hpdct_subsampling sub, const float* q_luma64,
                                      const float* q_chroma64, int64_t restart_interval,
                                      const hpdct_huffman_spec specs[4] /* or NULL */);
hpdct_status hpdct_jpeg_parse_tables(const uint8_t* h_file, int64_t bytes, hpdct_jpeg_layout* out,
                                     hpdct_huffman_spec specs[4]);

/* Work mapping of the kernels (new; the reference has one fixed decomposition
 * per program).  Output is bit-identical in every mapping; only speed differs.
 *   AUTO   per frame: eight lanes per 8x8 tile ("octet") for frames below
 *          8 x 64-tile sets per CU; above that two lanes per tile ("duo") for
 *          fp32 -> fp32 and the fp32 -> uint8 inverse, one lane per tile for
 *          the rest (DESIGN.md "Kernels").
 *   TILE   one lane per tile always.     OCTET  eight lanes per tile always.
 *   DUO    two lanes per tile for every fp32 -> fp32 kernel and the fp32 -> uint8
 *          inverse, AUTO otherwise.
 * The cublasDCTv2 pass order (HPDCT_FLAG_ROW_FIRST) runs two lanes per tile
 * (rows first) except under TILE.  Process-wide; the initial value comes from the environment variable
 * HPDCT_MAPPING ("auto", "tile", "octet", "duo"), else AUTO.  For A/B
 * measurement and tests; set it while no call is in flight. */
typedef enum hpdct_mapping {
    HPDCT_MAPPING_AUTO = 0,
    HPDCT_MAPPING_TILE = 1,
    HPDCT_MAPPING_OCTET = 2,
    HPDCT_MAPPING_DUO = 3
} hpdct_mapping;
hpdct_status hpdct_set_mapping(hpdct_mapping mapping);
hpdct_mapping hpdct_get_mapping(void);

/* Host-side helpers (no device work). */
void hpdct_fill_rand_u8(uint8_t* h_out, int64_t n, uint32_t seed); /* srand(seed); rand()%256 (glibc TYPE_3) */
void hpdct_u8_to_f32(const uint8_t* h_in, float* h_out, int64_t n); /* convertToFloat, utils.cu:10-15 */
void hpdct_f32_to_u8(const float* h_in, uint8_t* h_out, int64_t n); /* convertToUnsignedChar, utils.cu:18-24 */

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HPDCT_H */
