/*
 * sc_engine.h -- C-ABI of the MI355X-native SpectralConv engine (libsc_engine.so).
 *
 * The reference (neuraloperator v2.0.0) is 100 % Python: its hot path is a chain of ATen
 * calls inside neuralop/layers/spectral_convolution.py and there is no FFI boundary
 * upstream.  This header is the boundary a maintainer would bind
 * with ctypes from a `conv_module` drop-in; every entry point cites
 * the reference lines it replaces.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types.  All data pointers are DEVICE pointers
 *     owned by the caller (PyTorch's allocator); the plan owns only its twiddle tables.
 *   - real tensors: float32 (bfloat16 storage with SC_PLAN_IO_BF16), contiguous (B, C, d1..dN).
 *     complex tensors: interleaved (re, im) float32 pairs (== torch.complex64 memory).
 *   - truncated spectra are stored (B, C, k1..kN) with the mode dims in WEIGHT order:
 *     non-last dim row r  <->  signed frequency r - floor(k/2) (fftshift order, even k
 *     keeps -k/2 .. k/2-1), last dim column c <-> frequency c.
 *     (spectral_convolution.py:465-519.)
 *   - every function returns 0 on success, non-zero on error (sc_last_error() gives the
 *     message); no C++ exception crosses the ABI.
 *   - all work is enqueued on the hipStream_t passed in (void* here so that the header is
 *     usable without HIP headers); nothing synchronises the device.
 *   - a plan is immutable after creation and may be used from several streams as long as
 *     each call gets its own workspace.
 */
#ifndef SC_ENGINE_H
#define SC_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_MAX_DIMS 4

/* fft_norm of the reference module (spectral_convolution.py:303, 443, 548, 559) */
enum { SC_NORM_FORWARD = 0, SC_NORM_BACKWARD = 1, SC_NORM_ORTHO = 2 };

/* which linear map a transform call applies (all four share kernels, only tables differ) */
enum {
  SC_FWD_SCALED = 0,   /* rfftn(norm) restricted to the kept modes      (:443-449, 500-519) */
  SC_FWD_ADJ_C2R = 1,  /* adjoint of the zero-padded inverse: unscaled R2C, interior
                          last-dim columns x2  (autograd of :531-559)           */
  SC_INV_PADDED = 0,   /* zero-pad + ifftn + irfft(norm), DC/Nyquist imag ignored (:520-559)*/
  SC_INV_ADJ_R2C = 1   /* adjoint of SC_FWD_SCALED (autograd of :443)           */
};

typedef struct sc_plan sc_plan;

typedef struct {
  int32_t ndim;                  /* number of spatial dims, 1..SC_MAX_DIMS                  */
  int32_t fft_norm;              /* SC_NORM_*                                               */
  int64_t spatial[SC_MAX_DIMS];  /* d1..dN                                                  */
  int64_t kept[SC_MAX_DIMS];     /* extents of the used weight sub-block = kept modes       */
  int32_t flags;                 /* SC_PLAN_* bits                                          */
  int32_t real_col;              /* last-dim column whose imaginary part the zero-padded inverse
                                    ignores besides DC / Nyquist: the reference zeroes Im of the
                                    INPUT grid's last half-spectrum column before an irfft onto a
                                    different grid (:552-556).  0 = none (DC is always ignored)  */
  /* Optional frequency maps (host arrays, read during sc_plan_create only; NULL = default):
   * freq[d][r], r < kept[d], is the FFT index on THIS plan's grid (0 .. spatial[d]-1, negative
   * values taken mod spatial[d]) that kept row r of dim d reads / is written to, or
   * SC_FREQ_DROPPED when the row falls off the grid.  Defaults: non-last dims r - floor(k/2),
   * last dim r (real data) -- the same-grid rule of :502-517.  The host passes explicit maps
   * for the reference's resolution-changing inverse (rows stay at their INPUT-grid FFT index,
   * :524-559), its complex-data branch and the skip-path resample (resample.py:54-66); see
   * neuraloperator_amd/modes.py.  A plan with maps never takes the fused power-of-two kernels. */
  const int64_t* freq[SC_MAX_DIMS];
} sc_plan_desc;
#define SC_FREQ_DROPPED INT64_MIN

enum {
  SC_PLAN_FORCE_GENERIC = 1, /* never take the power-of-two fast kernels (debug / A-B)     */
  SC_PLAN_FFT_GEN2 = 2,      /* fast path on the generation-2 fused kernels (A-B)           */
  SC_PLAN_NO_MDFT = 4,       /* generic passes on the VALU kernels instead of the matrix cores (A-B) */
  SC_PLAN_COMPLEX = 8,       /* complex_data=True (:439-441, 536-538): x and y are complex (n_images,
                                d1..dN), every dim is a complex-to-complex pass, bias must be NULL
                                (the host adds the real bias); transforms only, no sc_layer_*      */
  SC_PLAN_NO_F2P_SMALL = 32, /* keep grids of 64 .. 640 points per axis (32 P, P in {2,3,4,5,6,8,10,12,20}) on the
                                direct-DFT passes instead of the two-pass factorised route (round 3; A-B)  */
  SC_PLAN_F2P_SMALL_ALWAYS = 64, /* take the two-pass route for supported grids below 128 x 128 points too (A-B, tests:
                                by default those stay on the one-launch direct-DFT plane passes, which are faster there) */
  SC_PLAN_NO_SPAN = 128,     /* complex -> real last-axis pass of widths off every factorised route: the 128-line chunked
                                kernel (k_mdft_c2r_stage) instead of the 32-line whole-span one (k_mdft_c2r_span; A-B, tests) */
  SC_PLAN_NO_MX_FFT = 256,   /* bfloat16 I/O: the transforms on the vector-ALU kernels k_fft2d_fwd3 / k_fft2d_inv3 instead of
                                the matrix-core row passes k_fft2d_fwd_mx / k_fft2d_inv_mx (H <= 256; round 5; A-B and tests) */
  SC_PLAN_MX_FFT_3TERM = 512, /* bfloat16 I/O: the twiddles of k_fft2d_fwd_mx as THREE bf16 terms (24 bits: the spectrum of
                                fp32 round-off class, 1.2e-7 from a float64 transform of the same values) instead of the
                                default two (16 bits: 1.3e-6 -- 3000 x below the 2^-9 the bf16 input carries per value, 8 x
                                below the 1e-5 bar of the fp32 gradients; 10 us per launch faster at the metric shape; round 6) */
  SC_PLAN_PLAIN_CACHE_POLICY = 1024, /* round 8 (A-B and tests): every spectrum leaves its kernel with plain stores and
                                sc_layer_* asks the contractions for no cache policy -- round 7's policy at every site.
                                Default: k_fft2d_fwd3 stores xhat / ghat write-through (nothing of them is dirty in the L2s
                                at the kernel boundary); the contractions of sc_layer_* run round 7's policy either way
                                (write-through yhat / gxhat and a streamed weight did not pay).  Same bits */
  SC_PLAN_IO_BF16 = 16      /* the REAL tensors (x, y, gy, gx) are bfloat16 in memory -- the `float*`
                                arguments that carry them then point at 2-byte elements; spectra,
                                weights, bias and every arithmetic step stay float32 and y / gx are
                                rounded to nearest even on the store (BASELINE configs[1] "bf16": the
                                reference has no bf16 spectral path, torch.fft rejects the dtype, so this
                                is y = bf16(layer(fp32(x)))).  Fused 2-D kernels only: sc_plan_create
                                fails for shapes that take the size-agnostic passes (the host converts) */
};

/* ---- plan ------------------------------------------------------------------------------ */
/* replaces the per-call index math of spectral_convolution.py:429-434, 465-519 */
int sc_plan_create(sc_plan** out, const sc_plan_desc* desc);
void sc_plan_destroy(sc_plan* plan);
/* bytes of scratch a transform call over `n_images` (= batch*channels) images needs */
size_t sc_plan_workspace_bytes(const sc_plan* plan, int64_t n_images);
/* 1 if the plan runs the fused power-of-two kernels, 0 for the generic pruned-DFT passes */
int sc_plan_is_fast(const sc_plan* plan);

/* ---- transforms -------------------------------------------------------------------------- */
/* x: real (n_images, d1..dN) [complex with SC_PLAN_COMPLEX]  ->  xhat: complex (n_images, k1..kN)
 * replaces rfftn + fftshift + x[slices_x]      (spectral_convolution.py:443-449, 500-519) */
int sc_transform_forward(const sc_plan* plan, int mode, const float* x, float* xhat,
                         int64_t n_images, void* workspace, void* stream);

/* yhat: complex (n_images, k1..kN) -> y: real (n_images, d1..dN), y += bias[image % channels]
 * replaces zeros + out_fft[slices_x]= + ifftshift + ifftn + imag.zero_ + irfft + bias
 * (spectral_convolution.py:456-462, 520, 531-568).  bias may be NULL. */
int sc_transform_inverse(const sc_plan* plan, int mode, const float* yhat, const float* bias,
                         int64_t channels, float* y, int64_t n_images, void* workspace,
                         void* stream);

/* ---- mode-batched complex GEMM ---------------------------------------------------------------
 * C[p, q, m] (+)= sum_r opA(A[p, r, m]) * opB(B[r, q, m]),   m = 0..n_modes-1 on the lanes.
 * Element (complex) offsets: A: p*a_sp + r*a_sr + m*a_sm;  B: r*b_sr + q*b_sq + off_b(m);
 * C: p*c_sp + q*c_sq + off_c(m), where off(m) = idx[m] if the index table is given
 * (device int32, lets B / C be a strided sub-block of the stored weight), else m*sm.
 * a_sm / b_sm may be 0 (operand shared by all modes: Tucker/CP factor matrices).
 * replaces tl.einsum('bixy,ioxy->boxy') and its two autograd einsums
 * (spectral_convolution.py:21-46) and the pairwise steps of _contract_tucker/_contract_cp
 * (:55-103). */
enum {
  SC_GEMM_FORCE_VALU = 1,    /* never take the matrix-core kernel (debug / A-B)            */
  SC_GEMM_STREAM_C = 2,      /* C is not consumed by the next kernel: non-temporal stores    */
  SC_GEMM_PAIRED = 4,        /* P = 32: two 4-wave workgroups per CU, 5 modes each (A-B; slower from HBM) */
  SC_GEMM_WIDE = 8,          /* 9 modes per workgroup even for a small mode count (A-B / tests)          */
  SC_GEMM_NO_STREAM = 16,    /* never take the LDS-DMA streamed kernel (k_modegemm_s8): generation 1 (A-B) */
  SC_GEMM_NO_SB = 64,        /* never take the small-extent streaming kernel (k_modegemm_sb; A-B / tests)  */
  SC_GEMM_SB_WM4 = 128,      /* k_modegemm_sb: the four waves over 512 contiguous modes of one tile (A-B / tests) */
  SC_GEMM_SB_ALT_ORDER = 1 << 25, /* small-batch kernels: the OTHER work-item order (round 5; A-B / tests).  Default: k_modegemm_sb
                                walks its mode tiles slowest (the tiles of a mode tile share the small operand in one L2), the
                                one-pass backward pair k_modegemm_sb_bwd mode tiles FASTEST (neighbouring workgroups stream
                                neighbouring pieces of the same weight rows: 5.78 -> 5.54 ms per step at configs[4]) */
  SC_GEMM_NO_FMX = 1 << 24,  /* never take the matrix-core factor-matrix / mode-sum kernels (sc_kernels_fmx.h; A-B / tests) */
  /* round 8, cache policy of the streamed matrix-core kernel (k_modegemm_dma / k_modegemm_dma_bwd; other routes ignore
   * the three bits).  None of them changes a bit of C. */
  SC_GEMM_C_WT = 1 << 26,    /* C IS consumed by the next kernel: write-through stores, no dirty lines at the kernel
                                boundary (SC_GEMM_STREAM_C wins when both are set) */
  SC_GEMM_NT_A = 1 << 27,    /* the caller calls A cold (not in the caches from an earlier kernel): its operand requests are
                                non-temporal IF every piece of it has one reader in the launch (one column block, Q <= 32)
                                and the launch runs the 4-wave shape; ignored otherwise */
  SC_GEMM_NT_B = 1 << 28,    /* the same for B (one row block, P <= 32) */
  SC_GEMM_F16 = 32           /* the reference's complex-half contraction (fno_block_precision "half" / "mixed",
                              * einsum_utils.py:10-36): operands rounded to float16, four real products summed in
                              * fp32 and rounded to float16, re = t00 - t11, im = t10 + t01 rounded to float16;
                              * fp32 storage throughout.  Plain C = opA(A) opB(B) launches (no accumulate) */
};
/* flags bits 8..23: cap on the number of workgroups of the matrix-core kernel (0 = auto) */
#define SC_GEMM_GRID(n) (((n) & 0xffff) << 8)

typedef struct {
  int64_t P, Q, R, n_modes;
  int64_t a_sp, a_sr, a_sm;
  int64_t b_sr, b_sq, b_sm;
  int64_t c_sp, c_sq, c_sm;
  int32_t conj_a, conj_b;
  int32_t accumulate;       /* 0: C = ..., 1: C += ...                                     */
  int32_t flags;            /* SC_GEMM_* bits                                               */
  const int32_t* b_idx;     /* optional device table [n_modes], NULL -> m*b_sm              */
  const int32_t* c_idx;     /* optional device table [n_modes], NULL -> m*c_sm              */
  /* tiled ("mode-group-major") operands, engine-private layouts only: with a_sg != 0 mode m of A lives at element
   * offset (m / 16) * a_sg + (m % 16) (+ p*a_sp + r*a_sr), i.e. the 16 modes of a group stay contiguous and the
   * groups are a_sg apart -- e.g. [group][p][r][16] with a_sg = P*R*16, a_sp = R*16, a_sr = 16 makes everything one
   * workgroup of k_modegemm_dma reads one contiguous block.  Same for b_sg / c_sg.  0 = plain (m * sm).  Needs
   * n_modes % 16 == 0, sm == 1 and no index table; only k_modegemm_dma takes it (sc_modegemm fails otherwise). */
  int64_t a_sg, b_sg, c_sg;
} sc_modegemm_desc;

int sc_modegemm(const sc_modegemm_desc* d, const float* A, const float* B, float* C,
                void* stream);
/* Two independent contractions: sc_modegemm(d0, ...) followed by sc_modegemm(d1, ...) (no output may alias an operand
 * of the other call) -- bit-identical to those two calls whenever each of them alone runs the 4-wave streamed shape or
 * the pair runs as two launches, equal up to the rounding of the last bits otherwise (a job that alone would take the
 * 8-wave four-product shape, e.g. the weight gradient at hidden 128, runs the 4-wave three-product shape here).  The pair of a layer's backward pass -- d0 the weight gradient
 * (conj_a, autograd of spectral_convolution.py:21-46 w.r.t. the weight), d1 the gradient of the spectrum (conj_b) --
 * runs as ONE launch of k_modegemm_dma_bwd when both qualify for the streamed matrix-core kernel: the second round of
 * one job fills the tail of the other.  sc_modegemm_pair_fused: 1 if a pair with 16-byte aligned operands takes that
 * launch, 0 if it runs as two.
 * Round 3, session 2: a SMALL-BATCH pair (d0->R = d1->P <= 4 rows against weight-sized d0's C / d1's B, B0 and A1 the
 * same array; BASELINE configs[4]) runs as ONE launch of k_modegemm_sb_bwd (sc_kernels_sb.h): a single pass over the
 * weight serves both gradients (the weight is read while its gradient is written), bit-identical to the two
 * k_modegemm_sb launches it replaces; sc_layer_backward takes the same launch. */
int sc_modegemm_pair(const sc_modegemm_desc* d0, const float* A0, const float* B0, float* C0,
                     const sc_modegemm_desc* d1, const float* A1, const float* B1, float* C1, void* stream);
int sc_modegemm_pair_fused(const sc_modegemm_desc* d0, const sc_modegemm_desc* d1);
/* Which launch(es) sc_modegemm_pair issues for 16-byte aligned operands with B0 == A1 (introspection for tests and
 * profiles, like sc_modegemm_path): 2 = one launch of k_modegemm_sb_bwd, 1 = one launch of k_modegemm_dma_bwd,
 * 0 = two sc_modegemm launches. */
int sc_modegemm_pair_path(const sc_modegemm_desc* d0, const sc_modegemm_desc* d1);
/* The cache policy a sc_modegemm call with this descriptor runs with (introspection for tests, round 8): -1 when the call
 * does not take the streamed matrix-core kernel (sc_modegemm_path != 2), else bits 0-1 = store policy of C (0 plain,
 * 1 non-temporal, 2 write-through), bit 2 = A requested non-temporally, bit 3 = B requested non-temporally. */
int sc_modegemm_policy(const sc_modegemm_desc* d);
/* C[p, q] += sum_m sum_r opA(A[p, r, m]) * opB(B[r, q, m]) -- the gradient of a mode-independent
 * operand (Tucker / CP factor matrices, autograd of spectral_convolution.py:55-103): lanes run over
 * the modes, wave reduction, one atomic add per (p, q) and mode tile.  C (element offsets
 * p*c_sp + q*c_sq) must be zeroed by the caller; c_sm / c_idx / accumulate are ignored. */
int sc_modegemm_msum(const sc_modegemm_desc* d, const float* A, const float* B, float* C,
                     void* stream);
/* The same sum, C[p, q] OVERWRITTEN (no zeroing by the caller), on the matrix cores (round 3, sc_kernels_fmx.h:
 * k_modegemm_msum_mx stages [rows][64 modes] chunks of both operands in LDS and accumulates 16 x 16 tiles over all
 * chunks of a workgroup; one partial per workgroup in `workspace`, fixed-order reduction: run-to-run deterministic,
 * unlike the atomic adds of sc_modegemm_msum).  The matrix-core kernel takes problems where both operands have mode
 * stride 1, 8 <= P, Q <= 64 and n_modes >= 64 (sc_modegemm_msum_path == 1); every other problem runs the VALU kernel
 * of sc_modegemm_msum with one workspace slot per (mode split, r split) instead of atomics and the same fixed-order
 * reduction (path 0; session 2) -- so the result of this entry point is the same bits on every run for every shape.
 * sc_modegemm_msum_workspace_bytes returns the bytes needed (0 only for an empty problem or one beyond the launch grid). */
size_t sc_modegemm_msum_workspace_bytes(const sc_modegemm_desc* d);
int sc_modegemm_msum_ws(const sc_modegemm_desc* d, const float* A, const float* B, float* C, void* workspace,
                        size_t workspace_bytes, void* stream);
/* 1: sc_modegemm_msum_ws runs k_modegemm_msum_mx (matrix cores), 0: the slot form of the VALU kernel */
int sc_modegemm_msum_path(const sc_modegemm_desc* d);
/* 1 if this call runs on a matrix-core kernel, 0 for the VALU kernel */
int sc_modegemm_uses_matrix_cores(const sc_modegemm_desc* d);
/* which kernel a call with 16-byte aligned operands takes: 0 k_modegemm (VALU), 1 k_modegemm_mfma (register-staged
 * matrix-core kernel: sub-blocks through index tables, ragged ranks, factor operands), 2 k_modegemm_s8 (LDS-DMA
 * streamed matrix-core kernel: plain contiguous-mode operands, mode count a multiple of 8), 3 k_modegemm_sb (round 3:
 * small-extent streaming kernel on the vector ALUs -- a batch of <= 4 rows against a large weight, or a reduction of
 * <= 4 terms into a weight-sized result: plain contiguous-mode operands, even mode count, even row strides;
 * bit-identical to path 0), 4 k_modegemm_bfac (round 3: b_sm == 0, i.e. a mode-independent right operand -- the channel
 * factor matrices of Tucker / CP contractions -- read through the scalar cache; unit mode strides of A and C, Q >= 8;
 * bit-identical to path 0), 5 k_modegemm_bfac_mx (round 3: the same operand shape with 8 <= Q <= 64, 4 <= R <= 64 and
 * >= 64 modes on the matrix cores: chunks of 64 modes staged in LDS, 16 x 16 x 4 MFMA tiles, three real products per
 * complex product -- equal to path 0 up to the rounding of the last bits) */
int sc_modegemm_path(const sc_modegemm_desc* d);

/* out[i] = float16(in[i]) (round to nearest even), kept in fp32 storage; in == out allowed.  The cast points of
 * fno_block_precision "half" / "mixed" (spectral_convolution.py:436-437 x.half(), :451-454 x.chalf(), and the
 * float16 result of the inverse transform). */
int sc_round_f16(const float* in, float* out, int64_t n, void* stream);

/* ---- the complex32 wire of the mode-parallel layer's half-precision exchanges (fno_block_precision "half" /
 * "mixed") ----
 * spec: complex64 (interleaved fp32) [n][c][k1][rest]; wire: complex32 (two float16 words, real part in the low half)
 * in the rank-major send layout [P][n][c][rows][rest].  Global wire row w0 + r (rank (w0 + r) / rows, local row
 * (w0 + r) % rows) holds spectrum row r; w0 + k1 <= P * rows.  Values are rounded with sc_round_f16 (nearest even,
 * torch's cast).  P = 1, w0 = 0, k1 = rows: a plain complex64 <-> complex32 conversion.
 *
 * sc_wire_pack_c32: spec -> wire, every wire row outside [w0, w0 + k1) written zero.  Replaces the zero-filled
 * (n, c, P rows, rest) staging tensor, the slice copy of the kept rows into it and the chunk-major send-buffer copy of
 * the fp32 exchange (mpu.mappings.all_to_all) on the half-precision route of ModeParallelSpectralConv. */
int sc_wire_pack_c32(const float* spec, void* wire, int64_t n, int64_t c, int64_t k1, int64_t rest, int64_t P,
                     int64_t rows, int64_t w0, void* stream);

/* sc_wire_unpack_c32: wire -> spec, rows [w0, w0 + k1) of the P * rows concatenation.  Replaces the rank-order
 * concatenation copy after the fp32 exchange and the slice copy of the kept rows out of it. */
int sc_wire_unpack_c32(const void* wire, float* spec, int64_t n, int64_t c, int64_t k1, int64_t rest, int64_t P,
                       int64_t rows, int64_t w0, void* stream);

/* ---- 2-D bicubic resample of a ROW RANGE of a global grid (the skip path of the spatially decomposed layer) ----
 * resample(x, 1.0, [2, 3], output_shape) of neuralop/layers/resample.py:49-52, i.e. F.interpolate(mode="bicubic",
 * align_corners=True) of a global (h_in, w_in) grid to (h_out, w_out), evaluated on one rank's rows.  x holds the
 * global input rows [src_row0, src_row0 + rows_in) of `images` images, (images, rows_in, w_in) fp32 contiguous; y is
 * the global output rows [out_row0, out_row0 + rows_out), (images, rows_out, w_out).  ATen's arithmetic: scale =
 * (in - 1) / (out - 1) in fp32 (0 when out == 1), source index scale * dst, taps floor - 1 .. floor + 2 clamped to the
 * GLOBAL grid, cubic convolution A = -0.75.  The input rows must cover every tap of the output rows (else an error);
 * the column upsampling factor is at most ~45.
 * Backward: gx (images, rows_in, w_in) OVERWRITTEN with the adjoint of the forward applied to gy (images, rows_out,
 * w_out) -- the part of the input gradient these output rows contribute, halo rows included; deterministic gather
 * (no atomics): two runs give the same bits. */
int sc_bicubic_rows_forward(const float* x, float* y, int64_t images, int64_t rows_in, int64_t w_in, int64_t src_row0,
                            int64_t h_in, int64_t h_out, int64_t w_out, int64_t out_row0, int64_t rows_out, void* stream);
int sc_bicubic_rows_backward(const float* gy, float* gx, int64_t images, int64_t rows_in, int64_t w_in, int64_t src_row0,
                             int64_t h_in, int64_t h_out, int64_t w_out, int64_t out_row0, int64_t rows_out, void* stream);

/* ---- Legendre (latitude) stage of the real spherical-harmonic transforms ----
 * Replaces the two einsums of torch_harmonics' RealSHT / InverseRealSHT that neuralop/layers/spherical_convolution.py
 * calls through its SHT wrapper (:206-281, SphericalConv.forward :430-472):
 *   analysis   c[line, l, m] = sum_k x[line, k, m] tab[l, k, m]    x (lines, nlat, mmax), c (lines, lmax, mmax)
 *   synthesis  x[line, k, m] = sum_l c[line, l, m] tab[l, k, m]    c (lines, lmax, mmax), x (lines, nlat, mmax)
 * Operands complex64 interleaved and contiguous (x is the output of a 1-d real sc_transform_forward plan read in place,
 * resp. the input of its inverse); tab a REAL fp32 table (lmax, nlat, mmax), zero for l < m: those terms are skipped,
 * not read.  The output is overwritten in full (zeros at l < m in c).  With a real table the two calls are each
 * other's adjoint (the autograd of one is the other with the same table).  Deterministic: no atomics. */
int sc_legendre_analysis(const float* x, const float* tab, float* c, int64_t lines, int64_t nlat, int64_t lmax,
                         int64_t mmax, void* stream);
int sc_legendre_synthesis(const float* c, const float* tab, float* x, int64_t lines, int64_t nlat, int64_t lmax,
                          int64_t mmax, void* stream);

/* ---- spectral-derivative multiplier pass ----
 * The step between the two transforms of neuralop/losses/differentiation.py's FourierDiff (:1167-1345): every
 * requested derivative spectrum from ONE read of the source spectra, the multipliers formed from per-axis tables:
 *   yhat[g, t, m] = sum over terms j with term_out[j] = t of
 *                   term_coef[j] * 1/2 (prod_d A[d][term_tab[j][d]][i_d(m)] + prod_d B[d][term_tab[j][d]][i_d(m)])
 *                   * xhat[g, term_src[j], m]
 * xhat (groups, n_src, kept[0..ndim-1]) complex64 contiguous: the output of a full-spectrum SC_FWD_SCALED plan in the
 * plan's row order.  yhat element (g, t, m) lies at complex offset g * y_group_stride + t * y_out_stride + m (m the
 * flattened contiguous mode index), so the caller lays the outputs out as (n_out, groups, ..) or (groups, n_out, ..).
 * A[d], B[d]: device tables [n_tab[d]][kept[d]] complex64 in the same row order.  conj != 0 conjugates both products
 * (with a Hermitian multiplier that is the adjoint: the backward pass is this call with src / out exchanged and conj).
 * Every addressed yhat element is overwritten; an output without a term is written as zeros.  At most
 * SC_SPECOP_MAX_TERMS terms plus term-less outputs (and as many outputs): longer lists are split by the
 * caller.  8-byte alignment of xhat / yhat suffices.  Deterministic: no atomics. */
#define SC_SPECOP_MAX_TERMS 12
typedef struct {
  int32_t ndim;                               /* 1..3 mode dims                                            */
  int32_t n_src, n_out, n_terms;              /* n_src <= 3                                                */
  int32_t conj, reserved;
  int64_t kept[3];
  int64_t groups;
  int64_t y_group_stride, y_out_stride;       /* complex elements                                          */
  int32_t n_tab[3];
  int32_t term_src[SC_SPECOP_MAX_TERMS], term_out[SC_SPECOP_MAX_TERMS];
  int32_t term_tab[SC_SPECOP_MAX_TERMS][3];
  float term_coef[SC_SPECOP_MAX_TERMS];
  const float* A[3];
  const float* B[3];
} sc_specop_desc;
int sc_spectral_op(const sc_specop_desc* desc, const float* xhat, float* yhat, void* stream);

/* ---- divergence-free (Helmholtz-Hodge) spectral projection ----
 * The step between the two transforms of neuralop/layers/spectral_projection.py's
 * spectral_projection_divergence_free (:6-102): the spectra of the ndim components of a vector field times the per-mode
 * projector, which does not factor into per-axis tables.  T[d]: a REAL fp32 device table [kept[d]][2][3] in the plan's
 * row order; entry [i][s] = (kappa, keep, z) of row i for s = 0 (the mode itself) and s = 1 (its mirror -k): the
 * wavenumber the row is assigned, whether it is kept (0 / 1) and whether it is the row of the zeroed mode (0 / 1).
 *   per mode m and sign s:  K_c = kappa_{sel[c]},  w = prod_d keep_d * (1 - prod_d z_d),
 *                           G_ab = w (delta_ab - K_a K_b / (sum_c K_c^2 + eps))
 *   yhat[g, a, m] = sum_b 1/2 (G+_ab + G-_ab) xhat[g, b, m]
 * (the real multiplier under which irfftn(. rfftn(u)) equals real(ifftn(G fftn(u))) for real u).  xhat (groups, ndim,
 * kept[0..ndim-1]) complex64 contiguous; yhat element (g, a, m) lies at complex offset g * y_group_stride +
 * a * y_comp_stride + m.  yhat == xhat is allowed with the source's strides (every lane loads all of its sources
 * before its first store); buffers that overlap in any other way are not.  Every addressed yhat element is
 * overwritten.  8-byte alignment of xhat / yhat suffices.  Refused before any launch: ndim outside 2..3, sel outside
 * [0, ndim), a null pointer, a non-positive extent, a negative stride, eps <= 0.  No LDS, no atomics, fixed summation
 * order: deterministic.  At most 3 ndim + 2 roundings per real component of an output (sc_kernels_helmholtz.h). */
typedef struct {
  int32_t ndim;                               /* 2..3 mode dims = components                               */
  int32_t sel[3];                             /* the axis whose kappa component c takes                    */
  float eps;
  int32_t reserved;
  int64_t kept[3];
  int64_t groups;
  int64_t y_group_stride, y_comp_stride;      /* complex elements                                          */
  const float* T[3];
} sc_helmholtz_desc;
int sc_helmholtz_project(const sc_helmholtz_desc* desc, const float* xhat, float* yhat, void* stream);

/* ---- banded real-space operators: finite differences and the Lp / H1 data losses ----
 * neuralop/losses/differentiation.py's FiniteDiff (:11-660) is, along one axis, an N x N matrix with three interior
 * bands and (non-periodic) two one-sided boundary rows of four entries; it, its transpose and D^T D are banded with
 * half-width <= 3.  A table T[d] holds n_tab[d] such matrices of axis d as [n_tab[d]][dims[d]][7] fp32: entry o + 3 of
 * row i multiplies the neighbour i + o (o = -3..3).
 *   y[g, t, p] = scale[g] * scale_mul[0] * sum over terms j with term_out[j] = t of
 *                term_coef[j] * sum_o T[axis_j][term_tab[j]][i_axis(p)][o + 3] * s[g, term_src[j], p + o stride_axis]
 * u (groups, n_src, dims[0..ndim-1]) fp32 contiguous; s = u, or u - u2 where u2 (same shape) is given.  term_axis -1 is
 * the identity, term_coef * s[p].  scale ([groups]) and scale_mul ([1]) are optional device pointers.  y element
 * (g, t, p) lies at float offset g * y_group_stride + t * y_out_stride + p.  On a periodic axis neighbour indices wrap
 * modulo dims[d] (any extent >= 1: the caller puts every matrix entry into exactly one tap); on a non-periodic axis
 * (extent >= 4) a neighbour outside the line must have a zero table entry -- its address is clamped into the line, never
 * read outside the buffer.  Every addressed y element is overwritten, an output without a term with zeros.  At most
 * SC_BAND_MAX_TERMS terms plus term-less outputs, n_src <= 3, n_out <= 3.  Deterministic: no atomics. */
#define SC_BAND_MAX_TERMS 12
typedef struct {
  int32_t ndim;                               /* 1..3                                                       */
  int32_t n_src, n_out, n_terms;
  int64_t dims[3];
  int32_t periodic[3];
  int32_t reserved;
  int64_t groups;
  int64_t y_group_stride, y_out_stride;       /* floats                                                     */
  int32_t n_tab[3];
  int32_t term_src[SC_BAND_MAX_TERMS], term_out[SC_BAND_MAX_TERMS];
  int32_t term_axis[SC_BAND_MAX_TERMS], term_tab[SC_BAND_MAX_TERMS];
  float term_coef[SC_BAND_MAX_TERMS];
  const float* T[3];
  const float* scale;
  const float* scale_mul;
} sc_band_desc;
int sc_band_apply(const sc_band_desc* desc, const float* u, const float* u2, float* y, void* stream);

/* The reductions of LpLoss / H1Loss (neuralop/losses/data_losses.py:21-491) over x, y (lines, dims..) fp32 contiguous,
 * two launches.  Stage 1 writes per (line, chunk) the partial sums
 *   h1 != 0:  num = sum_p [e^2 + sum_d (D_d e)^2],  den = sum_p [y^2 + sum_d (D_d y)^2],  e = x - y, D_d = T[d] ([dims[d]][7])
 *   h1 == 0:  num = sum |e|^p,  den = sum |y|^p   (integer p >= 1; dims only give the point count)
 * into ws ([lines][chunks][2] floats, sc_sobolev_workspace_bytes); a line is split over as many workgroups as fill the
 * device (chunks != 0 in the descriptor asks for about that many).  Stage 2 (one workgroup) sums the chunks in a fixed
 * order and writes per line v_l, dv[l] = factor * dv_l / dnum_l and loss[0] = factor * sum_l v_l, factor = 1 or 1 / lines:
 *   relative == 0:  v = konst num, its p-th root with take_root (never for p = 1)
 *   relative != 0:  v = num^(1/p) / (den^(1/p) + eps) with take_root (and p != 1), else num / (den + eps)
 * H1 is p = 2.  sc_lp_grad: gx[l, i] = dv[l] * gout[0] * p |e_i|^(p-1) sign(e_i) (the H1 gradient is one sc_band_apply
 * with the D^T D tables, sources x, y, scale = dv, scale_mul = gout).  Deterministic: no atomics. */
typedef struct {
  int32_t ndim;                               /* 1..3                                                       */
  int32_t h1, p, relative, take_root, reduce_mean;
  int32_t chunks;                             /* 0: chosen by the engine                                    */
  int32_t periodic[3];
  int64_t dims[3];
  int64_t lines;
  double konst, eps;
  const float* T[3];                          /* h1: D of each axis                                         */
} sc_sobolev_desc;
size_t sc_sobolev_workspace_bytes(const sc_sobolev_desc* desc);
int sc_sobolev_sums(const sc_sobolev_desc* desc, const float* x, const float* y, float* ws, size_t ws_bytes, float* v,
                    float* dv, float* loss, void* stream);
int sc_lp_grad(const sc_sobolev_desc* desc, const float* x, const float* y, const float* dv, const float* gout,
               float* gx, void* stream);

/* ---- graph neural operator layer: radius search, CSR transpose, fused kernel integral, first layer by point ----
 * All arrays contiguous; coordinates and features fp32, neighbour indices and splits int64 (the reference's dtypes).
 * Every entry point refuses a bad descriptor before any launch (d outside 1..3, negative counts, null pointers,
 * n_splits != rows + 1); m == 0, n == 0 or no edges are valid and launch nothing (owed outputs are zero-filled).
 * Every index read from a caller's array is range-checked on the device before it addresses memory.  No float atomics:
 * every sum runs in a fixed order.
 *
 * Fixed-radius search (neuralop/layers/neighbor_search.py:84-119, native_neighbor_search: the dense cdist, the two
 * where(), nonzero() and the cumsum): data (n, d), queries (m, d), d = 1..3.  A pair is kept iff d2 <= r2, d2 =
 * sum_k (q_k - p_k)^2 in fp32 in dimension order, r2 = (float)(radius * radius) formed in double; zero distances are
 * kept (:104-107).  sc_radius_count writes deg[m] and row_splits[m + 1] (exclusive scan); the caller reads
 * row_splits[m] -- ONE 8-byte copy, where the reference's nonzero() synchronises too -- to size the outputs of
 * sc_radius_fill: index[n_edges], each query's neighbours in ascending data index (the nonzero() order), and with
 * return_norm weights[n_edges] = d2, or 1e-14 where d2 == 0 (:105-111). */
typedef struct {
  int32_t d, return_norm;
  int64_t n, m;
  double radius;
} sc_radius_desc;
int sc_radius_count(const sc_radius_desc* desc, const float* data, const float* queries, int32_t* deg,
                    int64_t* row_splits, void* stream);
int sc_radius_fill(const sc_radius_desc* desc, const float* data, const float* queries, const int64_t* row_splits,
                   int64_t n_edges, int64_t* index, float* weights, void* stream);

/* The same search over a uniform grid of cells at least radius wide: the data points are binned on the device (bounds,
 * cell histogram, scan, slot scatter into cell order) and a query is tested against the points of its own and the
 * adjacent cells only.  Same descriptor, same refusals, and the SAME BYTES out as the two calls above for every input:
 * the hit test is the same fp32 expression, and each row is ranked into ascending data index.  The grid lives in ws
 * (sc_radius_grid_workspace_bytes: a function of the descriptor alone, 0 for a bad one); a short or null workspace is
 * refused before any launch.  sc_radius_grid_count builds the grid and counts; sc_radius_grid_fill reuses the grid
 * the count pass left in the same ws.  The host reads nothing but row_splits[m]. */
size_t sc_radius_grid_workspace_bytes(const sc_radius_desc* desc);
int sc_radius_grid_count(const sc_radius_desc* desc, const float* data, const float* queries, int32_t* deg,
                         int64_t* row_splits, void* ws, size_t ws_bytes, void* stream);
int sc_radius_grid_fill(const sc_radius_desc* desc, const float* data, const float* queries, const int64_t* row_splits,
                        int64_t n_edges, int64_t* index, float* weights, void* ws, size_t ws_bytes, void* stream);

/* Transpose of any valid CSR graph (rows, cols, n_edges; the backward pass of integral_transform.py:167 f_y[:, idx]):
 * col_splits[cols + 1], perm[n_edges] = edge ids grouped by column, ascending within each group, row_of_edge[n_edges].
 * Integer atomics build a histogram and fill slots; one wave per column then ranks its slice, so the output does not
 * depend on their order.  ws: sc_csr_transpose_workspace_bytes. */
typedef struct {
  int64_t rows, cols, n_edges;
  int64_t n_splits;                           /* entries of row_splits: must be rows + 1                    */
} sc_csr_desc;
size_t sc_csr_transpose_workspace_bytes(const sc_csr_desc* desc);
int sc_csr_transpose(const sc_csr_desc* desc, const int64_t* row_splits, const int64_t* index, int64_t* col_splits,
                     int32_t* perm, int32_t* row_of_edge, void* ws, size_t ws_bytes, void* stream);

/* The fused kernel integral (integral_transform.py:167 gather, :198 mul_(in_features), :211 mul_(nbr_weights), :221
 * segment_csr; segment_csr.py:63-98):
 *   out[b, i, c] = s_i sum_{k in [splits[i], splits[i+1])} K[(b,) e, c] F[b, row(e), c] w[e] t(e),   e = perm[k] or k
 * s_i = 1, or 1 / (segment length) with mean (an empty segment gives 0); F (b, n_f, c) and w [n_edges] optional;
 * row(e) = gather64[e], gather32[e] or e; t(e) = 1 / (scale_splits[r + 1] - scale_splits[r]), r = gather32[e], where
 * scale_splits is given (the mean of the ORIGINAL rows inside a transposed sum).  K (b, n_edges, c) or, with
 * k_batch_stride 0, (n_edges, c); strides in floats.  One wave per (b, i) walks its segment in order.
 * sc_csr_edge_grad, over the graph's own rows (no perm, no scale_splits):
 *   gK[(b,) e, c] = s_i w[e] g[b, i, c] F[b, row(e), c],   summed over b inside the kernel when k_batch_stride is 0. */
typedef struct {
  int64_t rows, n_splits, n_edges;
  int64_t n_f, n_scale_rows;
  int64_t k_batch_stride, f_batch_stride;
  int32_t channels, batch, mean, reserved;
  const int64_t* splits;
  const int32_t* perm;
  const int64_t* gather64;
  const int32_t* gather32;
  const int64_t* scale_splits;
  const float* w;
} sc_csr_reduce_desc;
int sc_csr_reduce(const sc_csr_reduce_desc* desc, const float* K, const float* F, float* out, void* stream);
int sc_csr_edge_grad(const sc_csr_reduce_desc* desc, const float* g, const float* F, float* gK, void* stream);

/* The first Linear of the kernel MLP by point instead of by edge (integral_transform.py:158-191: y[idx],
 * repeat_interleave(x), the cat and fcs[0] of LinearChannelMLP, channel_mlp.py):
 *   H[(b,) e, c] = act(Py[(b,) index[e], c] + Px[row(e), c] + bias[c]),   act = identity or GELU (erf)
 * Py (b, n_py, c) or, with py_batch_stride 0, (n_py, c); Px (rows, c); H (batch, n_edges, c).  sc_edge_lift_bwd
 * recomputes the pre-activation and writes gPre = gH act'(pre) in H's layout. */
#define SC_LIFT_IDENTITY 0
#define SC_LIFT_GELU 1
typedef struct {
  int64_t rows, n_splits, n_edges, n_py;
  int64_t py_batch_stride;
  int32_t channels, batch, act, reserved;
  const int64_t* splits;
  const int64_t* index;
} sc_edge_lift_desc;
int sc_edge_lift(const sc_edge_lift_desc* desc, const float* Py, const float* Px, const float* bias, float* H,
                 void* stream);
int sc_edge_lift_bwd(const sc_edge_lift_desc* desc, const float* Py, const float* Px, const float* bias,
                     const float* gH, float* gPre, void* stream);

/* The whole kernel MLP over CHUNKS of edges (LinearChannelMLP with GELU of n_layers >= 2 Linear layers, channel_mlp.py):
 *   h_0 = gelu(Py[(b,) index[e]] + Px[row(e)] + bias0)            widths[0] channels, never stored for all edges
 *   h_l = gelu(h_{l-1} W_l^T + b_l), l = 1 .. n_layers - 2        W_l (widths[l], widths[l-1]) row-major
 *   K[(b,) e] = h_{L-2} W_{L-1}^T + b_{L-1}                        widths[L-1] channels
 * W / b / gW / gb are HOST arrays of n_layers - 1 device pointers (entry l - 1 belongs to layer l; a null b entry means
 * no bias, a null gW / gb entry not wanted).  One call walks the edges in chunks of chunk_edges (a multiple of
 * SC_EDGE_MLP_TILE; 0 = the default) with stream-ordered launches and no host wait; the workspace of
 * sc_edge_mlp_workspace_bytes(desc) depends on widths, batch and chunk_edges alone, not on n_edges.
 * sc_edge_mlp_backward recomputes the chain per chunk and ADDS each chunk's share into gPy ((b,) n_py, widths[0]), gPx
 * (rows, widths[0]), gW_l and gb_l, which it zero-fills first; it needs col_splits / perm of sc_csr_transpose when gPy
 * is wanted.  row(e) is found by a binary search in splits; row_of_edge is accepted and not read.  An index[e] outside
 * [0, n_py) gives h_0 = 0 for that edge and no gradient.  Deterministic: no float atomics, fixed-order sums.
 * Refused before any launch: n_layers outside 2 .. 8, a width outside 1 .. 512, a chunk_edges that is no multiple of the
 * tile, a workspace that is too small, a null pointer.  n_edges = 0: no launch (backward: the zero gradients alone). */
#define SC_EDGE_MLP_MAX_LAYERS 8
#define SC_EDGE_MLP_MAX_WIDTH 512
#define SC_EDGE_MLP_TILE 128
typedef struct {
  int64_t rows, n_splits, n_edges, n_py;
  int64_t py_batch_stride;     /* floats; 0: Py (n_py, c) and batch = 1 */
  int64_t chunk_edges;
  int32_t batch, n_layers;
  int32_t widths[SC_EDGE_MLP_MAX_LAYERS];
  const int64_t* splits;
  const int64_t* index;
  const int32_t* row_of_edge;  /* optional */
  const int64_t* col_splits;   /* backward */
  const int32_t* perm;         /* backward */
} sc_edge_mlp_desc;
size_t sc_edge_mlp_workspace_bytes(const sc_edge_mlp_desc* desc);
int sc_edge_mlp_forward(const sc_edge_mlp_desc* desc, const float* Py, const float* Px, const float* bias0,
                        const float* const* W, const float* const* b, float* K, void* ws, size_t ws_bytes,
                        void* stream);
int sc_edge_mlp_backward(const sc_edge_mlp_desc* desc, const float* Py, const float* Px, const float* bias0,
                         const float* const* W, const float* const* b, const float* gK, float* gPy, float* gPx,
                         float* const* gW, float* const* gb, void* ws, size_t ws_bytes, void* stream);

/* ---- finite-difference convolution of the local neural operator (neuralop/layers/differential_conv.py:6-101) ----
 *   y = (conv_pad(x, W) - conv_1x1(x, sum_taps W)) * inv_h
 * as ONE convolution with folded weights: W'[.., t] = W[.., t] inv_h off the centre, W'[.., centre] = -(sum of the other
 * taps) inv_h.  x (batch, c_in, dims[0..ndim-1]), W (c_out, c_in / groups, k..k), y (batch, c_out, dims..), all fp32
 * contiguous; k in {3, 5, 7}; padding as below (the reference's periodic / zeros / replicate / reflect).
 * sc_fdconv_backward writes gx (like x), gw (like W; its centre tap is exactly 0), or both -- a null pointer means not
 * wanted: gx is the adjoint of padding followed by the convolution, gw[.., t] = (G[.., t] - G[.., centre]) inv_h with
 * G[o, c, t] = sum_{b, p} gout[b, o, p] xpad[b, c, p + t].  x may be null when gw is, w when gx is.
 * The backward call needs sc_fdconv_workspace_bytes(desc) bytes (the folded weights, the partial sums of gw, the padded
 * data gradient of replicate / reflect), the forward call sc_fdconv_forward_workspace_bytes(desc) (the folded weights
 * alone; a workspace of the larger size serves both).  Refused before any launch: an even k, k outside 3..7, groups that do not divide both
 * channel counts, reflect with an extent <= k / 2, periodic with an extent < k / 2, a null pointer, a small workspace.
 * sc_fdconv_path: the route a descriptor takes (0 = refused) -- SC_FDCONV_PATH_MFMA for groups = 1, ndim = 2, k = 3,
 * c_in, c_out in {32, 64, 128}, periodic or zeros (implicit GEMM on the exact-fp32 matrix instruction), the vector-ALU
 * route otherwise.  Deterministic: no float atomics, every sum in a fixed order that depends on the descriptor alone. */
#define SC_FDCONV_PERIODIC 0
#define SC_FDCONV_ZEROS 1
#define SC_FDCONV_REPLICATE 2
#define SC_FDCONV_REFLECT 3
#define SC_FDCONV_PATH_GENERAL 1
#define SC_FDCONV_PATH_MFMA 2
typedef struct {
  int32_t ndim, k, padding, groups;
  int64_t dims[3];
  int64_t batch, c_in, c_out;
  float inv_h;
  int32_t reserved;
} sc_fdconv_desc;
int sc_fdconv_path(const sc_fdconv_desc* desc);
size_t sc_fdconv_workspace_bytes(const sc_fdconv_desc* desc);
size_t sc_fdconv_forward_workspace_bytes(const sc_fdconv_desc* desc);
int sc_fdconv_forward(const sc_fdconv_desc* desc, const float* x, const float* w, float* y, void* workspace,
                      size_t workspace_bytes, void* stream);
int sc_fdconv_backward(const sc_fdconv_desc* desc, const float* x, const float* w, const float* gout, float* gx,
                       float* gw, void* workspace, size_t workspace_bytes, void* stream);

/* ---- equidistant discrete-continuous (DISCO) convolution of the local neural operator ----------------------------
 * (neuralop/layers/discrete_continuous_convolution.py: EquidistantDiscreteContinuousConv2d and ...ConvTranspose2d)
 *   kernel[o, c, i, j] = q_weight sum_k psi[k, i, j] weight[o, c, k]
 *   transposed = 0:  y = conv2d(x, kernel, bias, stride (sh, sw), padding (pad_h, pad_w), groups), zero padding
 *   transposed = 1:  y = conv_transpose2d(x, kernel, bias, stride, padding, output_padding (opad_h, opad_w), groups)
 * x (batch, c_in, h_in, w_in), y (batch, c_out, h_out, w_out), psi (basis, ph, pw) -- the layer's filter buffer with its
 * two spatial axes swapped and both flipped, contiguous --, bias (c_out) or null, all fp32 contiguous.  weight is
 * (c_out, c_in / groups, basis) for transposed = 0 and (c_in, c_out / groups, basis) for transposed = 1.
 * sc_disco_backward writes gx, gw, gbias or any subset (null = not wanted); gw is the weight-gradient correlation
 * projected onto the basis, gbias the sum of gout over batch and points.  x may be null when gw is, weight when gx is.
 * Workspaces as for sc_fdconv_*.  Refused before any launch: output extents that do not follow from the other fields
 * (conv2d's / conv_transpose2d's own formula), groups that do not divide both channel counts, a support outside 1..15 or
 * a stride outside 1..4 per axis, padding outside 0..support - 1, output padding outside 0..stride - 1 (0 for
 * transposed = 0), a null required pointer, a small workspace, extents whose offsets leave the index types.
 * sc_disco_path (0 = refused): SC_DISCO_PATH_MFMA for stride 1, support 3 x 3, padding 1, groups 1, c_in, c_out in
 * {32, 64, 128} (the implicit GEMM of sc_fdconv on the exact-fp32 matrix instruction), the vector-ALU route otherwise.
 * Deterministic: no float atomics, every sum in a fixed order that depends on the descriptor alone. */
#define SC_DISCO_PATH_GENERAL 1
#define SC_DISCO_PATH_MFMA 2
typedef struct {
  int64_t batch, c_in, c_out;
  int64_t h_in, w_in, h_out, w_out;
  int32_t groups, basis;
  int32_t ph, pw, sh, sw, pad_h, pad_w, opad_h, opad_w;
  int32_t transposed;
  float q_weight;
} sc_disco_desc;
int sc_disco_path(const sc_disco_desc* desc);
size_t sc_disco_workspace_bytes(const sc_disco_desc* desc);
size_t sc_disco_forward_workspace_bytes(const sc_disco_desc* desc);
int sc_disco_forward(const sc_disco_desc* desc, const float* x, const float* weight, const float* psi,
                     const float* bias, float* y, void* workspace, size_t workspace_bytes, void* stream);
int sc_disco_backward(const sc_disco_desc* desc, const float* x, const float* weight, const float* psi,
                      const float* gout, float* gx, float* gw, float* gbias, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- discrete-continuous (DISCO) convolution on point clouds --------------------------------------------------------
 * (neuralop/layers/discrete_continuous_convolution.py: DiscreteContinuousConv2d and DiscreteContinuousConvTranspose2d;
 * the two differ only in how Psi is built)
 *   Z[b, c, k, o]         = sum_i Psi[k, o, i] q[i] x[b, c, i]
 *   out[b, g og + oc, o]  = sum_{c < cg, k} Z[b, g cg + c, k, o] weight[g og + oc, c, k] + bias[g og + oc]
 * x (batch, c_in, n_in), out (batch, c_out, n_out), q (n_in), weight (c_out, c_in / groups, basis), bias (c_out) or null,
 * all fp32 contiguous.  Psi comes as two CSR matrices with int32 splits and columns and fp32 values, nnz entries each:
 *   forward CSR     rows = n_out basis, row o basis + k holds the input points i of (k, o, .) -- sc_dsparse_forward
 *   transposed CSR  rows = n_in, row i holds the columns o basis + k of (k, o, i)             -- sc_dsparse_backward
 * Entries are summed in stored order; a column outside its range counts as zero and is never used as an address.
 * sc_dsparse_forward also writes z, (n_out, batch, basis, c_in) fp32: the engine's layout of Z, which
 * sc_dsparse_backward reads for gw.  sc_dsparse_backward writes gx, gw, gbias or any subset (null = not wanted); psi_t,
 * q and weight may be null when gx is, z when gw is.  The forward call needs sc_dsparse_forward_workspace_bytes(desc),
 * the backward call sc_dsparse_workspace_bytes(desc).  Refused before any launch: groups that do not divide both
 * channel counts, n_out basis, n_in or nnz beyond int32, a CSR whose rows or nnz differ from the descriptor's, a null
 * required pointer, a small workspace.  Neither call reads device memory on the host or waits for the device.
 * sc_dsparse_path (0 = refused): SC_DSPARSE_PATH_MFMA for groups = 1 and c_in, c_out in {32, 64, 128} (the two
 * contractions and the weight gradient as tiled GEMMs on the exact-fp32 matrix instruction), SC_DSPARSE_PATH_GENERAL,
 * the vector-ALU contraction, for every other descriptor.
 * Deterministic: no float atomics, every sum in an order that depends on the descriptor and the CSR alone. */
#define SC_DSPARSE_PATH_GENERAL 1
#define SC_DSPARSE_PATH_MFMA 2
typedef struct {
  int64_t batch, c_in, c_out;
  int64_t n_in, n_out, nnz;
  int32_t groups, basis;
} sc_dsparse_desc;
typedef struct {
  const int32_t* splits;   /* [rows + 1] */
  const int32_t* cols;     /* [nnz] */
  const float* vals;       /* [nnz] */
  int64_t rows, nnz;
} sc_dsparse_csr;
int sc_dsparse_path(const sc_dsparse_desc* desc);
size_t sc_dsparse_workspace_bytes(const sc_dsparse_desc* desc);
size_t sc_dsparse_forward_workspace_bytes(const sc_dsparse_desc* desc);
int sc_dsparse_forward(const sc_dsparse_desc* desc, const sc_dsparse_csr* psi, const float* x, const float* q,
                       const float* weight, const float* bias, float* out, float* z, void* workspace,
                       size_t workspace_bytes, void* stream);
int sc_dsparse_backward(const sc_dsparse_desc* desc, const sc_dsparse_csr* psi_t, const float* q, const float* weight,
                        const float* z, const float* gout, float* gx, float* gw, float* gbias, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- attention kernel integral ---------------------------------------------------------------------------------------
 * (neuralop/layers/attention_kernel_integral.py: AttentionKernelIntegral, associative form, with the rotary embedding
 * of layers/embeddings.py RotaryEmbedding2D), on the raw outputs of the three projections in their own layout:
 *   kn = LN(k), vn = LN(v)       per point and head over the head_dim channels (biased variance, eps 1e-5, no affine)
 *   dots[b, h]  = sum_n (R(pos_src[b, n]) kn[b, n, h])^T vn[b, n, h]                          (head_dim x head_dim)
 *   u[b, n, h]  = ((R(pos_qry[b, n]) q[b, n, h]) dots[b, h]) w[b, n]
 * q, u (batch, n_qry, heads head_dim), k, v (batch, n_src, heads head_dim), dots (batch, heads, head_dim, head_dim),
 * pos_src (batch, n_src, rotary), pos_qry (batch, n_qry, rotary), weights (batch, n_qry), all fp32 contiguous.
 * w = 1 / n_src without weights, else weights[b, n] of the QUERY row (the reference's broadcast).  rotary = 0: R = 1 and
 * the positions and inv_freq may be null.  rotary = 1: channel i pairs with i + head_dim / 2 and inv_freq has
 * head_dim / 2 entries.  rotary = 2: the channels split into halves for the two coordinates, channel i of a half pairs
 * with i + head_dim / 4, inv_freq has head_dim / 4 entries.  The angle is (coordinate rot_scale) inv_freq[i] in fp32,
 * rot_scale = fl32(scale / min_freq) of the module; a pair (x1, x2) becomes (x1 cos - x2 sin, x2 cos + x1 sin).
 * sc_attn_forward writes u and dots; sc_attn_backward reads dots again and recomputes everything else from q, k, v: it
 * writes gq, gk, gv or any subset (null = not wanted; dots may be null when gq is, q, k, v, pos_src when gk and gv are).
 * Both calls take sc_attn_workspace_bytes(desc).  Refused before any launch: a head_dim that is odd or outside 2..128,
 * rotary = 2 with head_dim % 4, n_src, n_qry or batch n heads head_dim beyond int32, batch heads >= 65536, a null
 * required pointer, a small workspace.  n_qry != n_src is legal here.  Neither call reads device memory on the host or
 * waits for the device.  sc_attn_path (0 = refused): SC_ATTN_PATH_MFMA for head_dim in {32, 64, 128} (the products with
 * the head_dim x head_dim matrices, forward and backward, on the exact-fp32 matrix instruction with points as the K
 * dimension), SC_ATTN_PATH_VECTOR, the vector-ALU kernels, for every other even head_dim.
 * Deterministic: no float atomics; the sums over points run in ascending order within chunks of 256 points, the chunks
 * are added in chunk order. */
#define SC_ATTN_PATH_VECTOR 1
#define SC_ATTN_PATH_MFMA 2
typedef struct {
  int64_t batch, n_src, n_qry;
  int32_t heads, head_dim, rotary, has_weights;
} sc_attn_desc;
int sc_attn_path(const sc_attn_desc* desc);
size_t sc_attn_workspace_bytes(const sc_attn_desc* desc);
int sc_attn_forward(const sc_attn_desc* desc, const float* q, const float* k, const float* v, const float* pos_src,
                    const float* pos_qry, const float* inv_freq, float rot_scale, const float* weights, float* u,
                    float* dots, void* workspace, size_t workspace_bytes, void* stream);
int sc_attn_backward(const sc_attn_desc* desc, const float* q, const float* k, const float* v, const float* pos_src,
                     const float* pos_qry, const float* inv_freq, float rot_scale, const float* weights,
                     const float* dots, const float* gout, float* gq, float* gk, float* gv, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- finite differences on a point cloud -----------------------------------------------------------------------------
 * (neuralop/losses/differentiation.py:728-855, get_non_uniform_fd_weights / non_uniform_fd.)  All arrays contiguous,
 * coordinates, weights and values fp32, indices and splits int64.  None of the four calls needs a workspace, reads
 * device memory on the host or waits for the device; no float atomics, every sum runs in a fixed order.
 *
 * sc_knn: the k nearest data points (n, d) of every query (m, d), d = 1..3, 3 <= k <= min(32, n), by brute force:
 * index[m, k] and d2[m, k] in ascending (d2, data index), d2 = sum_i (q_i - p_i)^2 in fp32 in dimension order (the
 * expression of sc_radius_count; a NaN counts as +inf).  The order is total: two launches give the same bits.
 *
 * sc_nufd_weights: per point the minimum-norm solution of A w = e_{deriv + 1}, which is what the reference's lstsq
 * returns: row 0 of the (d + 1) x k matrix A is ones, row i + 1 the differences of coordinate i to the point's own,
 * the columns of masked neighbours are zero.  A neighbour is masked where has_radius and d2 > (float)(radius radius)
 * (formed in double), except the first three, and where its index lies outside [0, n).  w = A^T (A A^T + lambda I)^-1 e,
 * formed and solved by Cholesky in float64 and rounded to fp32 into weights[n, n_deriv, k]; lambda = 0, or 1e-6 for the
 * reference's regularize_lstsq (the same w as its (A^T A + lambda I) w = A^T e).  A point whose Cholesky meets a pivot
 * that is not above 2^-40 trace(A A^T + lambda I) -- collinear or coincident neighbours -- is ill-posed: all its weights
 * are 0 and flag[n] is 1 (0 elsewhere); the reference returns an rcond-dependent truncated solution there.
 *
 * sc_nufd_apply:         out[j, b, p] = sum_m weights[p, j, m] values[b, index[p, m]]        values (batch, n)
 * sc_nufd_apply_adjoint: gvalues[b, q] = sum_{(p, m): index[p, m] = q} sum_j weights[p, j, m] gout[j, b, p]
 * both in fp32 with fmaf, the first in neighbour order, the second over col_splits / perm of sc_csr_transpose of the
 * stencil (rows = cols = n, row_splits = k arange(n + 1)) in ascending entry id.  Every index read from an array is
 * range-checked on the device before it addresses memory.
 * Refused before any launch: d outside 1..3, k outside 3..32 (knn), k > n (knn), k < d + 1 (weights), more than 8
 * derivatives or one outside [0, d), a radius with d = 3 (the three neighbours always kept are fewer than d + 1), a
 * negative radius or lambda, batch outside 1..65535, counts beyond int32, null pointers.  n = 0 (m = 0) launches
 * nothing.  sc_nufd_apply and its adjoint read n, k, n_deriv and batch of the descriptor only. */
typedef struct {
  int32_t d, k;
  int64_t n, m;
} sc_knn_desc;
typedef struct {
  int64_t n;
  int32_t d, k, n_deriv, batch;
  int32_t deriv[8];
  int32_t has_radius, reserved;
  double radius, lambda;
} sc_nufd_desc;
int sc_knn(const sc_knn_desc* desc, const float* data, const float* queries, int64_t* index, float* d2, void* stream);
int sc_nufd_weights(const sc_nufd_desc* desc, const float* points, const int64_t* index, const float* d2,
                    float* weights, int32_t* flag, void* stream);
int sc_nufd_apply(const sc_nufd_desc* desc, const float* weights, const int64_t* index, const float* values, float* out,
                  void* stream);
int sc_nufd_apply_adjoint(const sc_nufd_desc* desc, const float* weights, const int64_t* col_splits,
                          const int32_t* perm, const float* gout, float* gvalues, void* stream);

/* gbias[c] = sum_b Re(ghat[b, c, dc]) -- the bias gradient read off the DC coefficient of
 * the already-computed SC_FWD_ADJ_C2R spectrum (autograd of :567-568). */
int sc_bias_grad(const sc_plan* plan, const float* ghat, int64_t batch, int64_t channels,
                 float* gbias, void* stream);

/* ---- batch-independent part of the 2-D Tucker contraction (TFNO) in one launch each way --------------------
 *   t[fg, x, y] = sum_{c, d} core[fg, c, d] ux[x, c] uy[y, d]
 * (_contract_tucker, neuralop/layers/spectral_convolution.py:76-103: the two mode factors absorbed into the core; fg =
 * the (in-rank, out-rank) pairs).  All arrays complex64 interleaved, contiguous: core (fg, rx, ry), ux (mx, rx),
 * uy (my, ry), t (fg, mx, my).  Backward: gcore / gux / guy overwritten, workspace sc_tucker_modes_workspace_bytes(d).
 * Limits: mx, my, rx, ry <= 64, my ry <= 1024 (sc_tucker_modes_supported; callers fall back to sc_modegemm).
 * sc_tucker_modes_path: which kernels the two calls launch (the launches switch on the same decision): 0 = unsupported,
 * 1 = the vector kernels k_tucker_modes_fwd / _bwd (the padded layout of the matrix-core kernels passes 150 KB of LDS),
 * else 10 f + b: f = 1..4 for k_tucker_modes_fwd_mx<4, 3>, <4, 4>, <16, 3>, <16, 4>, b = 1 for
 * k_tucker_modes_bwd_mx<3, 9, 3, 3, 2>, 2 for <16, 16, 4, 4, 4>. */
typedef struct sc_tucker_desc {
  int64_t fg, rx, ry, mx, my;
} sc_tucker_desc;
int sc_tucker_modes_supported(const sc_tucker_desc* d);
int sc_tucker_modes_path(const sc_tucker_desc* d);
int sc_tucker_modes_forward(const sc_tucker_desc* d, const float* core, const float* ux, const float* uy, float* t,
                            void* stream);
size_t sc_tucker_modes_workspace_bytes(const sc_tucker_desc* d);
int sc_tucker_modes_backward(const sc_tucker_desc* d, const float* core, const float* ux, const float* uy,
                             const float* gt, float* gcore, float* gux, float* guy, void* workspace, void* stream);

/* ---- activation side of the factorized Tucker contraction, ONE call each way (round 3, session 2) -----------------
 *   z[b, f, m] = sum_i xhat[b, i, m] u_in[i, f];   t[b, g, m] = sum_f z[b, f, m] t3[f, g, m];
 *   yhat[b, o, m] = sum_g t[b, g, m] u_out[o, g]
 * -- the pairwise order of _contract_tucker's einsum 'abcd,fghi,bf,eg,ch,di->aecd' (neuralop/layers/
 * spectral_convolution.py:76-103; t3 = the core with the mode factors absorbed, sc_tucker_modes_forward) and the six
 * products of its autograd.  The launches are exactly those of the corresponding sc_modegemm / sc_modegemm_msum_ws
 * calls (same kernels, same bits); the point is the HOST: a factorized layer step issued call by call from Python
 * costs 0.6-0.76 ms of host time for 0.76 ms of device time (profiles/r03s2_tfno_host.txt), one call per direction
 * takes the 9 products off the interpreter.  All arrays complex64 interleaved, contiguous: xhat (B, Cin, M),
 * u_in (Cin, R1), t3 (R1, R2, M), u_out (Cout, R2), z (B, R1, M), t (B, R2, M), yhat (B, Cout, M).
 * Backward: gy (B, Cout, M) in; gxhat (B, Cin, M), gu_in (Cin, R1), gt3 (R1, R2, M), gu_out (Cout, R2) overwritten
 * (a null pointer skips that gradient); workspace: sc_tucker_chain_workspace_bytes (holds gt, gz and the partial
 * sums of the two factor gradients).
 * The backward call uses TWO streams (session 2): gt, gt3, gxhat on `stream`, the factor gradients and gz on a
 * non-blocking stream the engine owns, forked from and joined back into `stream` with events (no host
 * synchronisation; records into a hipGraph as a fork / join): everything the call issued is complete, in `stream`'s
 * order, when work issued to `stream` afterwards runs.  The launches are latency-bound and only partly dependent; side
 * by side the six take 146 instead of 193 us under the profiler, 0.735 -> 0.721 ms per TFNO step
 * (profiles/r03s2_tfno_two_streams_ab.txt, _timeline.txt).  Same kernels, same bits.  SC_NO_SIDE_STREAM=1
 * (environment) keeps every launch on `stream`. */
typedef struct sc_tucker_chain_desc {
  int64_t batch, c_in, c_out, r_in, r_out, n_modes;
} sc_tucker_chain_desc;
int sc_tucker_chain_forward(const sc_tucker_chain_desc* d, const float* xhat, const float* u_in, const float* t3,
                            const float* u_out, float* z, float* t, float* yhat, void* stream);
size_t sc_tucker_chain_workspace_bytes(const sc_tucker_chain_desc* d);
int sc_tucker_chain_backward(const sc_tucker_chain_desc* d, const float* xhat, const float* u_in, const float* t3,
                             const float* u_out, const float* z, const float* t, const float* gy, float* gxhat,
                             float* gu_in, float* gt3, float* gu_out, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---- the same nine products as ONE kernel launch each way (round 5, csrc/sc_kernels_tkchain.h) -----------------------
 * Replaces the three einsum steps of _contract_tucker's pairwise order and their autograd
 * (neuralop/layers/spectral_convolution.py:76-103) for shapes inside sc_tucker_chain_fused_supported: batch <= 32,
 * channels <= 64, ranks <= 48, every extent and the number of modes a multiple of 4 (BASELINE configs[2]: 32 x 64 -> 64
 * channels, ranks 36, 2112 modes).  A workgroup owns four modes for the whole batch and walks x̂ -> z -> t -> ŷ
 * (backward: ĝ -> gt -> gz -> gx̂ with the factor gradients accumulated per workgroup and reduced in fixed order) out of
 * LDS; z and t are written once for the backward pass and never re-read by the forward call.
 *   t3m: a mode-major copy of t3, (n_modes, r_in, r_out) complex64 = sc_tucker_chain_t3m_bytes -- WRITTEN by the forward
 *        call (one transposing launch) and READ by the backward call: the caller keeps it between the two.
 *   backward workspace: sc_tucker_chain_backward_fused_workspace_bytes (the mode-major gradient of t3 + one partial
 *        sum of both factor gradients per workgroup).  gt3 is required; gxhat / gu_in / gu_out may be null.
 * Same arithmetic as the nine launches (exact-fp32 16 x 16 x 4 matrix tiles, three real products per complex product);
 * the factor gradients are summed in a different (fixed) order.  All tensors 16-byte aligned.
 * OPT-IN: sc_tucker_chain_fused_supported returns 0 unless SC_TKC=1 is set in the environment -- measured on MI355X
 * at configs[2] the fused kernels are as accurate as the nine launches and slower (forward 104-114 us against 68.6 us,
 * backward 182-195 us against 139 us; profiles/r05_tkchain_ab.txt), so callers keep the nine
 * launches by default. */
int sc_tucker_chain_fused_supported(const sc_tucker_chain_desc* d);
size_t sc_tucker_chain_t3m_bytes(const sc_tucker_chain_desc* d);
int sc_tucker_chain_forward_fused(const sc_tucker_chain_desc* d, const float* xhat, const float* u_in, const float* t3,
                                  const float* u_out, float* t3m, float* z, float* t, float* yhat, void* stream);
size_t sc_tucker_chain_backward_fused_workspace_bytes(const sc_tucker_chain_desc* d);
int sc_tucker_chain_backward_fused(const sc_tucker_chain_desc* d, const float* xhat, const float* u_in, const float* t3m,
                                   const float* u_out, const float* z, const float* t, const float* gy, float* gxhat,
                                   float* gu_in, float* gt3, float* gu_out, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* ---- peer-store exchange of the mode-parallel layer (round 5, csrc/sc_kernels_peer.h; OPT-IN) ---------------------------
 * The all-to-all "split modes, cat batch" of the mode-sharded layer (the shape contract of neuralop/mpu/helpers.py:81-99,
 * which the reference defines and never calls) as direct stores into the peers' memory: every rank of ONE node owns a
 * window -- fine-grained device memory, sc_peer_window_alloc -- whose 64-byte HIP IPC handle the host side hands to the
 * other ranks (any transport), which map it with sc_peer_window_open.  sc_peer_all_to_all then issues three plain kernel
 * launches on `stream`: block p of `send` ([world][block_bytes]) is stored into slot `rank` of peer p's window and this
 * rank's epoch is written to slot `rank` of every peer's flags with system-scope release; a one-workgroup launch waits until
 * all `world` flags of THIS rank carry the epoch and the third copies the window into `recv` ([world][block_bytes], block p from
 * rank p).  No host synchronisation, capturable into a hipGraph (the epoch lives in the window's header and advances
 * per call).  Every rank must call it for every exchange, in the same order; a window may serve the next exchange of
 * the same kind one layer step later (the layer's exchanges alternate directions -- csrc/sc_kernels_peer.h), the host
 * side rotates a few windows.  peer_window[p] = the mapped base of rank p's window (own entry: the local pointer);
 * world <= 8, block_bytes a multiple of 16, send / recv 16-byte aligned.  Unmeasured on more than one GPU (no multi-GPU
 * tier in the build environment); self-tested with two processes on one device.
 * sc_peer_window_control (round 6): the wait launch spins without bound by default -- a peer that is merely late must not
 * corrupt a step -- which turns a dead peer or a non-coherent mapping into a stream that never drains.  A rank may give
 * the waits on ITS window a budget (milliseconds of the device's 100 MHz wall clock; 0 = unbounded, negative = unchanged)
 * and read the error word a timed-out wait leaves behind (0 = none, 1 + p = the flag of peer p never came; reading
 * clears it).  The host side runs its set-up self-test under a 2 s budget and falls back to the collective path on error. */
typedef struct sc_peer_exchange {
  int32_t world, rank;
  int64_t block_bytes;
  void* peer_window[8];
} sc_peer_exchange;
int sc_peer_window_alloc(size_t data_bytes, void** ptr, void* handle64);
int sc_peer_window_open(const void* handle64, void** ptr);
int sc_peer_window_close(void* ptr);
int sc_peer_window_free(void* ptr);
int sc_peer_all_to_all(const sc_peer_exchange* d, const void* send, void* recv, void* stream);
int sc_peer_window_control(void* own_window, int64_t spin_budget_ms, int32_t* error_out);

/* ---- pointwise half of an FNO block in one pass ("next" row f1 of SURVEY.md section 8) -------------------
 *   out = act( W2 gelu(W1 x + b1) + b2 + gate (.) skip_src )
 * replaces ChannelMLP.forward (neuralop/layers/channel_mlp.py:82-119: two Conv1d with kernel size 1 and a GELU),
 * the soft-gating skip (neuralop/layers/skip_connections.py:53-130: per-channel weight times the block input) and
 * the closing non-linearity of FNOBlocks.forward_with_postactivation (neuralop/layers/fno_block.py:399-412).
 * x (batch, c_in, spatial), skip_src / out (batch, c_out, spatial) contiguous float32; w1 (c_hid, c_in), w2 (c_out,
 * c_hid) row-major (= Conv1d weights with the trailing 1 dropped); b1, b2, skip_src + gate optional (null).
 * Channel counts: multiples of 32 with (c_in, c_hid, c_out) / 32 in {(1,1,1), (2,1,2), (2,2,2), (4,2,4)};
 * spatial a multiple of 32 below 2^28 points per image (all sc_pointwise_* entry points: lane offsets are 32-bit byte counts). */
typedef struct sc_pmlp_desc {
  int64_t batch, c_in, c_hid, c_out, spatial;
  int32_t act;               /* SC_ACT_NONE / SC_ACT_GELU on the result */
  int32_t reserved;
} sc_pmlp_desc;
int sc_pointwise_mlp_forward(const sc_pmlp_desc* d, const float* x, const float* w1, const float* b1, const float* w2,
                             const float* b2, const float* skip_src, const float* gate, float* out, void* stream);
/* The whole pointwise side of a default block's forward in ONE pass (session 2):
 *     s = conv + (ws x + bs);   y = act(s);   out = act( W2 gelu(W1 y + b1) + b2 + gate (.) x )
 * conv = the spectral convolution's output (sc_layer_forward without an epilogue), ws / bs = the block's 1 x 1 linear
 * skip (neuralop/layers/skip_connections.py:119-169), x = the block input; y and -- with SC_ACT_GELU -- s (`pre`) are
 * STORED because the backward passes (sc_pointwise_mlp_backward_ex with x = y, x_pre = s, then
 * sc_pointwise_linear_backward and sc_layer_backward_ex) read them.  Replaces sc_pointwise_linear_forward + the block
 * epilogue of sc_layer_forward_ex + sc_pointwise_mlp_forward (8 tensor-sized passes) by 1 + 5: the skip is never
 * written and y is not read back.  d->c_in == d->c_out in {32, 64} channels with c_hid as for the MLP pass; bs, b1, b2
 * optional; `pre` is required with SC_ACT_GELU (receives s) or SC_ACT_GELU_DGRAD (receives gelu'(s), see the enum) and ignored otherwise. */
int sc_pointwise_block_forward(const sc_pmlp_desc* d, const float* conv, const float* x, const float* ws, const float* bs,
                               const float* w1, const float* b1, const float* w2, const float* b2, const float* gate,
                               float* y, float* pre, float* out, void* stream);
/* gradient of the above with respect to everything: nothing but the forward's INPUTS is needed (h and the
 * pre-activations are recomputed inside the tile).  gx (batch, c_in, spatial), gskip_src (batch, c_out, spatial; with a
 * gate), gw1 / gw2 like w1 / w2, gb1 / gb2 / ggate (null when the forward had none) are all overwritten.  workspace:
 * sc_pointwise_mlp_workspace_bytes(d) bytes (operand tables + one partial sum per workgroup; the partials are added
 * in a fixed order; inside a workgroup the waves add with LDS atomics).  Shapes: (32,32,32), (64,32,64), (64,64,64) --
 * (128,64,128) has the forward pass only. */
size_t sc_pointwise_mlp_workspace_bytes(const sc_pmlp_desc* d);
int sc_pointwise_mlp_backward(const sc_pmlp_desc* d, const float* x, const float* w1, const float* b1, const float* w2,
                              const float* b2, const float* skip_src, const float* gate, const float* gout, float* gx,
                              float* gw1, float* gb1, float* gw2, float* gb2, float* gskip_src, float* ggate,
                              void* workspace, void* stream);
/* the same with x_pre (optional, like x): x = gelu(x_pre) came out of sc_layer_forward_ex; gx is then the gradient with
 * respect to x_pre -- the GELU backward of the Fourier layer in this pass' store path instead of a pass of its own.
 * d->act == SC_ACT_GELU_DGRAD: the MLP's closing activation is GELU and x_pre holds gelu'(pre-activation) (what
 * sc_pointwise_block_forward stored under the same code). */
int sc_pointwise_mlp_backward_ex(const sc_pmlp_desc* d, const float* x, const float* x_pre, const float* w1,
                                 const float* b1, const float* w2, const float* b2, const float* skip_src,
                                 const float* gate, const float* gout, float* gx, float* gw1, float* gb1, float* gw2,
                                 float* gb2, float* gskip_src, float* ggate, void* workspace, void* stream);

/* Round 6 -- the backward of sc_pointwise_block_forward's pointwise side with the DATA path of the linear skip riding along
 * (fno_block.py:392-414 backwards: closing GELU, soft-gating skip, ChannelMLP, the Fourier layer's GELU, and the linear skip's
 * W_s^T product): one pass reads y, y_pre, x, gout and writes
 *     gz  = the gradient of the Fourier layer's pre-activation s (= the gradient of the spectral convolution's output and
 *           of the linear skip's output),
 *     gin = W_s^T gz + gate (.) g_z  = the whole gradient of the block input outside the spectral convolution (the addend
 *           of sc_layer_backward_ex),
 * and the gradients of w1 / b1 / w2 / b2 / gate -- instead of sc_pointwise_mlp_backward_ex + sc_pointwise_linear_backward
 * (10 tensor-sized reads / writes -> 5; the skip's own weight gradient is then sc_pointwise_linear_backward_ex with
 * gx = NULL: 2 more).  d->act: SC_ACT_NONE (last block: y_pre NULL), SC_ACT_GELU (y_pre = s) or SC_ACT_GELU_DGRAD
 * (y_pre = gelu'(s), as stored by the forward call under the same code).  (channels, hidden) in {(32, 32), (64, 32)}
 * (sc_pointwise_block_backward_supported); workspace sc_pointwise_mlp_workspace_bytes(d) bytes. */
int sc_pointwise_block_backward_supported(const sc_pmlp_desc* d);
int sc_pointwise_block_backward(const sc_pmlp_desc* d, const float* y, const float* y_pre, const float* x,
                                const float* ws_lin, const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* gate, const float* gout, float* gz, float* gin, float* gw1, float* gb1,
                                float* gw2, float* gb2, float* ggate, void* workspace, void* stream);

/* 1 x 1 linear map over the channels in one pass each way: out = W x (+ bias) -- the block's linear skip
 * (neuralop/layers/skip_connections.py:119-169: Flattened1dConv = Conv1d with kernel size 1 on the flattened grid).
 * x (batch, c_in, spatial), out (batch, c_out, spatial), w (c_out, c_in) row-major, bias (c_out) or null.
 * c_in = c_out in {32, 64, 128} forward, {32, 64} backward; spatial a multiple of 32.  Backward: gx, gw (and gbias
 * when not null) are overwritten; gx_addend (optional, like gx): gx = W^T gout + gx_addend -- the gradient another
 * branch of the block sends to the same input, added in the store path instead of by a separate pass; workspace
 * sc_pointwise_linear_workspace_bytes(d) bytes. */
typedef struct sc_plin_desc {
  int64_t batch, c_in, c_out, spatial;
} sc_plin_desc;
int sc_pointwise_linear_forward(const sc_plin_desc* d, const float* x, const float* w, const float* bias, float* out,
                                void* stream);
size_t sc_pointwise_linear_workspace_bytes(const sc_plin_desc* d);
int sc_pointwise_linear_backward(const sc_plin_desc* d, const float* x, const float* w, const float* gout,
                                 const float* gx_addend, float* gx, float* gw, float* gbias, void* workspace,
                                 void* stream);

/* ---- the same maps with the block's pointwise operations in their load / store paths (round 6, csrc/sc_kernels_plinx.h) ----
 * Channel counts 32 / 64 / 128 in any combination.  A ChannelMLP whose channel counts have no one-pass kernel (hidden 128,
 * configs[4]'s width: channel_mlp.py:82-119) is two of these passes each way, the hidden activations crossing memory once
 * as their pre-activation; the soft-gating skip (skip_connections.py:53-130), the GELUs (fno_block.py:392-414) and their
 * derivatives ride in the passes, so nothing elementwise is left for the caller:
 *   forward   out = act(W xin + bias + gate (.) skip);  xin = gelu(x) with SC_PLX_XACT (x = the previous pass' pre_out);
 *             act = gelu with SC_PLX_ACT; pre_out (optional) receives the value before act
 *   backward  g = gout (.) gelu'(pre) with SC_PLX_PRO;  gskip = gate (.) g, ggate = sum g (.) skip when gated;
 *             gx = (W^T g + gx_addend) (.) gelu'(xg) (addend optional; the last factor with SC_PLX_XGRAD: for an XACT pass
 *             xg = x and gx is the gradient of the pre-activation);  gw = g xin^T;  gbias = sum g (null = not wanted).
 *             gx == NULL: the weight / bias / gate gradients only.
 * The backward call issues ceil(C_out / n) kernel launches (n output tiles of weight-gradient accumulators fit the
 * register file) + fixed-order reductions; workspace sc_pointwise_linear_workspace_bytes_ex(d) bytes. */
#define SC_PLX_XACT 1
#define SC_PLX_ACT 2
#define SC_PLX_PRO 4
#define SC_PLX_XGRAD 8
typedef struct sc_plinx_desc {
  int64_t batch, c_in, c_out, spatial;
  int32_t flags;
} sc_plinx_desc;
int sc_pointwise_linear_forward_ex(const sc_plinx_desc* d, const float* x, const float* w, const float* bias,
                                   const float* skip, const float* gate, float* out, float* pre_out, void* stream);
size_t sc_pointwise_linear_workspace_bytes_ex(const sc_plinx_desc* d);
int sc_pointwise_linear_backward_ex(const sc_plinx_desc* d, const float* x, const float* w, const float* gout,
                                    const float* pre, const float* xg, const float* skip, const float* gate,
                                    const float* gx_addend, float* gx, float* gw, float* gbias, float* gskip,
                                    float* ggate, void* workspace, void* stream);

/* ---- fused AdamW step of the spectral weights ("next" row f2 of SURVEY.md section 8) -----------------
 * One pass over (param, grad, exp_avg, exp_avg_sq) instead of the ~10 elementwise launches of
 * neuralop/training/adamw.py:155-200 (non-GaLore branch), same arithmetic in the same order:
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g conj(g);  p -= step_size m / (sqrt(v) + eps);
 *   p -= lr weight_decay p        with step_size = lr sqrt(1-b2^t) / (1-b1^t) when correct_bias.
 * is_complex: the four arrays hold n complex64 values (exp_avg_sq keeps the reference's complex layout,
 * imaginary part 0); otherwise n floats.  `step` is the 1-based step count AFTER the increment. */
typedef struct {
  double lr, beta1, beta2, eps, weight_decay;   /* python floats: 1 - beta is formed in double like upstream */
  int64_t step;
  int32_t correct_bias;
  int32_t reserved;
} sc_adamw_desc;
int sc_adamw_step(const sc_adamw_desc* d, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  int64_t n, int is_complex, void* stream);

/* ---- fused dense layer (the reference module's forward / implicit backward) -------------------
 * w: complex (cin, cout, w_extent...) stored weight; the used sub-block starts at w_start[d]
 * in every mode dim and has the plan's `kept` extents (centred block of :465-489).
 * xhat_saved: complex (batch, cin, k...) written by forward, read by backward.
 * workspace: sc_layer_workspace_bytes(plan, batch, max(cin, cout)) bytes. */
typedef struct {
  int32_t batch, cin, cout, reserved;
  int64_t w_extent[SC_MAX_DIMS];
  int64_t w_start[SC_MAX_DIMS];
} sc_layer_desc;

size_t sc_layer_workspace_bytes(const sc_plan* plan, const sc_layer_desc* L);

int sc_layer_forward(const sc_plan* plan, const sc_layer_desc* L, const float* x,
                     const float* w, const float* bias, float* y, float* xhat_saved,
                     void* workspace, void* stream);

/* gw must be zero-initialised by the caller when the used sub-block is smaller than the
 * stored weight (only the sub-block is written).  gbias may be NULL. */
int sc_layer_backward(const sc_plan* plan, const sc_layer_desc* L, const float* gy,
                      const float* xhat_saved, const float* w, float* gx, float* gw,
                      float* gbias, void* workspace, void* stream);
/* sc_layer_backward with gx = (gradient through the layer) + gx_addend (optional; same shape as gx): the gradient the
 * other branches of an FNO block send to the layer's input, added in the store path of the last transform. */
int sc_layer_backward_ex(const sc_plan* plan, const sc_layer_desc* layer, const float* gy,
                         const float* xhat_saved, const float* w, float* gx, float* gw, float* gbias,
                         const float* gx_addend, void* workspace, void* stream);

/* ---- block epilogue (first "next" row f1 of SURVEY.md section 8) ---------------------------------------------------
 * The FNO block computes act(conv(x) + skip(x)) around the spectral convolution (neuralop/layers/fno_block.py:392-414:
 * x_fno + x_skip_fno, then the non-linearity) -- three more passes over tensors of the activation's size.  With an
 * epilogue the inverse transform adds `skip` (same shape and storage type as y) and applies the activation while it
 * stores:  y = act(irfft(...) + bias + skip).  preact (optional, same shape) receives the value before the
 * activation, which the backward of the activation needs.  On the fused 2-D kernels this happens in the store path of
 * the inverse transform (one extra read of the activation's size); other shapes run one streaming pass after it. */
/* GELU: torch.nn.functional.gelu's default form 0.5 v (1 + erf(v / sqrt 2)), with erf / erfc evaluated by the
 * 5-term rational approximation Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7 absolute in erf in exact arithmetic; the negative tail
 * is taken from erfc directly, so it does not cancel: relative error < 1 % down to v = -6) -- the library erff made
 * the fused inverse transform 5 x slower.  Absolute error of the activation <= 0.5 |v| 7e-7 incl. fp32 round-off
 * (rel-L2 ~1e-7 on N(0,1) data; pinned in tests/test_emu_epilogue.py for |v| <= 6).  The fused store path and the stand-alone
 * pass evaluate the SAME function (identical bits for every grid shape).
 * preact: written if and only if act == SC_ACT_GELU; preact != NULL together with SC_ACT_NONE is rejected. */
enum { SC_ACT_NONE = 0, SC_ACT_GELU = 1,
       /* round 6, sc_pointwise_block_forward / sc_pointwise_mlp_backward_ex only: as SC_ACT_GELU, but the `pre` buffer of the
          forward call receives gelu'(s) -- the DERIVATIVE of the Fourier layer's activation, which comes out of the same
          evaluation of the two transcendentals as gelu(s) itself -- and `x_pre` of the backward call holds that
          derivative: the backward multiplies by it instead of evaluating gelu' per value (on MI355X the vector work of
          these fp32 kernels runs in front of their matrix instructions, not beside them: DESIGN 3.16 b) */
       SC_ACT_GELU_DGRAD = 2 };
typedef struct {
  const float* skip;        /* device, (n_images, d1..dN); NULL = no epilogue at all          */
  float* preact;            /* device, optional                                                 */
  int32_t act;              /* SC_ACT_*                                                         */
  int32_t reserved;
} sc_epilogue;

int sc_transform_inverse_ex(const sc_plan* plan, int mode, const float* yhat, const float* bias, int64_t channels,
                            const sc_epilogue* ep, float* y, int64_t n_images, void* workspace, void* stream);
int sc_layer_forward_ex(const sc_plan* plan, const sc_layer_desc* L, const float* x, const float* w,
                        const float* bias, const sc_epilogue* ep, float* y, float* xhat_saved, void* workspace,
                        void* stream);

/* ---- sharded spectra (round 3; mode-parallel layers) -------------------------------------------
 * The reference defines the exchange of a mode-sharded layer only as a shape contract (mpu/helpers.py:81-99, the
 * unused `_transpose`: split dim0, all-to-all, concatenate dim1).  Here the transforms on either side of that
 * all-to-all write / read its rank-major buffer IN PLACE, so that no permutation copy is left around the collective:
 * the kept block of every image is cut along its FIRST mode dim into n_blocks blocks of `rows` rows
 * (n_blocks * rows >= k1; rows past k1 are zeros on the wire -- round 5: also whole blocks, e.g. k1 = 6 over 4 ranks =
 * three blocks of 2 rows and an empty one) and block p of image i lives at
 *     xhat + p * block_stride + (i * rows + r) * rest + j        (complex elements; rest = k2 * .. * kN)
 * i.e. xhat is the tensor [n_blocks][n_images][rows][rest] (block_stride >= n_images * rows * rest).  The fused 2-D
 * kernels address this layout natively; every other shape runs the plain transform through a staging copy in the
 * workspace plus ONE streaming permutation -- same results, sc_plan_workspace_bytes_sharded() bytes of workspace. */
typedef struct {
  int64_t n_blocks;      /* ranks of the model-parallel group                               */
  int64_t rows;          /* rows of the first kept dim per block: ceil(k1 / n_blocks)       */
  int64_t block_stride;  /* complex elements from one block to the next                     */
} sc_spectrum_shards;
size_t sc_plan_workspace_bytes_sharded(const sc_plan* plan, int64_t n_images);
/* as sc_transform_forward / sc_transform_inverse (same modes), spectrum in the sharded layout */
int sc_transform_forward_sharded(const sc_plan* plan, int mode, const float* x, float* xhat, int64_t n_images,
                                 const sc_spectrum_shards* shards, void* workspace, void* stream);
int sc_transform_inverse_sharded(const sc_plan* plan, int mode, const float* yhat, const float* bias,
                                 int64_t channels, float* y, int64_t n_images, const sc_spectrum_shards* shards,
                                 void* workspace, void* stream);
/* sc_bias_grad on a sharded adjoint spectrum (batch * channels images) */
int sc_bias_grad_sharded(const sc_plan* plan, const float* ghat, int64_t batch, int64_t channels,
                         const sc_spectrum_shards* shards, float* gbias, void* stream);

/* ---- misc ------------------------------------------------------------------------------------ */
const char* sc_last_error(void);
const char* sc_version(void);
/* name of the dominant kernel a transform over this plan launches (for profile matching) */
const char* sc_plan_kernel_name(const sc_plan* plan, int which);

#ifdef __cplusplus
}
#endif
#endif /* SC_ENGINE_H */
