// sc_host_modegemm.h -- the contraction router and its six routes (VALU, matrix cores, streamed matrix cores, small
// extent, factor matrix on the VALU / on the matrix cores).  Implements sc_modegemm(_path, _uses_matrix_cores),
// sc_modegemm_pair(_path, _fused) and sc_modegemm_msum(_ws, _path, _workspace_bytes).
// SC_DIAG_ENV comes from the includer (sc_engine.cpp defines it before the parts).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "sc_host_common.h"
#include "sc_kernels_generic.h"
#include "sc_kernels_sb.h"
#include "sc_kernels_tucker.h"   // tkm_ld_rows
#include "sc_kernels_fmx.h"
#include "sc_kernels_mfma.h"
#include "sc_kernels_gemm8.h"

template <int PT, int QT>
static int launch_modegemm(const ModeGemmArgs& g0, int ca, int cb, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  ModeGemmArgs g = g0;
  g.n_mt = (int)((g.M + SC_WAVE - 1) / SC_WAVE);
  g.n_pg = (int)((g.P + 4 * PT - 1) / (4 * PT));
  g.n_qt = (int)((g.Q + QT - 1) / QT);
  // (the four waves of a workgroup over four neighbouring mode tiles instead of p groups when P <= PT -- 2 KB
  // contiguous per operand row for the weight-streaming launches at B = 4 -- changed nothing:
  // profiles/r02_valu_contraction_wave_modes_ab.txt)
  const int64_t total = (int64_t)g.n_mt * g.n_pg * g.n_qt;
  g.per_xcd = (int)((total + 7) / 8);
  dim3 grid((unsigned)(8 * g.per_xcd));
  sc_conj_dispatch(ca, cb, [&](auto CA, auto CB) {
    SC_LAUNCH((k_modegemm<PT, QT, decltype(CA)::value, decltype(CB)::value>), grid, dim3(SC_BLOCK), 0, st, g, A, B, C);
  });
  return sc_check_launch("k_modegemm");
}

// ---- small-extent streaming path (sc_kernels_sb.h): a batch of <= SB_MAX rows against a large weight, or a
//      reduction of <= SB_MAX terms into a weight-sized result (BASELINE configs[4], B = 4)
static int sb_max_extent() {
  // default 4: the regime where both older kernels are known to be slow.  SC_SB_MAX=n (environment,
  // read once) moves the bound for A-B runs: 0 switches the path off, 8 also takes FNO3d's B = 8 launches
  static const int v = [] {
    const char* e = SC_DIAG_ENV("SC_SB_MAX");
    const int n = e ? std::atoi(e) : 4;
    return n < 0 ? 0 : (n > 8 ? 8 : n);
  }();
  return v;
}
// work-item order of the small-batch kernels (sc_kernels_sb.h, SbGemmArgs::mt_fastest).  Defaults (round 5, measured at
// configs[4], profiles/r05_sb_order_ab.txt): k_modegemm_sb mode tiles slowest, the one-pass pair k_modegemm_sb_bwd mode
// tiles fastest.  SC_GEMM_SB_ALT_ORDER on a descriptor and SC_SB_ALT_ORDER (environment, read once: bit 0 = single
// launches, bit 1 = the pair) each flip it.
static int sb_alt_order_env() {
  static const int v = [] { const char* e = SC_DIAG_ENV("SC_SB_ALT_ORDER"); return e ? std::atoi(e) : 0; }();
  return v;
}
static bool sb_gemm_eligible(const sc_modegemm_desc* d, const void* A, const void* B, const void* C) {
  if (d->flags & (SC_GEMM_F16 | SC_GEMM_NO_SB)) return false;
  if (d->accumulate || d->b_idx || d->c_idx || d->a_sg || d->b_sg || d->c_sg) return false;
  if (d->a_sm != 1 || d->b_sm != 1 || d->c_sm != 1) return false;
  if ((d->n_modes & 1) || d->n_modes < 2) return false;
  if ((d->a_sp | d->a_sr | d->b_sr | d->b_sq | d->c_sp | d->c_sq) & 1) return false;   // 16-byte aligned rows
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) return false;
  const int64_t small = d->P < d->R ? d->P : d->R;
  return small <= sb_max_extent();
}

template <int PT, int QT, int ST, int WM, int WP, int WQ>
static int run_sb_gemm_t(const sc_modegemm_desc* d, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  SbGemmArgs g;
  g.P = d->P; g.Q = d->Q; g.R = d->R; g.M = d->n_modes;
  g.a_sp = d->a_sp; g.a_sr = d->a_sr; g.b_sr = d->b_sr; g.b_sq = d->b_sq; g.c_sp = d->c_sp; g.c_sq = d->c_sq;
  g.n_mt = (int)((d->n_modes + 128 * WM - 1) / (128 * WM));
  g.n_pt = (int)((d->P + PT - 1) / PT);
  g.n_qt = (int)((d->Q + QT - 1) / QT);
  const int64_t total = (int64_t)g.n_mt * ((g.n_pt + WP - 1) / WP) * ((g.n_qt + WQ - 1) / WQ);
  if (total >= ((int64_t)1 << 30)) return -1;
  g.per_xcd = (int)((total + 7) / 8);
  g.mt_fastest = (0 ^ (sb_alt_order_env() & 1) ^ ((d->flags & SC_GEMM_SB_ALT_ORDER) ? 1 : 0)) & 1;
  // an operand that exactly one tile reads crosses the chip once: keep it out of the caches the shared one lives in
  g.nt_a = g.n_qt == 1;
  g.nt_b = g.n_pt == 1;
  static const bool plain_c = SC_DIAG_ENV("SC_SB_PLAIN_C") != nullptr;               // A-B
  g.nt_c = (d->flags & SC_GEMM_STREAM_C) && !plain_c ? 1 : 0;
  const dim3 grid((unsigned)(8 * g.per_xcd));
  sc_conj_dispatch(d->conj_a, d->conj_b, [&](auto CA, auto CB) {
    SC_LAUNCH((k_modegemm_sb<PT, QT, ST, WM, WP, WQ, decltype(CA)::value, decltype(CB)::value>), grid, dim3(SC_BLOCK), 0, st, g, A, B, C);
  });
  return sc_check_launch("k_modegemm_sb");
}

static int run_sb_gemm(const sc_modegemm_desc* d, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  // small batch: the register tile holds every row (4 x 4, or 8 x 2 for 5..8 rows), three reduction steps in
  // flight; short reduction (weight gradient): 4 x 4 outputs per lane, two steps in flight.  Wave arrangement
  // (sc_kernels_sb.h): the four waves over four column tiles (2 x 2 tiles for the weight gradient) of one 128-mode
  // tile; SC_GEMM_SB_WM4 / SC_SB_WM=4 (flag / environment, A-B) = four neighbouring 128-mode tiles of one tile instead
  static const bool wm4_env = [] { const char* e = SC_DIAG_ENV("SC_SB_WM"); return e && std::atoi(e) == 4; }();
  const bool wm4 = wm4_env || (d->flags & SC_GEMM_SB_WM4);
  if (d->P <= 4)
    return wm4 ? run_sb_gemm_t<4, 4, 3, 4, 1, 1>(d, A, B, C, st) : run_sb_gemm_t<4, 4, 3, 1, 1, 4>(d, A, B, C, st);
  if (d->P <= 8 && d->P <= d->R)
    return wm4 ? run_sb_gemm_t<8, 2, 3, 4, 1, 1>(d, A, B, C, st) : run_sb_gemm_t<8, 2, 3, 1, 1, 4>(d, A, B, C, st);
  return wm4 ? run_sb_gemm_t<4, 4, 2, 4, 1, 1>(d, A, B, C, st) : run_sb_gemm_t<4, 4, 2, 1, 2, 2>(d, A, B, C, st);
}

// ---- the two contractions of a small-batch backward pass in one pass over the weight (sc_kernels_sb.h,
//      k_modegemm_sb_bwd): d0 = weight gradient (conj A: xhat^H ghat), d1 = gradient of the spectrum (conj B: ghat W^H),
//      both operands named ghat the SAME array.  Returns -1 when the pair does not qualify.
template <int BT>
static int run_sb_bwd_t(const SbBwdArgs& g, const cf32* xhat, const cf32* ghat, const cf32* W, cf32* gW, cf32* gxhat,
                        sc_stream_t st) {
  SC_LAUNCH((k_modegemm_sb_bwd<BT, 4, 2>), dim3((unsigned)(8 * g.per_xcd)), dim3(SC_BLOCK), 0, st, g, xhat, ghat, W, gW,
            gxhat);
  return sc_check_launch("k_modegemm_sb_bwd");
}

static bool sb_bwd_eligible(const sc_modegemm_desc* d0, const void* A0, const void* B0, const void* C0,
                            const sc_modegemm_desc* d1, const void* A1, const void* B1, const void* C1) {
  static const bool off = SC_DIAG_ENV("SC_SB_NO_PAIR") != nullptr;                     // A-B
  if (off) return false;
  if (!sb_gemm_eligible(d0, A0, B0, C0) || !sb_gemm_eligible(d1, A1, B1, C1)) return false;
  if (!(d0->conj_a && !d0->conj_b && !d1->conj_a && d1->conj_b)) return false;
  if (B0 != A1 || d0->b_sr != d1->a_sp || d0->b_sq != d1->a_sr) return false;          // one ghat[b, o, m]
  if (d0->n_modes != d1->n_modes || d0->R != d1->P || d0->P != d1->Q || d0->Q != d1->R) return false;
  if (d0->R < 1 || d0->R > 4 || d0->R > sb_max_extent()) return false;                // the batch lives in registers
  // the weight-sized arrays must dominate: otherwise the separate launches (more, smaller work items) fill the chip better
  return d0->P * d0->Q >= 64 * d0->R;
}

static int run_sb_bwd(const sc_modegemm_desc* d0, const cf32* A0, const cf32* B0, cf32* C0,
                      const sc_modegemm_desc* d1, const cf32* A1, const cf32* B1, cf32* C1, sc_stream_t st) {
  if (!sb_bwd_eligible(d0, A0, B0, C0, d1, A1, B1, C1)) return -1;
  SbBwdArgs g;
  g.B = d0->R; g.Ci = d0->P; g.Co = d0->Q; g.M = d0->n_modes;
  g.x_si = d0->a_sp; g.x_sb = d0->a_sr;
  g.g_sb = d0->b_sr; g.g_so = d0->b_sq;
  g.gw_si = d0->c_sp; g.gw_so = d0->c_sq;
  g.w_so = d1->b_sr; g.w_si = d1->b_sq;
  g.gx_sb = d1->c_sp; g.gx_si = d1->c_sq;
  g.n_mt = (int)((g.M + 127) / 128);
  g.n_itg = (int)(((g.Ci + 3) / 4 + 3) / 4);
  const int64_t total = (int64_t)g.n_mt * g.n_itg;
  if (total >= ((int64_t)1 << 30)) return -1;
  g.per_xcd = (int)((total + 7) / 8);
  g.mt_fastest = (1 ^ ((sb_alt_order_env() >> 1) & 1) ^ (((d0->flags | d1->flags) & SC_GEMM_SB_ALT_ORDER) ? 1 : 0)) & 1;
  static const bool plain_c = SC_DIAG_ENV("SC_SB_PLAIN_C") != nullptr;                 // A-B
  g.nt_gw = (d0->flags & SC_GEMM_STREAM_C) && !plain_c ? 1 : 0;
  switch (g.B) {
    case 1: return run_sb_bwd_t<1>(g, A0, B0, B1, C0, C1, st);
    case 2: return run_sb_bwd_t<2>(g, A0, B0, B1, C0, C1, st);
    case 3: return run_sb_bwd_t<3>(g, A0, B0, B1, C0, C1, st);
    default: return run_sb_bwd_t<4>(g, A0, B0, B1, C0, C1, st);
  }
}

// ---- mode-independent right operand (sc_kernels_sb.h, k_modegemm_bfac): factor matrices through the scalar cache
static bool bfac_gemm_eligible(const sc_modegemm_desc* d) {
  if (d->flags & (SC_GEMM_F16 | SC_GEMM_NO_SB)) return false;
  if (d->accumulate || d->b_idx || d->c_idx || d->a_sg || d->b_sg || d->c_sg) return false;
  if (d->b_sm != 0 || d->a_sm != 1 || d->c_sm != 1) return false;
  return d->Q >= 8 && d->R >= 4 && d->n_modes >= 64 && d->R * ((d->Q + 1) & ~(int64_t)1) <= 8192;   // B in <= 64 KiB of LDS
}

template <int QC>
static int run_bfac_gemm_t(const sc_modegemm_desc* d, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  BfacGemmArgs g;
  g.P = d->P; g.Q = d->Q; g.R = d->R; g.M = d->n_modes;
  g.a_sp = d->a_sp; g.a_sr = d->a_sr; g.b_sr = d->b_sr; g.b_sq = d->b_sq; g.c_sp = d->c_sp; g.c_sq = d->c_sq;
  g.n_mt = (int)((d->n_modes + 63) / 64);
  g.n_qg = (int)((d->Q + 4 * QC - 1) / (4 * QC));
  const int64_t total = (int64_t)g.n_mt * g.n_qg * d->P;
  if (total >= ((int64_t)1 << 31)) return -1;
  const dim3 grid((unsigned)total);
  const size_t shmem = (size_t)(d->R * ((d->Q + 1) & ~(int64_t)1)) * sizeof(cf32);
  sc_conj_dispatch(d->conj_a, d->conj_b, [&](auto CA, auto CB) {
    SC_LAUNCH((k_modegemm_bfac<QC, decltype(CA)::value, decltype(CB)::value>), grid, dim3(SC_BLOCK), shmem, st, g, A, B, C);
  });
  return sc_check_launch("k_modegemm_bfac");
}

static int run_bfac_gemm(const sc_modegemm_desc* d, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  // columns per wave: 9 when that divides the work into whole waves better (ranks such as 36, 18, 27), else 8
  const int64_t w8 = (d->Q + 7) / 8, w9 = (d->Q + 8) / 9;
  return (w9 * 9 - d->Q < w8 * 8 - d->Q) ? run_bfac_gemm_t<9>(d, A, B, C, st) : run_bfac_gemm_t<8>(d, A, B, C, st);
}

#ifndef SC_EMU
#define SC_FMX_ATTR(kern, lds)                                                                                    \
  if ((lds) > 64 * 1024)                                                                                         \
  SC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)))
#else
#define SC_FMX_ATTR(kern, lds) (void)0
#endif
static int tucker_abl() {
  static const int v = [] { const char* e = SC_DIAG_ENV("SC_TK_ABL"); return e ? std::atoi(e) : 0; }();
  return v;
}
// ---- factor-matrix products and mode-summed contractions on the matrix cores (sc_kernels_fmx.h) ---------------
static bool fmx_off() {
  static const bool off = SC_DIAG_ENV("SC_FMX_OFF") != nullptr;                        // A-B against the VALU kernels
  return off;
}
// workgroups for n chunks with `cap` co-resident: every workgroup the same number of rounds
static int fmx_wgs(int64_t chunks, int64_t cap) {
  const int64_t rounds = (chunks + cap - 1) / cap;
  int64_t wgs = (chunks + rounds - 1) / rounds;
  // Session 2: a launch is as slow as its busiest compute unit, so the workgroup count is rounded DOWN to a multiple
  // of the unit count when that costs the busiest workgroup at most one more chunk: TFNO rank 0.1 has 1056 chunks
  // (32 rows x 33 mode blocks): 528 workgroups of 2 chunks put three workgroups = 6 chunks on 16 units (average 4.1),
  // 512 workgroups (32 of them with 3 chunks) put 5 on the busiest.  SC_FMX_WGS_EXACT=1 (environment, A-B): the old rule
  static const bool exact = SC_DIAG_ENV("SC_FMX_WGS_EXACT") != nullptr;
  const int64_t cus = sc_cu_count();
  const int64_t m = (wgs / cus) * cus;
  if (!exact && m >= cus && m < wgs && (chunks + m - 1) / m <= rounds + 1) wgs = m;
  return (int)wgs;
}
static bool fmx_bfac_eligible(const sc_modegemm_desc* d) {
  if (fmx_off() || (d->flags & (SC_GEMM_F16 | SC_GEMM_NO_FMX | SC_GEMM_FORCE_VALU))) return false;
  if (d->accumulate || d->b_idx || d->c_idx || d->a_sg || d->b_sg || d->c_sg) return false;
  if (d->b_sm != 0 || d->a_sm != 1 || d->c_sm != 1) return false;
  if (d->Q < 8 || d->Q > 64 || d->R < 4 || d->R > 64 || d->n_modes < 64) return false;
  return d->P * ((d->n_modes + 63) / 64) < ((int64_t)1 << 30);
}
template <int PF, int TQ>
static int run_fmx_bfac_t(const sc_modegemm_desc* d, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  FmxArgs g;
  g.P = d->P; g.Q = d->Q; g.R = d->R; g.M = d->n_modes;
  g.a_sp = d->a_sp; g.a_sr = d->a_sr; g.b_sr = d->b_sr; g.b_sq = d->b_sq; g.c_sp = d->c_sp; g.c_sq = d->c_sq;
  g.n_mb = (int)((d->n_modes + 63) / 64);
  g.n_chunks = (int)(d->P * g.n_mb);
  const int q4 = (int)((d->Q + 3) & ~(int64_t)3), r4 = (int)((d->R + 3) & ~(int64_t)3);
  g.ldb = tkm_ld_rows(r4);
  g.abl = tucker_abl();
  g.inv_q = (uint32_t)((((uint64_t)1 << 32) + (uint64_t)d->Q - 1) / (uint64_t)d->Q);
  const size_t lds = (size_t)(q4 * g.ldb + r4 * SC_FMX_LDK) * sizeof(cf32);
  g.n_wg = fmx_wgs(g.n_chunks, sc_cu_count() * (int64_t)(160 * 1024 / lds > 4 ? 4 : 160 * 1024 / lds));
  return sc_conj_dispatch(d->conj_a, d->conj_b, [&](auto CA, auto CB) -> int {
    auto kern = k_modegemm_bfac_mx<PF, TQ, decltype(CA)::value, decltype(CB)::value>;
    SC_FMX_ATTR(kern, lds);
    SC_LAUNCH(kern, dim3((unsigned)g.n_wg), dim3(256), lds, st, g, A, B, C);
    return sc_check_launch("k_modegemm_bfac_mx");
  });
}
static int run_fmx_bfac(const sc_modegemm_desc* d, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  if (d->R <= 36) return d->Q <= 48 ? run_fmx_bfac_t<9, 3>(d, A, B, C, st) : run_fmx_bfac_t<9, 4>(d, A, B, C, st);
  return d->Q <= 48 ? run_fmx_bfac_t<16, 3>(d, A, B, C, st) : run_fmx_bfac_t<16, 4>(d, A, B, C, st);
}

static bool fmx_msum_eligible(const sc_modegemm_desc* d) {
  if (fmx_off() || (d->flags & (SC_GEMM_F16 | SC_GEMM_NO_FMX | SC_GEMM_FORCE_VALU))) return false;
  if (d->b_idx || d->c_idx || d->a_sg || d->b_sg || d->c_sg) return false;
  if (d->a_sm != 1 || d->b_sm != 1) return false;
  if (d->P < 8 || d->P > 64 || d->Q < 8 || d->Q > 64 || d->n_modes < 64 || d->R < 1) return false;
  return d->R * ((d->n_modes + 63) / 64) < ((int64_t)1 << 30);
}
static void fmx_msum_args(const sc_modegemm_desc* d, FmxArgs& g, size_t& lds) {
  g.P = d->P; g.Q = d->Q; g.R = d->R; g.M = d->n_modes;
  g.a_sp = d->a_sp; g.a_sr = d->a_sr; g.b_sr = d->b_sr; g.b_sq = d->b_sq; g.c_sp = d->c_sp; g.c_sq = d->c_sq;
  g.n_mb = (int)((d->n_modes + 63) / 64);
  g.n_chunks = (int)(d->R * g.n_mb);
  g.ldb = 0;
  g.inv_q = 0;
  g.abl = tucker_abl();
  const int p4 = (int)((d->P + 3) & ~(int64_t)3), q4 = (int)((d->Q + 3) & ~(int64_t)3);
  lds = (size_t)((p4 + q4) * SC_FMX_LDR) * sizeof(cf32);
  const int64_t per_cu = 160 * 1024 / lds > 3 ? 3 : 160 * 1024 / lds;
  g.n_wg = fmx_wgs(g.n_chunks, sc_cu_count() * per_cu);
}
template <int PFA, int PFB, int SLOTS>
static int run_fmx_msum_t(const sc_modegemm_desc* d, const FmxArgs& g, size_t lds, const cf32* A, const cf32* B,
                          cf32* partial, sc_stream_t st) {
  return sc_conj_dispatch(d->conj_a, d->conj_b, [&](auto CA, auto CB) -> int {
    auto kern = k_modegemm_msum_mx<PFA, PFB, SLOTS, decltype(CA)::value, decltype(CB)::value>;
    SC_FMX_ATTR(kern, lds);
    SC_LAUNCH(kern, dim3((unsigned)g.n_wg), dim3(256), lds, st, g, A, B, partial);
    return sc_check_launch("k_modegemm_msum_mx");
  });
}

// ---- matrix-core path (sc_kernels_mfma.h): channel counts that fill 32 x 32 MFMA tiles ----------
static bool mfma_gemm_eligible(const sc_modegemm_desc* d) {
  // one workgroup tile is 32 or 64 rows x 64 columns; ragged problems (Tucker / TT ranks such as 36) take it
  // when they fill at least ~half of a tile, smaller ones stay on the lanes-are-modes VALU kernel
  if (d->accumulate) return false;
  if (d->Q < 24 || d->Q > 64) return false;
  if (d->P < 24 || d->P > 64) return false;
  if (d->R < 8) return false;
  // a single 8-deep stage only pays on a (nearly) full tile: P = Q = 32, R = 8 over 17 k modes was 148 us
  // here against 85 us on the VALU kernel
  const int64_t rows = d->P <= 32 ? 32 : 64;
  if (d->R < 16 && 4 * d->P * d->Q < 3 * rows * 64) return false;
  if (d->n_modes >= ((int64_t)1 << 31) / 16) return false;
  return true;
}

// two shapes of the matrix-core kernel:
//   wide   (default): 9 modes per workgroup, 8 waves, one workgroup per CU;
//   paired (P = 32, SC_GEMM_PAIRED, A-B only): 5 modes per workgroup, 4 waves, two workgroups per CU.
//     Measured: same speed with warm caches (53.9 vs 53.8 us), SLOWER from HBM (78.6 vs 63.9 us):
//     40-byte segments cost more DRAM/fabric efficiency than the second workgroup's latency hiding buys.
#define SC_MG_NM_WIDE 9
#define SC_MG_NM_PAIRED 5
//   few    (n_modes <= SC_MG_FEW_MAX, e.g. a 64 x 64 grid keeping 32 x 17): 4 modes per workgroup.  With 9
//     slots a small problem either leaves most CUs idle or, spread over all of them, multiplies stale
//     slots (the MFMAs of a workgroup always cover all its NM slots): 72 us for 53 MB at 544 modes.
#define SC_MG_NM_FEW 4
#ifndef SC_MG_FEW_MAX
#define SC_MG_FEW_MAX 1152
#endif
template <int PT, int NM, int NWV>
static void launch_mfma_gemm(const MfmaGemmArgs& g, int ca, int cb, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  sc_conj_dispatch(ca, cb, [&](auto CA, auto CB) {
    SC_LAUNCH((k_modegemm_mfma<PT, 4, NM, decltype(CA)::value, decltype(CB)::value, NWV>), dim3((unsigned)g.G),
              dim3((MfmaGemmCfg<PT, 4, NM, NWV>::THREADS)), 0, st, g, A, B, C);
  });
}

static int run_mfma_gemm(const sc_modegemm_desc* d, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  MfmaGemmArgs g;
  g.P = (int)d->P; g.Q = (int)d->Q; g.R = (int)d->R; g.M = (int)d->n_modes;
  g.a_sp = d->a_sp; g.a_sr = d->a_sr; g.a_sm = d->a_sm;
  g.b_sr = d->b_sr; g.b_sq = d->b_sq; g.b_sm = d->b_sm;
  g.c_sp = d->c_sp; g.c_sq = d->c_sq; g.c_sm = d->c_sm;
  g.b_idx = d->b_idx; g.c_idx = d->c_idx;
  g.stream_c = (d->flags & SC_GEMM_STREAM_C) ? 1 : 0;
  // contiguous mode ranges of <= NM modes, split evenly over (workgroups per CU) x 256 CUs
  const bool paired = d->P <= 32 && (d->flags & SC_GEMM_PAIRED);
  const int64_t M = d->n_modes;
  const bool few = !paired && M <= SC_MG_FEW_MAX && !(d->flags & SC_GEMM_WIDE);
  const int64_t nmx = paired ? SC_MG_NM_PAIRED : (few ? SC_MG_NM_FEW : SC_MG_NM_WIDE);
  int64_t G = (M + nmx - 1) / nmx;
  const int64_t slots = paired ? 512 : 256;
  if (few) G = G < 8 ? G : (G + 7) / 8 * 8;        // keep the ranges full: ceil(M / 4) workgroups
  else if (G < slots) G = M < slots ? M : slots;
  else G = (G + 7) / 8 * 8;
  if (G > M) G = M;
  const int64_t cap = (d->flags >> 8) & 0xffff;               // SC_GEMM_GRID(n): tests / tuning
  if (cap > 0 && cap < G && cap * nmx >= M) G = cap;
  g.G = (int)G;
  if (paired) launch_mfma_gemm<1, SC_MG_NM_PAIRED, 4>(g, d->conj_a, d->conj_b, A, B, C, st);
  else if (few && d->P <= 32) launch_mfma_gemm<1, SC_MG_NM_FEW, 8>(g, d->conj_a, d->conj_b, A, B, C, st);
  else if (few) launch_mfma_gemm<2, SC_MG_NM_FEW, 8>(g, d->conj_a, d->conj_b, A, B, C, st);
  else if (d->P <= 32) launch_mfma_gemm<1, SC_MG_NM_WIDE, 8>(g, d->conj_a, d->conj_b, A, B, C, st);
  else launch_mfma_gemm<2, SC_MG_NM_WIDE, 8>(g, d->conj_a, d->conj_b, A, B, C, st);
  return sc_check_launch("k_modegemm_mfma");
}

// ---- streamed matrix-core path (sc_kernels_gemm8.h): plain contiguous-mode operands ------------------------------
// Two shapes of the kernel are built into the library (profiles/r02_gemm_dma_v3_shapes_ab.txt):
//   narrow   8 modes x 32 x 32 tiles, 4 waves, 2 r pairs per stage, plain stage loop: 528 workgroups for the forward
//            / gX contraction of the metric shape (45 us; 16 modes x 8 waves: 54 us)
//   wide    16 modes x 32 x 32 tiles, 8 waves, 128-byte segments, software-pipelined stage: calls with >= 8 tiles per
//            mode group (hidden 128: weight gradient 173 against 224 us, and the store-dominated weight gradient of
//            the 1024^2 config 1.38 against 2.1 ms).  The metric shape's weight gradient (4 tiles) measures 46.6
//            against 51.2 us stand-alone but 63.9 against 53.5 us INSIDE a step (profiles/r02_gpu6_kernel_stats.txt:
//            its operands come from HBM there) and stays on the narrow shape
// Measured (profiles/r02_gemm_dma_diag_grid_layout.txt): ONE workgroup needs ~33 us for its stages whatever the
// operand layout, segment size, ring depth or instruction order -- so a launch is as fast as its busiest CU.
#if defined(SC_G8_SHAPE) && SC_G8_SHAPE == 1       // measurement builds: one r pair per stage, deeper ring
#define SC_G8_NARROW 4, 2, 1, 5, false             // 40 KiB of LDS: 4 workgroups per CU
#define SC_G8_NARROW_RESIDENT 1024
#elif defined(SC_G8_SHAPE) && SC_G8_SHAPE == 2
#define SC_G8_NARROW 4, 2, 1, 4, false             // 32 KiB: 5 per CU
#define SC_G8_NARROW_RESIDENT 1280
#else
#define SC_G8_NARROW 4, 2, 2, 3, false
#define SC_G8_NARROW_RESIDENT 768
#endif
#define SC_G8_WIDE 8, 2, 1, 4, true
// workgroups the chip holds at once: narrow 3 per CU (48 KiB of LDS each), wide 2 per CU (64 KiB)
#define SC_G8_RESIDENT(wide) ((wide) ? 512 : SC_G8_NARROW_RESIDENT)
static bool gemm8_eligible(const sc_modegemm_desc* d, const void* A, const void* B, const void* C) {
  if (d->flags & (SC_GEMM_FORCE_VALU | SC_GEMM_NO_STREAM | SC_GEMM_F16)) return false;
  if (d->accumulate || d->b_idx || d->c_idx) return false;
  if (d->a_sm != 1 || d->b_sm != 1 || d->c_sm != 1) return false;
  if (d->n_modes % 8 != 0 || d->n_modes >= ((int64_t)1 << 31)) return false;
  if ((d->a_sg || d->b_sg || d->c_sg) && d->n_modes % 16 != 0) return false;        // tiled operands: groups of 16
  if ((d->a_sg | d->b_sg | d->c_sg) & 1) return false;
  // 16-byte granules: every row / column of every operand must start on an even complex element
  if ((d->a_sp | d->a_sr | d->b_sr | d->b_sq | d->c_sp | d->c_sq) & 1) return false;
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) return false;
  // tiles are 32 rows x 32 columns: take problems that fill them to >= 1/2 (SC_G8_FILL4 quarters; round 2: 3/4).  The
  // ragged 36 x 36 per-mode products of the Tucker chain at configs[2] (two or four tiles, 56 % / 32 % filled) take
  // 24 / 25 / 39 us here against 57 / 57 / 65 us on the register-staged k_modegemm_mfma
  // (profiles/r03_tfno_kernel_stats_g8fill2.txt): the operand stream, not the matrix pipe, is what a tile costs
  const int64_t cols = 32;
  const int64_t Pp = (d->P + 31) / 32 * 32, Qp = (d->Q + cols - 1) / cols * cols;
  static const int64_t fill4 = [] { const char* e = SC_DIAG_ENV("SC_G8_FILL4"); return e ? (int64_t)std::atoi(e) : (int64_t)2; }();
  bool rows_ok = 4 * d->P >= fill4 * Pp;
  // a small batch against a weight read ACROSS its rows (the gradient of the spectrum: B[r, q] = W[q, r], q stride >
  // r stride): the lanes-are-modes VALU kernel gathers 512-byte pieces of W there (FNO3d 128^3, B = 8: 115 us), the
  // streamed kernel does not care (55 us) although 32 / P of its matrix work is spent on clamped duplicate rows.  Not
  // for the forward product (VALU 45 us, streamed 53 us) and not below 8 rows (B = 4 at 1024^2 / hidden 128: 1.09 ->
  // 1.50 ms): profiles/r02_gemm_small_batch_ab.txt
  if (d->P >= 8 && d->P <= 32 && d->b_sq > d->b_sr) rows_ok = true;
  if (!rows_ok || 4 * d->Q < fill4 * Qp) return false;
  if (d->R < 4) return false;
  if (Pp / 32 * (Qp / cols) * (d->n_modes / 8) >= ((int64_t)1 << 30)) return false;
  return true;
}

template <int GS, int QT, int SUB, int D, bool IL>
static void launch_gemm8(const Gemm8Args& g, int ca, int cb, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  sc_conj_dispatch(ca, cb, [&](auto CA, auto CB) {
    SC_LAUNCH((k_modegemm_dma<GS, QT, SUB, D, IL, decltype(CA)::value, decltype(CB)::value>), dim3((unsigned)g.G),
              dim3((Gemm8Cfg<GS, QT, SUB>::THREADS)), 0, st, g, A, B, C);
  });
}

// launch geometry of one contraction; `resident` = workgroups the launch may count on being co-resident
static bool gemm8_args(const sc_modegemm_desc* d, Gemm8Args& g, int64_t resident_narrow, int64_t resident_wide,
                       int force_shape /* -1: choose, 0: narrow, 1: wide */) {
  const int64_t cols = 32;
  const int64_t tiles = ((d->P + 31) / 32) * ((d->Q + cols - 1) / cols);
  bool wide;
  if (force_shape >= 0) wide = force_shape == 1;
  else {
#if defined(SC_G8_FORCE_NARROW)          // measurement builds only
    wide = false;
#elif defined(SC_G8_FORCE_WIDE)
    wide = d->n_modes % 16 == 0;
#else
    wide = d->n_modes % 16 == 0 && tiles >= 8;
#endif
  }
  const int64_t modes = wide ? 16 : 8;
  const int64_t resident = wide ? resident_wide : resident_narrow;
  g.P = (int)d->P; g.Q = (int)d->Q; g.R = (int)d->R;
  g.n_mg = (int)(d->n_modes / modes);
  g.n_pb = (int)((d->P + 31) / 32);
  g.n_qb = (int)((d->Q + cols - 1) / cols);
  g.a_sp = d->a_sp; g.a_sr = d->a_sr;
  g.b_sr = d->b_sr; g.b_sq = d->b_sq;
  g.c_sp = d->c_sp; g.c_sq = d->c_sq;
  g.a_sg = d->a_sg ? d->a_sg : 16;                            // groups of 16 modes (plain arrays: 16 apart)
  g.b_sg = d->b_sg ? d->b_sg : 16;
  g.c_sg = d->c_sg ? d->c_sg : 16;
  // cache policy (round 8).  C: non-temporal when nobody reads it next, write-through when the next kernel does.
  // Operands: a piece of A is read by the n_qb tiles of its (row block, mode group), a piece of B by the n_pb tiles of
  // its (column block, mode group) -- with ONE block on that side every piece has exactly one reader in the launch, and
  // if the caller also says the operand is cold (SC_GEMM_NT_A / _B) its requests are non-temporal.  An operand several
  // workgroups share, or one that an earlier kernel left in the caches, keeps the default: nt on re-read bytes costs time.
  // The 8-wave shape issues its requests between MFMAs and keeps the one request form it was tuned with.
  g.stream_c = (d->flags & SC_GEMM_STREAM_C) ? SC_ST_NT : ((d->flags & SC_GEMM_C_WT) ? SC_ST_WT : SC_ST_PLAIN);
  g.nt_a = (!wide && (d->flags & SC_GEMM_NT_A) && g.n_qb == 1) ? 1 : 0;
  g.nt_b = (!wide && (d->flags & SC_GEMM_NT_B) && g.n_pb == 1) ? 1 : 0;
  // tiles per workgroup: a launch a little larger than what the chip holds at once runs its tiles back to back
  // inside fewer workgroups instead of queueing a short second round
  const int64_t nblk = (int64_t)g.n_pb * g.n_qb;
  int64_t bpw = 1;
  if (g.n_mg <= resident && g.n_mg * nblk > resident) {
    bpw = nblk;
    for (int64_t b = 1; b <= nblk; ++b)
      if (g.n_mg * ((nblk + b - 1) / b) <= resident) {
        bpw = b;
        break;
      }
  }
  const int64_t cap = (d->flags >> 8) & 0xffff;               // SC_GEMM_GRID(n) doubles as "tiles per workgroup" (tests)
  if (cap > 0 && cap <= nblk) bpw = cap;
  g.bpw = (int)bpw;
  g.G = (int)(g.n_mg * ((nblk + bpw - 1) / bpw));
  return wide;
}

static int run_gemm8(const sc_modegemm_desc* d, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  Gemm8Args g;
  const bool wide = gemm8_args(d, g, SC_G8_RESIDENT(false), SC_G8_RESIDENT(true), -1);
  if (wide) launch_gemm8<SC_G8_WIDE>(g, d->conj_a, d->conj_b, A, B, C, st);
  else launch_gemm8<SC_G8_NARROW>(g, d->conj_a, d->conj_b, A, B, C, st);
  return sc_check_launch("k_modegemm_dma");
}

// The two contractions of a backward pass (and the bias gradient) as ONE launch of k_modegemm_dma_bwd
// (sc_kernels_gemm8.h): d0 = weight gradient (conj A), d1 = gradient of the spectrum (conj B).  Returns -1 when the
// pair does not qualify (the caller then launches them one after the other).
#ifndef SC_G8_PAIR_BPW                   // measurement builds: 0 = one tile per workgroup, 1 = all tiles of a mode group in
#define SC_G8_PAIR_BPW 0                 // one workgroup (both jobs), 2 = that for the weight gradient only
#endif
// geometry of the two jobs of k_modegemm_dma_bwd: the narrow shape, ONE tile per workgroup (the kernel puts the job
// with the longer workgroups first: many short workgroups at the end of the launch balance the CUs better than a
// second round of tiles run back to back; profiles/r07_pair_schedule_ab.txt)
static void gemm8_pair_args(const sc_modegemm_desc* d0, const sc_modegemm_desc* d1, Gemm8Args& g0, Gemm8Args& g1) {
  gemm8_args(d0, g0, SC_G8_RESIDENT(false), SC_G8_RESIDENT(true), 0);
  gemm8_args(d1, g1, SC_G8_RESIDENT(false), SC_G8_RESIDENT(true), 0);
  for (Gemm8Args* g : {&g0, &g1}) {
    g->bpw = 1;
    g->G = (int)((int64_t)g->n_mg * g->n_pb * g->n_qb);
  }
#if SC_G8_PAIR_BPW >= 1
  g0.bpw = g0.n_pb * g0.n_qb; g0.G = g0.n_mg;
#endif
#if SC_G8_PAIR_BPW == 1
  g1.bpw = g1.n_pb * g1.n_qb; g1.G = g1.n_mg;
#endif
}

static int run_gemm8_bwd(const sc_modegemm_desc* d0, const cf32* A0, const cf32* B0, cf32* C0,
                         const sc_modegemm_desc* d1, const cf32* A1, const cf32* B1, cf32* C1,
                         const Gemm8Bias& bias, sc_stream_t st) {
#ifdef SC_G8_NO_PAIR                     // measurement builds only: the round-1 sequence of launches
  return -1;
#endif
  if (!gemm8_eligible(d0, A0, B0, C0) || !gemm8_eligible(d1, A1, B1, C1)) return -1;
  if (!(d0->conj_a && !d0->conj_b && !d1->conj_a && d1->conj_b)) return -1;
  if (d0->n_modes != d1->n_modes) return -1;
  // the narrow shape (3 workgroups per CU) for both jobs: the wide one wins on a weight gradient alone but loses
  // inside a step, and one kernel has one shape
  Gemm8Args g0, g1;
#ifdef SC_G8_PAIR_NARROW_ONLY            // measurement builds: pair only what would run the narrow shape anyway
  if (gemm8_args(d0, g0, SC_G8_RESIDENT(false), SC_G8_RESIDENT(true), -1) ||
      gemm8_args(d1, g1, SC_G8_RESIDENT(false), SC_G8_RESIDENT(true), -1)) return -1;
#endif
  gemm8_pair_args(d0, d1, g0, g1);
  if ((g0.G & 7) || (g1.G & 7)) return -1;                    // the jobs are laid out in octets of workgroups
  typedef Gemm8Cfg<4, 2, 2> K;
  const int64_t nb = bias.ghat ? (bias.channels + K::NW - 1) / K::NW : 0;
  if ((int64_t)g0.G + g1.G + nb >= ((int64_t)1 << 30)) return -1;
  SC_LAUNCH((k_modegemm_dma_bwd<SC_G8_NARROW>), dim3((unsigned)(g0.G + g1.G + nb)), dim3(K::THREADS), 0, st,
            g0, A0, B0, C0, g1, A1, B1, C1, bias);
  return sc_check_launch("k_modegemm_dma_bwd");
}

extern "C" int sc_modegemm(const sc_modegemm_desc* d, const float* A, const float* B, float* C,
                           void* stream) {
  SC_CHECK_ARG(d && A && B && C, "null argument");
  SC_CHECK_ARG(d->P >= 0 && d->Q >= 0 && d->R >= 0 && d->n_modes >= 0, "negative extent");
  if (d->P == 0 || d->Q == 0 || d->n_modes == 0) return 0;
  SC_CHECK_ARG(d->R > 0, "R must be > 0");
  ModeGemmArgs g;
  g.P = d->P; g.Q = d->Q; g.R = d->R; g.M = d->n_modes;
  g.a_sp = d->a_sp; g.a_sr = d->a_sr; g.a_sm = d->a_sm;
  g.b_sr = d->b_sr; g.b_sq = d->b_sq; g.b_sm = d->b_sm;
  g.c_sp = d->c_sp; g.c_sq = d->c_sq; g.c_sm = d->c_sm;
  g.b_idx = d->b_idx; g.c_idx = d->c_idx;
  g.accumulate = d->accumulate;
  SC_CHECK_ARG(((g.M + 63) / 64) * ((g.P + 15) / 16) * ((g.Q + 3) / 4) < ((int64_t)1 << 30),
               "problem too large for one launch grid");
  sc_stream_t st = (sc_stream_t)stream;
  const cf32* a = (const cf32*)A;
  const cf32* b = (const cf32*)B;
  cf32* c = (cf32*)C;
  if (d->flags & SC_GEMM_F16) {
    SC_CHECK_ARG(!d->accumulate && !(d->a_sg || d->b_sg || d->c_sg), "SC_GEMM_F16: plain C = A B launches only");
    g.n_mt = (int)((g.M + SC_WAVE - 1) / SC_WAVE);
    g.n_pg = (int)((g.P + 15) / 16);
    g.n_qt = (int)((g.Q + 3) / 4);
    g.per_xcd = 0;
    const dim3 grid((unsigned)((int64_t)g.n_mt * g.n_pg * g.n_qt));
    sc_conj_dispatch(d->conj_a, d->conj_b, [&](auto CA, auto CB) {
      SC_LAUNCH((k_modegemm_f16<decltype(CA)::value, decltype(CB)::value>), grid, dim3(SC_BLOCK), 0, st, g, a, b, c);
    });
    return sc_check_launch("k_modegemm_f16");
  }
  if (fmx_bfac_eligible(d)) return run_fmx_bfac(d, a, b, c, st);
  if (bfac_gemm_eligible(d)) {
    const int rc = run_bfac_gemm(d, a, b, c, st);
    if (rc >= 0) return rc;
  }
  if (sb_gemm_eligible(d, A, B, C)) {
    const int rc = run_sb_gemm(d, a, b, c, st);
    if (rc >= 0) return rc;
  }
  if (gemm8_eligible(d, A, B, C)) return run_gemm8(d, a, b, c, st);
  SC_CHECK_ARG(!(d->a_sg || d->b_sg || d->c_sg),
               "tiled operands (a_sg / b_sg / c_sg) need the streamed matrix-core kernel: n_modes % 16 == 0, unit mode "
               "strides, no index tables, 16-byte aligned rows, near-full 32 x 32 tiles");
  if (!(d->flags & SC_GEMM_FORCE_VALU) && mfma_gemm_eligible(d))
    return run_mfma_gemm(d, a, b, c, st);
  if (g.Q > 4) return launch_modegemm<4, 8>(g, d->conj_a, d->conj_b, a, b, c, st);
  return launch_modegemm<4, 4>(g, d->conj_a, d->conj_b, a, b, c, st);
}

extern "C" int sc_modegemm_path(const sc_modegemm_desc* d) {
  if (!d) return 0;
  if (fmx_bfac_eligible(d)) return 5;
  if (bfac_gemm_eligible(d)) return 4;
  if (sb_gemm_eligible(d, nullptr, nullptr, nullptr)) return 3;
  if (gemm8_eligible(d, nullptr, nullptr, nullptr)) return 2;
  return !(d->flags & SC_GEMM_FORCE_VALU) && mfma_gemm_eligible(d) ? 1 : 0;
}

extern "C" int sc_modegemm_policy(const sc_modegemm_desc* d) {
  if (!d || sc_modegemm_path(d) != 2) return -1;
  Gemm8Args g;
  gemm8_args(d, g, SC_G8_RESIDENT(false), SC_G8_RESIDENT(true), -1);
  return g.stream_c | (g.nt_a << 2) | (g.nt_b << 3);
}

extern "C" int sc_modegemm_uses_matrix_cores(const sc_modegemm_desc* d) {
  const int path = sc_modegemm_path(d);
  return path == 1 || path == 2;
}

extern "C" int sc_modegemm_pair(const sc_modegemm_desc* d0, const float* A0, const float* B0, float* C0,
                                const sc_modegemm_desc* d1, const float* A1, const float* B1, float* C1,
                                void* stream) {
  SC_CHECK_ARG(d0 && d1 && A0 && B0 && C0 && A1 && B1 && C1, "null argument");
  if (d0->P > 0 && d0->Q > 0 && d0->R > 0 && d0->n_modes > 0 && d1->P > 0 && d1->Q > 0 && d1->R > 0) {
    Gemm8Bias nobias;
    std::memset(&nobias, 0, sizeof(nobias));
    int rc = run_sb_bwd(d0, (const cf32*)A0, (const cf32*)B0, (cf32*)C0, d1, (const cf32*)A1, (const cf32*)B1, (cf32*)C1,
                        (sc_stream_t)stream);
    if (rc >= 0) return rc;
    rc = run_gemm8_bwd(d0, (const cf32*)A0, (const cf32*)B0, (cf32*)C0, d1, (const cf32*)A1,
                       (const cf32*)B1, (cf32*)C1, nobias, (sc_stream_t)stream);
    if (rc >= 0) return rc;
  }
  const int rc = sc_modegemm(d0, A0, B0, C0, stream);
  return rc ? rc : sc_modegemm(d1, A1, B1, C1, stream);
}

// which launch(es) a pair with 16-byte aligned operands (B0 and A1 the same array) takes: 2 = ONE pass over the weight
// (k_modegemm_sb_bwd), 1 = one launch of k_modegemm_dma_bwd, 0 = two launches
extern "C" int sc_modegemm_pair_path(const sc_modegemm_desc* d0, const sc_modegemm_desc* d1) {
  if (!d0 || !d1) return 0;
  static const float* const al = reinterpret_cast<const float*>(uintptr_t(256));   // alignment probe only
  if (sb_bwd_eligible(d0, al, al, al, d1, al, al, al)) return 2;
  return sc_modegemm_pair_fused(d0, d1) ? 1 : 0;
}

extern "C" int sc_modegemm_pair_fused(const sc_modegemm_desc* d0, const sc_modegemm_desc* d1) {
  if (!d0 || !d1) return 0;
#ifdef SC_G8_NO_PAIR
  return 0;
#else
  static const float* const al = reinterpret_cast<const float*>(uintptr_t(256));   // alignment probe only
  if (!gemm8_eligible(d0, al, al, al) || !gemm8_eligible(d1, al, al, al)) return 0;
  if (!(d0->conj_a && !d0->conj_b && !d1->conj_a && d1->conj_b) || d0->n_modes != d1->n_modes) return 0;
  Gemm8Args g0, g1;
  gemm8_pair_args(d0, d1, g0, g1);
  return !((g0.G & 7) || (g1.G & 7));
#endif
}

// launch geometry of k_modegemm_msum; returns the number of (mode split, r split) slots
static int64_t msum_geometry(ModeGemmArgs& g, bool* wide_out) {
  g.n_mt = (int)((g.M + SC_WAVE - 1) / SC_WAVE);
  // 4 x 8 outputs per wave (12 operand loads per 32 products) when the problem still yields enough workgroups,
  // 2 x 4 for small outputs
  const bool wide = g.P >= 16 && g.Q >= 8;
  const int PT = wide ? 4 : 2, QT = wide ? 8 : 4;
  g.n_pg = (int)((g.P + 4 * PT - 1) / (4 * PT));
  g.n_qt = (int)((g.Q + QT - 1) / QT);
  // mode splits: enough workgroups to fill the chip (~4096), as few partial sums per output as that allows
  int64_t splits = 4096 / ((int64_t)g.n_pg * g.n_qt);
  if (splits < 1) splits = 1;
  if (splits > g.n_mt) splits = g.n_mt;
  g.per_xcd = (int)splits;
  // when the mode tiles alone do not fill the chip (TFNO rank 0.1: 33 tiles x 20 output tiles = 660 workgroups, 2.8 waves
  // per SIMD, 45 % of the wave cycles issue-stalled: profiles/r03_tfno_pmc.txt) the reduction index is cut as well;
  // SC_MSUM_RSPLIT (environment, A-B) overrides
  static const int rsplit_env = [] { const char* e = SC_DIAG_ENV("SC_MSUM_RSPLIT"); return e ? std::atoi(e) : 0; }();
  int64_t rsplit = rsplit_env > 0 ? rsplit_env : 1;
  if (rsplit > g.R) rsplit = g.R;
  g.r_split = (int)rsplit;
  *wide_out = wide;
  return splits * rsplit;
}

template <bool PART>
static void launch_msum(const ModeGemmArgs& g0, int ca, int cb, const cf32* A, const cf32* B, cf32* C, sc_stream_t st) {
  ModeGemmArgs g = g0;
  bool wide;
  const int64_t total = msum_geometry(g, &wide) * g.n_pg * g.n_qt;
  sc_conj_dispatch(ca, cb, [&](auto CA, auto CB) {
    if (wide) SC_LAUNCH((k_modegemm_msum<4, 8, decltype(CA)::value, decltype(CB)::value, PART>), dim3((unsigned)total), dim3(SC_BLOCK), 0, st, g, A, B, C);
    else SC_LAUNCH((k_modegemm_msum<2, 4, decltype(CA)::value, decltype(CB)::value, PART>), dim3((unsigned)total), dim3(SC_BLOCK), 0, st, g, A, B, C);
  });
}

static void msum_args(const sc_modegemm_desc* d, ModeGemmArgs& g) {
  g.P = d->P; g.Q = d->Q; g.R = d->R; g.M = d->n_modes;
  g.a_sp = d->a_sp; g.a_sr = d->a_sr; g.a_sm = d->a_sm;
  g.b_sr = d->b_sr; g.b_sq = d->b_sq; g.b_sm = d->b_sm;
  g.c_sp = d->c_sp; g.c_sq = d->c_sq; g.c_sm = 0;
  g.b_idx = d->b_idx; g.c_idx = nullptr;
  g.accumulate = 1;
}

/* C[p,q] += sum_m sum_r opA(A[p,r,m]) opB(B[r,q,m]); C (strides c_sp, c_sq) zeroed by the caller */
extern "C" int sc_modegemm_msum(const sc_modegemm_desc* d, const float* A, const float* B, float* C,
                                void* stream) {
  SC_CHECK_ARG(d && A && B && C, "null argument");
  SC_CHECK_ARG(d->P >= 0 && d->Q >= 0 && d->R >= 0 && d->n_modes >= 0, "negative extent");
  if (d->P == 0 || d->Q == 0 || d->n_modes == 0 || d->R == 0) return 0;
  ModeGemmArgs g;
  msum_args(d, g);
  SC_CHECK_ARG(((g.P + 7) / 8) * ((g.Q + 3) / 4) < ((int64_t)1 << 30) && (g.M + 63) / 64 < ((int64_t)1 << 31),
               "problem too large for one launch grid");
  sc_stream_t st = (sc_stream_t)stream;
  const cf32* a = (const cf32*)A;
  const cf32* b = (const cf32*)B;
  cf32* c = (cf32*)C;
  launch_msum<false>(g, d->conj_a, d->conj_b, a, b, c, st);
  return sc_check_launch("k_modegemm_msum");
}

// C[p, q] = sum over modes and r (OVERWRITTEN, not accumulated) with a caller-provided workspace: the matrix-core
// kernel of sc_kernels_fmx.h where the problem qualifies, else k_modegemm_msum<PART>; one partial per workgroup /
// slot and a fixed-order reduction either way (bit-reproducible, unlike the atomics of sc_modegemm_msum)
static bool msum_slots_ok(const sc_modegemm_desc* d) {
  return ((d->P + 7) / 8) * ((d->Q + 3) / 4) < ((int64_t)1 << 30) && (d->n_modes + 63) / 64 < ((int64_t)1 << 31) &&
         d->P * d->Q < ((int64_t)1 << 31);
}
extern "C" size_t sc_modegemm_msum_workspace_bytes(const sc_modegemm_desc* d) {
  if (!d || d->P <= 0 || d->Q <= 0 || d->n_modes <= 0 || d->R <= 0) return 0;
  if (!fmx_msum_eligible(d)) {
    if (!msum_slots_ok(d)) return 0;
    ModeGemmArgs mg;
    msum_args(d, mg);
    bool wide;
    return (size_t)msum_geometry(mg, &wide) * (size_t)(d->P * d->Q) * sizeof(cf32) + 256;
  }
  FmxArgs g;
  size_t lds;
  fmx_msum_args(d, g, lds);
  return (size_t)g.n_wg * (size_t)(d->P * d->Q) * sizeof(cf32) + 256;
}

extern "C" int sc_modegemm_msum_path(const sc_modegemm_desc* d) {
  return d && d->P > 0 && d->Q > 0 && d->n_modes > 0 && d->R > 0 && fmx_msum_eligible(d) ? 1 : 0;
}

extern "C" int sc_modegemm_msum_ws(const sc_modegemm_desc* d, const float* A, const float* B, float* C, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  SC_CHECK_ARG(d && A && B && C && workspace, "null argument");
  SC_CHECK_ARG(d->P > 0 && d->Q > 0 && d->R > 0 && d->n_modes > 0, "empty extent");
  SC_CHECK_ARG(fmx_msum_eligible(d) || msum_slots_ok(d),
               "sc_modegemm_msum_ws: the problem does not qualify (sc_modegemm_msum_workspace_bytes == 0)");
  SC_CHECK_ARG(workspace_bytes >= sc_modegemm_msum_workspace_bytes(d), "workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  cf32* partial = (cf32*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const cf32* a = (const cf32*)A;
  const cf32* b = (const cf32*)B;
  if (!fmx_msum_eligible(d)) {
    ModeGemmArgs mg;
    msum_args(d, mg);
    bool wide;
    const int64_t slots = msum_geometry(mg, &wide);
    launch_msum<true>(mg, d->conj_a, d->conj_b, a, b, partial, st);
    int rc = sc_check_launch("k_modegemm_msum<slots>");
    if (rc) return rc;
    const int npc = (int)(d->P * d->Q);
    SC_LAUNCH(k_fmx_reduce, dim3((unsigned)((npc + 15) / 16)), dim3(16 * SC_FMX_RED_RG), 0, st, (const cf32*)partial, (int)slots, npc,
              (int)d->Q, (cf32*)C, d->c_sp, d->c_sq);
    return sc_check_launch("k_fmx_reduce");
  }
  FmxArgs g;
  size_t lds;
  fmx_msum_args(d, g, lds);
  const int64_t pa = (d->P + 3) / 4, pb = (d->Q + 3) / 4;
  int rc;
  if (pa <= 16 && pb <= 9 && d->Q <= 48) rc = run_fmx_msum_t<16, 9, 3>(d, g, lds, a, b, partial, st);
  else if (pa <= 9) rc = run_fmx_msum_t<9, 16, 4>(d, g, lds, a, b, partial, st);
  else rc = run_fmx_msum_t<16, 16, 4>(d, g, lds, a, b, partial, st);
  if (rc) return rc;
  const int npc = (int)(d->P * d->Q);
  SC_LAUNCH(k_fmx_reduce, dim3((unsigned)((npc + 15) / 16)), dim3(16 * SC_FMX_RED_RG), 0, st, (const cf32*)partial, g.n_wg, npc, (int)d->Q,
            (cf32*)C, d->c_sp, d->c_sq);
  return sc_check_launch("k_fmx_reduce");
}
