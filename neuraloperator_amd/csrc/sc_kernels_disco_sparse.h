// sc_kernels_disco_sparse.h -- the discrete-continuous convolution on point clouds (DiscreteContinuousConv2d and its
// transpose): a sparse Psi applied to point-major data, then a small dense contraction with the weight.
//
//   Xq[i][b][c]     = q[i] x[b][c][i]                                             k_dsp_pack        (LDS tile transpose)
//   Z[o][b][k][c]   = sum_e v_e Xq[i_e][b][c],  e over row (o, k) of the CSR      k_dsp_spmm        (one wave per row)
//   out2[o][b][oc]  = sum_{k, c in group} Z[o][b][k][c] weight[oc][c][k]          k_dsp_contract
//   out[b][oc][o]   = out2[o][b][oc] + bias[oc]                                   k_dsp_unpack
// and back:  g2 = pack(g),  gZ = k_dsp_contract(g2, W2T),  gXq = k_dsp_spmm(transposed CSR, gZ),  gx = unpack(gXq) q,
// gW / gbias = fixed slices of rows in k_dsp_wgrad, reduced in slice order by k_dsp_wreduce.
//
// No float atomics; every sum runs in an order fixed by the descriptor and the CSR (entries in stored order, k before c,
// slices in slice order).  Every index read from a CSR array is range-checked before it addresses memory.  No register
// array is indexed at run time.
//
// Matrix-core route (groups = 1, c_in and c_out in {32, 64, 128}): the two contractions are one tiled GEMM kernel,
// k_dsp_gemm_mfma, and the weight gradient k_dsp_wgrad_mfma, both on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered
// fmaf chain); pack, unpack, the sparse product, the fold and the reduce are shared with the general route.
#pragma once
#include "sc_device.h"
#include "sc_kernels_mfma.h"

#define DSP_TP 64              // points / columns per side of a transpose tile
#define DSP_ROWS 32            // (o, b) rows per workgroup of the contraction
#define DSP_RPT (DSP_ROWS / 4) // rows a thread accumulates
#define DSP_CC 128             // reduction columns staged in LDS per round of the contraction
#define DSP_WG_OC 16           // output channels per workgroup of the weight gradient
#define DSP_WG_J 64            // (k, c) columns per workgroup of the weight gradient
#define DSP_WG_R 32            // rows staged per round of the weight gradient
#define DSPM_ROWS 128          // rows per workgroup of the matrix-core GEMM: 32 to a wave
#define DSPM_RC 32             // reduction values staged in LDS per round of the matrix-core GEMM
#define DSPM_WG_PAIRS 4        // row pairs in flight per trip of the matrix-core weight gradient

// ---- pack / unpack ----------------------------------------------------------------------------------------------------
// src (cols, n) channel-first -> dst [n][cols] point-major, times scale[i] where given
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_pack(const float* __restrict__ src, const float* __restrict__ scale,
                                                float* __restrict__ dst, const int n, const int cols) {
  SC_SHARED float tile[DSP_TP * (DSP_TP + 1)];
  const int i0 = SC_BID_X * DSP_TP, j0 = SC_BID_Y * DSP_TP, lo = SC_TID & 63, hi = SC_TID >> 6;
#pragma unroll 4
  for (int r = 0; r < DSP_TP / 4; ++r) {
    const int jl = hi + 4 * r, j = j0 + jl, i = i0 + lo;
    float v = 0.f;
    if (j < cols && i < n) v = src[(size_t)j * n + i] * (scale ? scale[i] : 1.f);
    tile[jl * (DSP_TP + 1) + lo] = v;
  }
  SC_SYNC();
#pragma unroll 4
  for (int r = 0; r < DSP_TP / 4; ++r) {
    const int il = hi + 4 * r, i = i0 + il, j = j0 + lo;
    if (j < cols && i < n) dst[(size_t)i * cols + j] = tile[lo * (DSP_TP + 1) + il];
  }
}

// src [n][cols] point-major -> dst (cols, n) channel-first, times scale[i] and plus bias[col % c] where given
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_unpack(const float* __restrict__ src, const float* __restrict__ scale,
                                                  const float* __restrict__ bias, float* __restrict__ dst, const int n,
                                                  const int cols, const int c) {
  SC_SHARED float tile[DSP_TP * (DSP_TP + 1)];
  const int i0 = SC_BID_X * DSP_TP, j0 = SC_BID_Y * DSP_TP, lo = SC_TID & 63, hi = SC_TID >> 6;
#pragma unroll 4
  for (int r = 0; r < DSP_TP / 4; ++r) {
    const int il = hi + 4 * r, i = i0 + il, j = j0 + lo;
    float v = 0.f;
    if (j < cols && i < n) v = src[(size_t)i * cols + j];
    tile[il * (DSP_TP + 1) + lo] = v;
  }
  SC_SYNC();
#pragma unroll 4
  for (int r = 0; r < DSP_TP / 4; ++r) {
    const int jl = hi + 4 * r, j = j0 + jl, i = i0 + lo;
    if (j < cols && i < n) {
      float v = tile[lo * (DSP_TP + 1) + jl];
      if (scale) v *= scale[i];
      if (bias) v += bias[j % c];
      dst[(size_t)j * n + i] = v;
    }
  }
}

// ---- sparse product ---------------------------------------------------------------------------------------------------
// A point-major operand seen as [outer][b][inner][c]: row r = outer * per + inner starts at outer * outer_s + inner * c,
// and its column j = b * c + cc lies at (j / c) * batch_s + j % c.  Xq, gXq: per = 1; Z, gZ: per = K.
struct DspSide {
  long long outer_s;
  int per, batch_s;
};
struct DspSpmmArgs {
  const int* splits;           // [rows + 1]
  const int* cols;             // [nnz]: rows of the source
  const float* vals;           // [nnz]
  const float* src;
  float* dst;
  DspSide s, d;
  int rows, src_rows, nnz, c, width;   // width = batch * c
};

SC_DEVICE size_t dsp_row_base(const DspSide& s, const int r, const int c) {
  const int o = r / s.per;
  return (size_t)o * (size_t)s.outer_s + (size_t)(r - o * s.per) * c;
}

// dst[row][j] = sum_e vals[e] src[cols[e]][j]: one wave per row whatever its length, lanes along the channels, entries in
// stored order; an empty row writes zeros
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_spmm(const DspSpmmArgs a) {
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const long long row64 = (long long)SC_BID_X * 4 + wave;
  if (row64 >= a.rows) return;                               // wave-uniform
  const int row = (int)row64;
  int lo = a.splits[row], hi = a.splits[row + 1];
  lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
  hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
  float* drow = a.dst + dsp_row_base(a.d, row, a.c);
#pragma unroll 1
  for (int j0 = 0; j0 < a.width; j0 += 64) {
    const int j = j0 + lane;
    const bool ok = j < a.width;
    const int b = ok ? j / a.c : 0, cc = ok ? j - b * a.c : 0;
    const size_t soff = (size_t)b * a.s.batch_s + cc;
    float acc = 0.f;
#pragma unroll 2
    for (int e = lo; e < hi; ++e) {
      const int col = a.cols[e];
      if (col < 0 || col >= a.src_rows) continue;            // wave-uniform
      const float v = a.vals[e];
      if (ok) acc = fmaf(v, a.src[dsp_row_base(a.s, col, a.c) + soff], acc);
    }
    if (ok) drow[(size_t)b * a.d.batch_s + cc] = acc;
  }
}

// ---- weight layouts ---------------------------------------------------------------------------------------------------
// weight (c_out, cg, K) -> W2[k][cl][oc] and W2T[ocl][k][c] (c = g cg + cl, oc = g og + ocl): what the lanes of the two
// contractions read contiguously
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_fold(const float* __restrict__ w, float* __restrict__ w2,
                                                float* __restrict__ w2t, const int c_out, const int cg, const int og,
                                                const int K) {
  const long long t = (long long)SC_BID_X * 256 + SC_TID, n = (long long)c_out * cg * K;
  if (t >= n) return;
  const int k = (int)(t % K), cl = (int)((t / K) % cg), oc = (int)(t / ((long long)K * cg));
  const int g = oc / og, ocl = oc - g * og, c_in = cg * (c_out / og);
  const float v = w[t];
  if (w2) w2[((size_t)k * cg + cl) * c_out + oc] = v;
  if (w2t) w2t[((size_t)ocl * K + k) * c_in + g * cg + cl] = v;
}

// ---- contraction ------------------------------------------------------------------------------------------------------
// out[row][j] = sum_{kk < KK} sum_{l < L} in[row][kk CI + grp(j) L + l] m[(kk L + l) NJ + j],  grp(j) = (j % jmod) / jdiv
//   forward:  in = Z, KK = K, CI = c_in, L = cg, NJ = c_out, grp(j) = j / og                 m = W2
//   data gradient:  in = g2, KK = 1, CI = c_out, L = og, NJ = K c_in, grp(j) = (j % c_in) / cg      m = W2T
// A workgroup owns DSP_ROWS rows and 64 columns j; the rows' operands pass through LDS DSP_CC columns at a time, a thread
// carries DSP_RPT rows of one column.  The sum of a column runs kk-major, l ascending.
struct DspContractArgs {
  const float* in;
  const float* m;
  float* out;
  long long rows;
  int KK, CI, L, NJ, jmod, jdiv;
};

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_contract(const DspContractArgs a) {
  SC_SHARED float zs[DSP_ROWS * DSP_CC];
  const int lane = SC_TID & 63, sub = SC_TID >> 6;
  const long long row0 = (long long)SC_BID_X * DSP_ROWS;
  const int j = SC_BID_Y * 64 + lane;
  const bool ok = j < a.NJ;
  const int first = ok ? ((j % a.jmod) / a.jdiv) * a.L : 0;  // the lane's first column of `in` within one kk
  const size_t in_w = (size_t)a.KK * a.CI;
  float acc[DSP_RPT];
#pragma unroll
  for (int r = 0; r < DSP_RPT; ++r) acc[r] = 0.f;
#pragma unroll 1
  for (int kk = 0; kk < a.KK; ++kk) {
#pragma unroll 1
    for (int c0 = 0; c0 < a.CI; c0 += DSP_CC) {
      const int cw = a.CI - c0 < DSP_CC ? a.CI - c0 : DSP_CC;
      SC_SYNC();
      for (int t = SC_TID; t < DSP_ROWS * DSP_CC; t += 256) {
        const int r = t / DSP_CC, cc = t - r * DSP_CC;
        const long long row = row0 + r;
        zs[t] = row < a.rows && cc < cw ? a.in[(size_t)row * in_w + (size_t)kk * a.CI + c0 + cc] : 0.f;
      }
      SC_SYNC();
      // the lane's own columns [first, first + L) cut to this round's [c0, c0 + cw)
      const int lo = first > c0 ? first : c0, hi = first + a.L < c0 + cw ? first + a.L : c0 + cw;
      if (ok) {
#pragma unroll 1
        for (int c = lo; c < hi; ++c) {
          const float w = a.m[((size_t)kk * a.L + (c - first)) * a.NJ + j];
          const float* z = zs + sub * DSP_RPT * DSP_CC + (c - c0);
#pragma unroll
          for (int r = 0; r < DSP_RPT; ++r) acc[r] = fmaf(z[r * DSP_CC], w, acc[r]);
        }
      }
    }
  }
  if (ok) {
#pragma unroll
    for (int r = 0; r < DSP_RPT; ++r) {
      const long long row = row0 + sub * DSP_RPT + r;
      if (row < a.rows) a.out[(size_t)row * a.NJ + j] = acc[r];
    }
  }
}

// ---- weight and bias gradient ------------------------------------------------------------------------------------------
// parts[s][oc][jj] = sum_{rows of slice s} g2[row][oc] Z[row][k c_in + g cg + cl],  jj = k cg + cl, and
// parts_b[s][oc] = sum_{rows of slice s} g2[row][oc], rows ascending.  Workgroup: (slice, group, 16 oc of the group, 64 jj);
// a thread carries 4 oc of one jj.  Z null: the bias sums alone.
struct DspWgArgs {
  const float* g2;             // [rows][c_out]
  const float* Z;              // [rows][K c_in]
  float* parts;                // [slices][c_out][K cg]
  float* parts_b;              // [slices][c_out]
  long long rows, per_slice;
  int c_in, c_out, cg, og, K, slices, oc_tiles, j_tiles;
};

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_wgrad(const DspWgArgs a) {
  SC_SHARED float gs[DSP_WG_R * DSP_WG_OC];
  SC_SHARED float zs[DSP_WG_R * DSP_WG_J];
  int id = SC_BID_X;
  const int jt = id % a.j_tiles;
  id /= a.j_tiles;
  const int ot = id % a.oc_tiles;
  id /= a.oc_tiles;
  const int g = id % (a.c_out / a.og), s = id / (a.c_out / a.og);
  const int lane = SC_TID & 63, sub = SC_TID >> 6;
  const int nj = a.K * a.cg, jj = jt * DSP_WG_J + lane;
  const bool jok = jj < nj && a.Z != nullptr;
  const int k = jok ? jj / a.cg : 0, cl = jok ? jj - k * a.cg : 0;
  const size_t zcol = (size_t)k * a.c_in + (size_t)g * a.cg + cl, zw = (size_t)a.K * a.c_in;
  const int ocl0 = ot * DSP_WG_OC;                           // first output channel of the tile within the group
  const long long r_lo = (long long)s * a.per_slice;
  const long long r_hi = r_lo + a.per_slice < a.rows ? r_lo + a.per_slice : a.rows;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f, bsum = 0.f;
#pragma unroll 1
  for (long long r0 = r_lo; r0 < r_hi; r0 += DSP_WG_R) {
    SC_SYNC();
    for (int t = SC_TID; t < DSP_WG_R * DSP_WG_OC; t += 256) {
      const int r = t / DSP_WG_OC, o = t - r * DSP_WG_OC;
      gs[t] = r0 + r < r_hi && ocl0 + o < a.og ? a.g2[(size_t)(r0 + r) * a.c_out + g * a.og + ocl0 + o] : 0.f;
    }
    if (a.Z) {
      for (int t = SC_TID; t < DSP_WG_R * DSP_WG_J; t += 256) {
        const int r = t / DSP_WG_J;                          // t % 64 == lane: the thread's own column
        zs[t] = r0 + r < r_hi && jok ? a.Z[(size_t)(r0 + r) * zw + zcol] : 0.f;
      }
    }
    SC_SYNC();
    if (a.Z) {
#pragma unroll 4
      for (int r = 0; r < DSP_WG_R; ++r) {
        const float z = zs[r * DSP_WG_J + lane];
        const float* gr = gs + r * DSP_WG_OC + sub * 4;
        acc0 = fmaf(gr[0], z, acc0);
        acc1 = fmaf(gr[1], z, acc1);
        acc2 = fmaf(gr[2], z, acc2);
        acc3 = fmaf(gr[3], z, acc3);
      }
    }
    if (jt == 0 && SC_TID < DSP_WG_OC) {
      for (int r = 0; r < DSP_WG_R; ++r) bsum += gs[r * DSP_WG_OC + SC_TID];
    }
  }
  if (jok) {
    const int o = ocl0 + sub * 4;
    float* p = a.parts + ((size_t)s * a.c_out + g * a.og + o) * nj + jj;
    if (o + 0 < a.og) p[0] = acc0;
    if (o + 1 < a.og) p[(size_t)nj] = acc1;
    if (o + 2 < a.og) p[2 * (size_t)nj] = acc2;
    if (o + 3 < a.og) p[3 * (size_t)nj] = acc3;
  }
  if (jt == 0 && SC_TID < DSP_WG_OC && ocl0 + SC_TID < a.og)
    a.parts_b[(size_t)s * a.c_out + g * a.og + ocl0 + SC_TID] = bsum;
}

// gw[oc][cl][k] = sum_s parts[s][oc][k cg + cl] and gbias[oc] = sum_s parts_b[s][oc], slices ascending
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_wreduce(const float* __restrict__ parts, const float* __restrict__ parts_b,
                                                   float* __restrict__ gw, float* __restrict__ gbias, const int c_out,
                                                   const int cg, const int K, const int slices) {
  const long long wn = (long long)c_out * cg * K, t = (long long)SC_BID_X * 256 + SC_TID;
  if (t < wn) {
    if (!gw) return;
    const int k = (int)(t % K), cl = (int)((t / K) % cg), oc = (int)(t / ((long long)K * cg));
    const size_t src = ((size_t)oc * K + k) * cg + cl;
    float acc = 0.f;
    for (int s = 0; s < slices; ++s) acc += parts[(size_t)s * wn + src];
    gw[t] = acc;
  } else if (t < wn + c_out && gbias) {
    const int oc = (int)(t - wn);
    float acc = 0.f;
    for (int s = 0; s < slices; ++s) acc += parts_b[(size_t)s * c_out + oc];
    gbias[oc] = acc;
  }
}

// ---- matrix-core route -------------------------------------------------------------------------------------------------
// C[M x N] = A[M x R] B[R x N], all row-major; R a multiple of DSPM_RC, a workgroup's 32 NOB columns inside N.
//   forward:        A = Z (lda = K c_in), B = W2 [k c][oc], C = out2, NOB = c_out / 32, one column group
//   data gradient:  A = g2 (lda = c_out), B = W2T [oc][k c], C = gZ, NOB = c_in / 32, K column groups
// A wave owns 32 rows and all 32 NOB columns of the group: lane l feeds A[l & 31][2 kk + (l >> 5)] and
// B[2 kk + (l >> 5)][l & 31] and holds D[(v & 3) + 8 (v >> 2) + 4 (l >> 5)][l & 31].  Both operands pass through LDS
// in coalesced rows; A's row stride of 33 keeps the 32 rows of a read on 32 banks.  A sum runs over r ascending.
struct DspGemmArgs {
  const float* A;
  const float* B;
  float* C;
  long long M;
  int R, lda, ldb, ldc;
};

template <int NOB>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_gemm_mfma(const DspGemmArgs a) {
  SC_SHARED float as[DSPM_ROWS * (DSPM_RC + 1)];
  SC_SHARED float bs[DSPM_RC * 32 * NOB];
  const int lane = SC_TID & 63, wave = SC_TID >> 6;
  const long long row0 = (long long)SC_BID_X * DSPM_ROWS;
  const int col0 = SC_BID_Y * 32 * NOB;
  sc_f32x16 acc[NOB];
#pragma unroll
  for (int u = 0; u < NOB; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[u][v] = 0.f;
#pragma unroll 1
  for (int r0 = 0; r0 < a.R; r0 += DSPM_RC) {
    SC_SYNC();
#pragma unroll 4
    for (int t = SC_TID; t < DSPM_ROWS * DSPM_RC; t += 256) {
      const int r = t >> 5, cc = t & 31;
      const long long row = row0 + r;
      as[r * (DSPM_RC + 1) + cc] = row < a.M ? a.A[(size_t)row * a.lda + r0 + cc] : 0.f;
    }
#pragma unroll 4
    for (int t = SC_TID; t < DSPM_RC * 32 * NOB; t += 256) {
      const int rr = t / (32 * NOB), j = t - rr * (32 * NOB);
      bs[t] = a.B[(size_t)(r0 + rr) * a.ldb + col0 + j];
    }
    SC_SYNC();
    const float* ap = as + (wave * 32 + (lane & 31)) * (DSPM_RC + 1) + (lane >> 5);
    const float* bp = bs + (lane >> 5) * (32 * NOB) + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < DSPM_RC / 2; ++kk) {
      const float av = ap[2 * kk];
#pragma unroll
      for (int u = 0; u < NOB; ++u) sc_mfma_32x32x2(acc[u], av, bp[2 * kk * (32 * NOB) + 32 * u]);
    }
  }
#pragma unroll
  for (int u = 0; u < NOB; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const long long row = row0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
      if (row < a.M) a.C[(size_t)row * a.ldc + col0 + 32 * u + (lane & 31)] = acc[u][v];
    }
}

// parts[s][oc][k c_in + c] = sum_{rows of slice s} g2[row][oc] Z[row][k c_in + c] and parts_b[s][oc] (even rows of the
// slice, then odd rows): a wave owns (slice, 32 oc, one k) and walks its rows two at a time, both operands straight from
// global memory in 128-byte segments.  Z null: the bias sums alone (kj = 1).
struct DspWgMArgs {
  const float* g2;
  const float* Z;
  float* parts;
  float* parts_b;
  long long rows, per_slice;
  int c_in, c_out, K, kj, slices;
};

template <int NOB>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_dsp_wgrad_mfma(const DspWgMArgs a) {
  SC_SHARED float red[256];
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int ots = a.c_out / 32;
  const long long job = (long long)SC_BID_X * 4 + wave;
  if (job >= (long long)a.slices * ots * a.kj) return;       // wave-uniform
  const int k = (int)(job % a.kj), ot = (int)((job / a.kj) % ots), s = (int)(job / ((long long)a.kj * ots));
  const long long r_lo = (long long)s * a.per_slice;
  const long long r_hi = r_lo + a.per_slice < a.rows ? r_lo + a.per_slice : a.rows;
  const size_t zw = (size_t)a.K * a.c_in;
  const float* gp = a.g2 + ot * 32 + (lane & 31);
  const float* zp = a.Z ? a.Z + (size_t)k * a.c_in + (lane & 31) : nullptr;
  sc_f32x16 acc[NOB];
#pragma unroll
  for (int u = 0; u < NOB; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[u][v] = 0.f;
  float bsum = 0.f;
  // four row pairs to a trip: their 4 (1 + NOB) loads are issued before the first matrix instruction needs one, in the
  // order of the rows, so the sums are those of one pair per trip
#pragma unroll 1
  for (long long base = r_lo; base < r_hi; base += 2 * DSPM_WG_PAIRS) {
    float av[DSPM_WG_PAIRS], bv[DSPM_WG_PAIRS][NOB];
#pragma unroll
    for (int t = 0; t < DSPM_WG_PAIRS; ++t) {
      const long long row = base + 2 * t + (lane >> 5);
      const bool ok = row < r_hi;
      av[t] = ok ? gp[(size_t)row * a.c_out] : 0.f;
#pragma unroll
      for (int u = 0; u < NOB; ++u) bv[t][u] = ok && zp ? zp[(size_t)row * zw + 32 * u] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < DSPM_WG_PAIRS; ++t) {
      bsum += av[t];
      if (zp) {                                              // wave-uniform
#pragma unroll
        for (int u = 0; u < NOB; ++u) sc_mfma_32x32x2(acc[u], av[t], bv[t][u]);
      }
    }
  }
  if (zp) {
#pragma unroll
    for (int u = 0; u < NOB; ++u)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int oc = ot * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
        a.parts[((size_t)s * a.c_out + oc) * zw + (size_t)k * a.c_in + 32 * u + (lane & 31)] = acc[u][v];
      }
  }
  if (k == 0) {
    red[SC_TID] = bsum;
    SC_WAVE_SYNC();
    if (lane < 32) a.parts_b[(size_t)s * a.c_out + ot * 32 + lane] = red[wave * 64 + lane] + red[wave * 64 + lane + 32];
  }
}
