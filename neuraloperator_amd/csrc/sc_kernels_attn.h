// sc_kernels_attn.h -- the attention kernel integral (AttentionKernelIntegral, associative form) in fused passes over
// the raw [B, N, H D] outputs of the q / k / v projections; the kernels do the head split, no permuted copy exists.
//
//   kn = LN_D(k), vn = LN_D(v)     per point and head over the D head channels (biased variance, eps 1e-5, no affine):
//                                  what the reference's InstanceNorm1d on its [B H, N, D] view really computes
//   kr = R(pos_src) kn, qr = R(pos_qry) q                                        rotary embedding, per point
//   dots[b, h] = sum_n kr[n]^T vn[n]                 k_attn_outer (partials per chunk of points) + k_attn_reduce
//   u[n]       = (qr[n] dots[b, h]) w[n]             k_attn_apply
// and back, recomputing instead of saving anything of B N H D floats:
//   g = w g_u;   g_q = R^T (g dots^T)                k_attn_apply on dots^T
//   g_dots = sum_n qr[n]^T g[n]                      k_attn_outer + k_attn_reduce
//   g_vn = kr g_dots,  g_kn = R^T (vn g_dots^T),  then the layer-norm backward of each      k_attn_kv_bwd
//
// One lane layout for every even D <= 128 (DP = D rounded up to 32, 64 or 128): a workgroup stages a tile of TP points
// of one (batch, head) in LDS, row stride DP + 1; the layer norm is TP points x 256 / TP sub-lanes with the sub-lane
// partials added in sub-lane order; a product with a D x D matrix gives a thread one output channel of TP DP / 256
// points; the outer-product sum gives it one column and DP DP / 256 rows of the D x D partial.
// No float atomics: a chunk's sum runs over its points in ascending order, the chunks are added in chunk order.  No
// register array is indexed at run time.  Rows past the end of a tile are zeros and add exactly nothing.
#pragma once
#include "sc_device.h"
#include "sc_kernels_mfma.h"
#ifdef SC_EMU
#include <math.h>
#endif

#define ATT_CHUNK 256          // points of one partial of a D x D sum
#define ATT_EPS 1e-5f

struct AttGeom {
  int n;                       // points per batch of the operand the kernel walks
  int heads, D, rotary;        // rotary: 0 none, 1 / 2 = position dimension
  float rot_scale;             // fl32(scale / min_freq) of the embedding module
  float wconst;                // 1 / n_src where no weights are given
};

// tile[p][c] = src[row0 + p][hoff + c] (times the point's weight where scaled): zeros past np points and D channels
template <int TP, int DP>
SC_DEVICE void att_load(float* tile, const float* __restrict__ src, const size_t row0, const int np, const int hd,
                        const int hoff, const int D, const bool scaled, const float* __restrict__ wrow,
                        const float wconst) {
#pragma unroll 4
  for (int t = SC_TID; t < TP * DP; t += 256) {
    const int p = t / DP, c = t - p * DP;
    float v = 0.f;
    if (p < np && c < D) {
      v = src[(row0 + p) * (size_t)hd + hoff + c];
      if (scaled) v *= wrow ? wrow[p] : wconst;
    }
    tile[p * (DP + 1) + c] = v;
  }
}

template <int TP, int DP>
SC_DEVICE void att_store(const float* tile, float* __restrict__ dst, const size_t row0, const int np, const int hd,
                         const int hoff, const int D) {
#pragma unroll 4
  for (int t = SC_TID; t < TP * DP; t += 256) {
    const int p = t / DP, c = t - p * DP;
    if (p < np && c < D) dst[(row0 + p) * (size_t)hd + hoff + c] = tile[p * (DP + 1) + c];
  }
}

// the layer norm of every row of the tile in place, 1 / sqrt(var + eps) of the rows to rstd; ends on a barrier
template <int TP, int DP>
SC_DEVICE void att_norm(float* tile, float* red, float* rstd, const int D) {
  constexpr int S = 256 / TP;
  const int p = SC_TID / S, s = SC_TID - p * S;
  float* row = tile + p * (DP + 1);
  const float inv_d = 1.f / (float)D;
  float a = 0.f;
  for (int c = s; c < D; c += S) a += row[c];
  red[SC_TID] = a;
  SC_SYNC();
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) m += red[p * S + i];
  m *= inv_d;
  SC_SYNC();
  float q = 0.f;
  for (int c = s; c < D; c += S) {
    const float d = row[c] - m;
    q = fmaf(d, d, q);
  }
  red[SC_TID] = q;
  SC_SYNC();
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) var += red[p * S + i];
  const float r = 1.f / sqrtf(fmaf(var, inv_d, ATT_EPS));
  for (int c = s; c < D; c += S) row[c] = (row[c] - m) * r;
  if (s == 0) rstd[p] = r;
  SC_SYNC();
}

// The backward of att_norm row by row: g <- r (g - mean(g) - xn mean(g xn)) with xn = (x - mean) r recomputed from the raw
// rows x in global memory, statistics and combination in float64.  The difference cancels to a relative 1e-5 / var of
// its terms where the centred channels span little more than xn itself (exactly so at D = 2): in fp32 the rounding of xn
// alone is then a per-cent error of the gradient.  Ends on a barrier.
template <int TP, int DP>
SC_DEVICE void att_norm_bwd(float* g, const float* __restrict__ src, const size_t row0, const int np, const int hd,
                            const int hoff, double* red, const int D) {
  constexpr int S = 256 / TP;
  const int p = SC_TID / S, s = SC_TID - p * S;
  float* grow = g + p * (DP + 1);
  const float* xrow = src + (row0 + (p < np ? p : 0)) * (size_t)hd + hoff;
  const int Dp = p < np ? D : 0;                             // rows past the end stay zeros
  const double inv_d = 1.0 / (double)D;
  double a = 0.0, b = 0.0;
  for (int c = s; c < Dp; c += S) a += (double)xrow[c];
  red[SC_TID] = a;
  SC_SYNC();
  double mu = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) mu += red[p * S + i];
  mu *= inv_d;
  SC_SYNC();
  a = 0.0;
  for (int c = s; c < Dp; c += S) {
    const double d = (double)xrow[c] - mu;
    a = fma(d, d, a);
  }
  red[SC_TID] = a;
  SC_SYNC();
  double var = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) var += red[p * S + i];
  const double r = 1.0 / sqrt(fma(var, inv_d, 1e-5));
  SC_SYNC();
  a = 0.0;
  for (int c = s; c < Dp; c += S) {
    const double gc = (double)grow[c];
    a += gc;
    b = fma(gc, ((double)xrow[c] - mu) * r, b);
  }
  red[SC_TID] = a;
  red[256 + SC_TID] = b;
  SC_SYNC();
  double m1 = 0.0, m2 = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    m1 += red[p * S + i];
    m2 += red[256 + p * S + i];
  }
  m1 *= inv_d;
  m2 *= inv_d;
  for (int c = s; c < Dp; c += S)
    grow[c] = (float)(r * (((double)grow[c] - m1) - ((double)xrow[c] - mu) * r * m2));
  SC_SYNC();
}

// the rotary embedding of every row in place: dir = 1 applies R, dir = -1 its transpose.  Pair j of a row is channels
// (a, a + Q), Q = D / (2 rotary) pairs to an axis, a = 2 Q axis + i; the angle is the reference's two fp32 products
// (coordinate scale) inv_freq[i], its sine and cosine the accurate ones.  Ends on a barrier where it rotates.
template <int TP, int DP>
SC_DEVICE void att_rotate(float* tile, const float* __restrict__ pos, const int np, const AttGeom& g,
                          const float* __restrict__ inv_freq, const float dir) {
  if (g.rotary == 0) return;                                 // uniform over the launch
  const int half = g.D >> 1, Q = half / g.rotary;
  for (int t = SC_TID; t < TP * half; t += 256) {
    const int p = t / half, j = t - p * half;
    if (p >= np) continue;
    const int ax = j / Q, i = j - ax * Q;
    const float ang = (pos[p * g.rotary + ax] * g.rot_scale) * inv_freq[i];
    float sn, cs;
    sincosf(ang, &sn, &cs);
    sn *= dir;
    float* a = tile + p * (DP + 1) + 2 * Q * ax + i;
    const float x1 = a[0], x2 = a[Q];
    a[0] = x1 * cs - x2 * sn;
    a[Q] = x2 * cs + x1 * sn;
  }
  SC_SYNC();
}

// acc[r] = sum_i tile[pg PR + r][i] M[i][j]: the thread's channel j = tid % DP of its PR = TP DP / 256 points, i ascending
template <int TP, int DP>
SC_DEVICE void att_apply(const float* tile, const float* __restrict__ M, const int D, float (&acc)[TP * DP / 256]) {
  constexpr int PR = TP * DP / 256;
  const int j = SC_TID % DP, pg = SC_TID / DP;
  const float* x = tile + pg * PR * (DP + 1);
#pragma unroll
  for (int r = 0; r < PR; ++r) acc[r] = 0.f;
  if (j < D) {
#pragma unroll 4
    for (int i = 0; i < D; ++i) {
      const float m = M[(size_t)i * D + j];
#pragma unroll
      for (int r = 0; r < PR; ++r) acc[r] = fmaf(x[r * (DP + 1) + i], m, acc[r]);
    }
  }
}

template <int TP, int DP>
SC_DEVICE void att_put(float* tile, const float (&acc)[TP * DP / 256], const float scale) {
  constexpr int PR = TP * DP / 256;
  const int j = SC_TID % DP, pg = SC_TID / DP;
#pragma unroll
  for (int r = 0; r < PR; ++r) tile[(pg * PR + r) * (DP + 1) + j] = acc[r] * scale;
}

// ---- matrix-core forms (D = DP in {32, 64, 128}): v_mfma_f32_32x32x2_f32, exact fp32, a k-ordered fmaf chain --------------
// lane l feeds A[l & 31][l >> 5] and B[l >> 5][l & 31] and holds D[(v & 3) + 8 (v >> 2) + 4 (l >> 5)][l & 31], v = 0..15
SC_DEVICE int att_mrow(const int v, const int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }

// acc += A^T B over the points of a 32-point tile, two points to an instruction, points ascending.  D = 32: one 32 x 32
// block, wave w takes points 8 w .. 8 w + 7 (the waves' sums meet in wave order at the end of the kernel); D = 64: four
// blocks, one to a wave; D = 128: sixteen blocks, wave w takes row block w and all four column blocks
template <int DP>
SC_DEVICE void att_outer_mfma(const float* ta, const float* tb, sc_f32x16 (&acc)[DP == 128 ? 4 : 1]) {
  constexpr int NB = DP / 32, NACC = NB == 4 ? 4 : 1, DS = DP + 1;
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int ib = NB == 1 ? 0 : (NB == 2 ? wave >> 1 : wave), jb0 = NB == 2 ? (wave & 1) : 0;
  const int p0 = NB == 1 ? 8 * wave : 0, p1 = NB == 1 ? p0 + 8 : 32;
  const float* ap = ta + (lane >> 5) * DS + ib * 32 + (lane & 31);
  const float* bp = tb + (lane >> 5) * DS + jb0 * 32 + (lane & 31);
#pragma unroll 4
  for (int p = p0; p < p1; p += 2) {
    const float a = ap[p * DS];
#pragma unroll
    for (int u = 0; u < NACC; ++u) sc_mfma_32x32x2(acc[u], a, bp[p * DS + 32 * u]);
  }
}

// acc = tile M for a tile of TP = 128 points (64 at D = 128): wave w owns the 32 points of block w / WPB and NJ column
// blocks of 32, WPB = 128 / TP waves to a point block; the matrix rows come from global memory, 128 bytes to a half wave
#define ATT_MTP(DP) ((DP) == 128 ? 64 : 128)
#define ATT_MNJ(DP) ((DP) / 32 * ATT_MTP(DP) / 128)
template <int DP>
SC_DEVICE void att_apply_mfma(const float* tile, const float* __restrict__ M, sc_f32x16 (&acc)[ATT_MNJ(DP)]) {
  constexpr int TP = ATT_MTP(DP), WPB = 128 / TP, NJ = ATT_MNJ(DP), DS = DP + 1;
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int pb = wave / WPB, jb0 = (wave % WPB) * NJ;
#pragma unroll
  for (int u = 0; u < NJ; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[u][v] = 0.f;
  const float* xp = tile + (pb * 32 + (lane & 31)) * DS + (lane >> 5);
  const float* mp = M + (size_t)(lane >> 5) * DP + jb0 * 32 + (lane & 31);
#pragma unroll 4
  for (int kk = 0; kk < DP / 2; ++kk) {
    const float a = xp[2 * kk];
#pragma unroll
    for (int u = 0; u < NJ; ++u) sc_mfma_32x32x2(acc[u], a, mp[(size_t)(2 * kk) * DP + 32 * u]);
  }
}

template <int DP>
SC_DEVICE void att_put_mfma(float* tile, const sc_f32x16 (&acc)[ATT_MNJ(DP)]) {
  constexpr int TP = ATT_MTP(DP), WPB = 128 / TP, NJ = ATT_MNJ(DP), DS = DP + 1;
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int pb = wave / WPB, jb0 = (wave % WPB) * NJ;
#pragma unroll
  for (int u = 0; u < NJ; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) tile[(pb * 32 + att_mrow(v, lane)) * DS + (jb0 + u) * 32 + (lane & 31)] = acc[u][v];
}

// ---- D x D sums over points -------------------------------------------------------------------------------------------
// parts[bh][chunk][i][j] = sum over the chunk's points of A[n][i] B[n][j]:
//   mode 0  A = R LN(k), B = LN(v)          (forward: the partials of dots)
//   mode 1  A = R q,     B = w g_u          (backward: the partials of g_dots)
struct AttOuterArgs {
  const float* a;              // [B, n, H D]
  const float* b;              // [B, n, H D]
  const float* pos;            // [B, n, rotary], null without rotary
  const float* inv_freq;
  const float* weights;        // mode 1: [B, n] or null
  float* parts;                // [B H][chunks][D][D]
  AttGeom g;
  int chunks, mode;
};

template <int DP, bool MF>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_attn_outer(const AttOuterArgs a) {
  constexpr int TP = 32, DS = DP + 1, R = MF ? 1 : DP * DP / 256, NACC = MF ? (DP == 128 ? 4 : 1) : 1;
  SC_SHARED float ta[TP * DS];
  SC_SHARED float tb[TP * DS];
  SC_SHARED float red[256];
  SC_SHARED float rstd[TP];
  SC_SHARED float comb[MF && DP == 32 ? 4 * 1024 : 1];
  sc_f32x16 macc[NACC];
#pragma unroll
  for (int u = 0; u < NACC; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) macc[u][v] = 0.f;
  const int bh = SC_BID_Y, b = bh / a.g.heads, h = bh - b * a.g.heads, ch = SC_BID_X;
  const int D = a.g.D, hd = a.g.heads * D, hoff = h * D;
  const int n_lo = ch * ATT_CHUNK, n_hi = n_lo + ATT_CHUNK < a.g.n ? n_lo + ATT_CHUNK : a.g.n;
  const int j = SC_TID % DP, ig = SC_TID / DP;
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll 1
  for (int n0 = n_lo; n0 < n_hi; n0 += TP) {
    const int np = n_hi - n0 < TP ? n_hi - n0 : TP;
    const size_t row0 = (size_t)b * a.g.n + n0;
    SC_SYNC();
    att_load<TP, DP>(ta, a.a, row0, np, hd, hoff, D, false, nullptr, 0.f);
    att_load<TP, DP>(tb, a.b, row0, np, hd, hoff, D, a.mode == 1, a.weights ? a.weights + row0 : nullptr, a.g.wconst);
    SC_SYNC();
    if (a.mode == 0) {
      att_norm<TP, DP>(ta, red, rstd, D);
      att_norm<TP, DP>(tb, red, rstd, D);
    }
    att_rotate<TP, DP>(ta, a.pos ? a.pos + row0 * a.g.rotary : nullptr, np, a.g, a.inv_freq, 1.f);
    if constexpr (MF) {
      att_outer_mfma<DP>(ta, tb, macc);
    } else {
      const float* ap = ta + ig * R;
#pragma unroll 2
      for (int p = 0; p < TP; ++p) {
        const float bj = tb[p * DS + j];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(ap[p * DS + r], bj, acc[r]);
      }
    }
  }
  if constexpr (MF) {
    constexpr int NB = DP / 32;
    const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
    float* out = a.parts + ((size_t)bh * a.chunks + ch) * DP * DP;
    if constexpr (NB == 1) {                                 // the four waves' shares of the points, in wave order
#pragma unroll
      for (int v = 0; v < 16; ++v) comb[wave * 1024 + att_mrow(v, lane) * 32 + (lane & 31)] = macc[0][v];
      SC_SYNC();
      for (int t = SC_TID; t < 1024; t += 256) out[t] = ((comb[t] + comb[1024 + t]) + comb[2048 + t]) + comb[3072 + t];
    } else {
      const int ib = NB == 2 ? wave >> 1 : wave, jb0 = NB == 2 ? (wave & 1) : 0;
#pragma unroll
      for (int u = 0; u < NACC; ++u)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          out[(size_t)(ib * 32 + att_mrow(v, lane)) * DP + (jb0 + u) * 32 + (lane & 31)] = macc[u][v];
    }
  } else if (j < D) {
    float* out = a.parts + ((size_t)bh * a.chunks + ch) * D * D + j;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (ig * R + r < D) out[(size_t)(ig * R + r) * D] = acc[r];
  }
}

// M[bh][i][j] = sum_chunk parts[bh][chunk][i][j], chunks ascending; MT, where given, its transpose per (batch, head)
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_attn_reduce(const float* __restrict__ parts, float* __restrict__ M,
                                                   float* __restrict__ MT, const int D, const int chunks,
                                                   const long long total) {
  const long long t = (long long)SC_BID_X * 256 + SC_TID;
  if (t >= total) return;
  const int dd = D * D;
  const long long bh = t / dd;
  const int e = (int)(t - bh * dd), i = e / D, j = e - i * D;
  const float* p = parts + (size_t)bh * chunks * dd + e;
  float acc = 0.f;
  for (int c = 0; c < chunks; ++c) acc += p[(size_t)c * dd];
  M[t] = acc;
  if (MT) MT[(size_t)bh * dd + (size_t)j * D + i] = acc;
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_attn_transpose(const float* __restrict__ M, float* __restrict__ MT, const int D,
                                                      const long long total) {
  const long long t = (long long)SC_BID_X * 256 + SC_TID;
  if (t >= total) return;
  const int dd = D * D;
  const long long bh = t / dd;
  const int e = (int)(t - bh * dd), i = e / D, j = e - i * D;
  MT[(size_t)bh * dd + (size_t)j * D + i] = M[t];
}

// ---- per-point products with a D x D matrix ----------------------------------------------------------------------------
//   mode 0  out = ((R x) M) w        x = q, M = dots: the forward output u
//   mode 1  out = R^T ((w x) M)      x = g_u, M = dots^T: g_q
struct AttApplyArgs {
  const float* x;              // [B, n, H D]
  const float* M;              // [B H][D][D]
  const float* pos;
  const float* inv_freq;
  const float* weights;        // [B, n] or null
  float* out;                  // [B, n, H D]
  AttGeom g;
  int mode;
};

template <int DP, bool MF>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_attn_apply(const AttApplyArgs a) {
  constexpr int TP = MF ? ATT_MTP(DP) : 32, DS = DP + 1, PR = TP * DP / 256;
  SC_SHARED float tx[TP * DS];
  const int bh = SC_BID_Y, b = bh / a.g.heads, h = bh - b * a.g.heads;
  const int D = a.g.D, hd = a.g.heads * D, hoff = h * D;
  const int n0 = SC_BID_X * TP, np = a.g.n - n0 < TP ? a.g.n - n0 : TP;
  const size_t row0 = (size_t)b * a.g.n + n0;
  const float* wrow = a.weights ? a.weights + row0 : nullptr;
  const float* pos = a.pos ? a.pos + row0 * a.g.rotary : nullptr;
  att_load<TP, DP>(tx, a.x, row0, np, hd, hoff, D, a.mode == 1, wrow, a.g.wconst);
  SC_SYNC();
  if (a.mode == 0) att_rotate<TP, DP>(tx, pos, np, a.g, a.inv_freq, 1.f);
  if constexpr (MF) {
    sc_f32x16 macc[ATT_MNJ(DP)];
    att_apply_mfma<DP>(tx, a.M + (size_t)bh * D * D, macc);
    SC_SYNC();
    att_put_mfma<DP>(tx, macc);
  } else {
    float acc[PR];
    att_apply<TP, DP>(tx, a.M + (size_t)bh * D * D, D, acc);
    SC_SYNC();
    att_put<TP, DP>(tx, acc, 1.f);
  }
  SC_SYNC();
  if (a.mode == 1) att_rotate<TP, DP>(tx, pos, np, a.g, a.inv_freq, -1.f);
  if (a.mode == 0) {
    // the quadrature weight of the query row, after the product as in the reference
#pragma unroll 4
    for (int t = SC_TID; t < TP * DP; t += 256) {
      const int p = t / DP, c = t - p * DP;
      if (p < np && c < D) a.out[(row0 + p) * (size_t)hd + hoff + c] = tx[p * DS + c] * (wrow ? wrow[p] : a.g.wconst);
    }
  } else {
    att_store<TP, DP>(tx, a.out, row0, np, hd, hoff, D);
  }
}

// ---- gradients of k and v ----------------------------------------------------------------------------------------------
// per tile of source points: kn, vn and kr recomputed; g_vn = kr G; g_kn = R^T (vn G^T); the two layer-norm backwards
struct AttKvBwdArgs {
  const float* k;
  const float* v;
  const float* pos;
  const float* inv_freq;
  const float* G;              // g_dots [B H][D][D]
  const float* GT;             // its transpose
  float* gk;                   // null: not wanted
  float* gv;
  AttGeom g;
};

template <int DP>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_attn_kv_bwd(const AttKvBwdArgs a) {
  constexpr int TP = 32, DS = DP + 1, PR = TP * DP / 256;
  SC_SHARED float tk[TP * DS];
  SC_SHARED float tv[TP * DS];
  SC_SHARED float tg[TP * DS];
  SC_SHARED float red[256];
  SC_SHARED double red64[512];
  SC_SHARED float rstd[TP];
  const int bh = SC_BID_Y, b = bh / a.g.heads, h = bh - b * a.g.heads;
  const int D = a.g.D, hd = a.g.heads * D, hoff = h * D;
  const int n0 = SC_BID_X * TP, np = a.g.n - n0 < TP ? a.g.n - n0 : TP;
  const size_t row0 = (size_t)b * a.g.n + n0;
  const float* pos = a.pos ? a.pos + row0 * a.g.rotary : nullptr;
  att_load<TP, DP>(tk, a.k, row0, np, hd, hoff, D, false, nullptr, 0.f);
  att_load<TP, DP>(tv, a.v, row0, np, hd, hoff, D, false, nullptr, 0.f);
  SC_SYNC();
  att_norm<TP, DP>(tk, red, rstd, D);
  att_norm<TP, DP>(tv, red, rstd, D);
  att_rotate<TP, DP>(tk, pos, np, a.g, a.inv_freq, 1.f);
  float acc[PR];
  if (a.gv) {                                                // uniform over the launch
    att_apply<TP, DP>(tk, a.G + (size_t)bh * D * D, D, acc);
    att_put<TP, DP>(tg, acc, 1.f);
    SC_SYNC();
    att_norm_bwd<TP, DP>(tg, a.v, row0, np, hd, hoff, red64, D);
    att_store<TP, DP>(tg, a.gv, row0, np, hd, hoff, D);
  }
  if (a.gk) {
    att_apply<TP, DP>(tv, a.GT + (size_t)bh * D * D, D, acc);
    SC_SYNC();                                               // the stores of g_v have read tg
    att_put<TP, DP>(tg, acc, 1.f);
    SC_SYNC();
    att_rotate<TP, DP>(tg, pos, np, a.g, a.inv_freq, -1.f);
    att_norm_bwd<TP, DP>(tg, a.k, row0, np, hd, hoff, red64, D);
    att_store<TP, DP>(tg, a.gk, row0, np, hd, hoff, D);
  }
}

// the same on the matrix cores: two tiles of ATT_MTP points; the two products leave their results in registers, which then
// take the places of their own operands (the layer-norm backward recomputes xn from the raw rows)
template <int DP>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_attn_kv_bwd_mfma(const AttKvBwdArgs a) {
  constexpr int TP = ATT_MTP(DP), DS = DP + 1;
  SC_SHARED float tk[TP * DS];
  SC_SHARED float tv[TP * DS];
  SC_SHARED float red[256];
  SC_SHARED double red64[512];
  SC_SHARED float rstd[TP];
  const int bh = SC_BID_Y, b = bh / a.g.heads, h = bh - b * a.g.heads;
  const int D = a.g.D, hd = a.g.heads * D, hoff = h * D;
  const int n0 = SC_BID_X * TP, np = a.g.n - n0 < TP ? a.g.n - n0 : TP;
  const size_t row0 = (size_t)b * a.g.n + n0;
  const float* pos = a.pos ? a.pos + row0 * a.g.rotary : nullptr;
  att_load<TP, DP>(tk, a.k, row0, np, hd, hoff, D, false, nullptr, 0.f);
  att_load<TP, DP>(tv, a.v, row0, np, hd, hoff, D, false, nullptr, 0.f);
  SC_SYNC();
  att_norm<TP, DP>(tk, red, rstd, D);
  att_norm<TP, DP>(tv, red, rstd, D);
  att_rotate<TP, DP>(tk, pos, np, a.g, a.inv_freq, 1.f);
  sc_f32x16 gvn[ATT_MNJ(DP)], gkr[ATT_MNJ(DP)];
  if (a.gv) att_apply_mfma<DP>(tk, a.G + (size_t)bh * D * D, gvn);       // uniform over the launch
  if (a.gk) att_apply_mfma<DP>(tv, a.GT + (size_t)bh * D * D, gkr);
  SC_SYNC();
  if (a.gv) att_put_mfma<DP>(tv, gvn);
  if (a.gk) att_put_mfma<DP>(tk, gkr);
  SC_SYNC();
  if (a.gk) {
    att_rotate<TP, DP>(tk, pos, np, a.g, a.inv_freq, -1.f);
    att_norm_bwd<TP, DP>(tk, a.k, row0, np, hd, hoff, red64, D);
    att_store<TP, DP>(tk, a.gk, row0, np, hd, hoff, D);
  }
  if (a.gv) {
    att_norm_bwd<TP, DP>(tv, a.v, row0, np, hd, hoff, red64, D);
    att_store<TP, DP>(tv, a.gv, row0, np, hd, hoff, D);
  }
}
