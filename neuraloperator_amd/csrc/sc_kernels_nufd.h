// sc_kernels_nufd.h -- finite differences on a point cloud (neuralop/losses/differentiation.py:728-855,
// get_non_uniform_fd_weights / non_uniform_fd): the k nearest neighbours of every point, one small solve per point, and
// the stencil applied to any number of fields.
//
//   k_knn<D>            the k nearest data points of every query (3 <= k <= 32) by brute force over LDS tiles of the data
//                       points, in ascending (d2, data index): a total order, so two launches give the same bits
//   k_nufd_weights<D>   one thread per point: mask, G = A A^T + lambda I in float64, Cholesky in registers, one solve per
//                       requested derivative, w = A^T y rounded to fp32; an ill-posed point gets zeros and a flag
//   k_nufd_apply        out[j, b, n] = sum_m weights[n, j, m] values[b, index[n, m]], fp32 fmaf in neighbour order
//   k_nufd_adjoint      g_values[b, p] = sum over the entries of the transposed stencil that name p, in ascending entry
//                       id, of sum_j weights[n, j, m] g_out[j, b, n]: a gather, no float atomics
//
// k_knn keeps the tile / queries-per-wave shape of k_radius (sc_kernels_gno.h).  Every query owns a buffer of NUFD_CAP
// (d2, index) pairs in LDS and a wave-uniform threshold, the d2 of its current k-th best.  A data point is a candidate
// while the query has seen fewer than k points, or if its d2 is BELOW the threshold: the data points arrive in ascending
// index, so one that only equals the threshold ranks behind the k entries already held.  The candidates of a chunk of 64
// points are ballot-compacted behind the entries the buffer holds; when it cannot take another 64, the wave ranks the
// buffer in place (every lane counts, for its two entries, the entries with a smaller (d2, index)), keeps the best k and
// tightens the threshold.  d2 is fp32 from the coordinate differences in dimension order, the expression of k_radius; a
// NaN distance counts as +inf.  No register array is indexed at run time (no scratch memory).
#pragma once
#include "sc_device.h"

#define NUFD_TILE 1024             // data points per LDS tile (structure of arrays: 3 x 4 KiB)
#define NUFD_QPW 8                 // queries a wave carries through one pass over the tiles
#define NUFD_QPB (4 * NUFD_QPW)    // queries per workgroup
#define NUFD_CAP 128               // (d2, index) pairs a query's buffer holds: k <= 32 kept + candidates
#define NUFD_KMAX 32
#define NUFD_MAX_DERIV 8
#define NUFD_PIVOT 9.094947017729282e-13   // 2^-40: a pivot must exceed this times trace(G)

struct KnnArgs {
  const float* data;           // [n, D]
  const float* queries;        // [m, D]
  long long n, m;
  int k;
  long long* index;            // [m, k]
  float* d2;                   // [m, k]
};

SC_DEVICE bool nufd_before(const float da, const int ia, const float db, const int ib) {
  return da < db || (da == db && ia < ib);
}

// ranks the cnt <= NUFD_CAP pairs of one query's buffer in place, ascending (d2, index), and keeps the first min(cnt, k);
// one wave, every lane of it
SC_DEVICE int nufd_rank_keep(float* bd, int* bi, const int cnt, const int k, const int lane) {
  SC_WAVE_SYNC();                                            // the candidates have been written
  const float d0 = lane < cnt ? bd[lane] : 0.f, d1 = lane + 64 < cnt ? bd[lane + 64] : 0.f;
  const int i0 = lane < cnt ? bi[lane] : 0, i1 = lane + 64 < cnt ? bi[lane + 64] : 0;
  int r0 = 0, r1 = 0;
#pragma unroll 1
  for (int t = 0; t < cnt; ++t) {
    const float dt = bd[t];
    const int it = bi[t];
    r0 += nufd_before(dt, it, d0, i0) ? 1 : 0;
    r1 += nufd_before(dt, it, d1, i1) ? 1 : 0;
  }
  SC_WAVE_SYNC();                                            // every lane has read the whole buffer
  if (lane < cnt && r0 < k) {
    bd[r0] = d0;
    bi[r0] = i0;
  }
  if (lane + 64 < cnt && r1 < k) {
    bd[r1] = d1;
    bi[r1] = i1;
  }
  SC_WAVE_SYNC();
  return cnt < k ? cnt : k;
}

template <int D>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_knn(const KnnArgs a) {
  SC_SHARED float L[3 * NUFD_TILE];
  SC_SHARED float Bd[NUFD_QPB * NUFD_CAP];
  SC_SHARED int Bi[NUFD_QPB * NUFD_CAP];
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const long long q0 = (long long)SC_BID_X * NUFD_QPB + wave * NUFD_QPW;
  float qx[NUFD_QPW], qy[NUFD_QPW], qz[NUFD_QPW], thr[NUFD_QPW];
  int cnt[NUFD_QPW];
#pragma unroll
  for (int j = 0; j < NUFD_QPW; ++j) {
    const bool ok = q0 + j < a.m;
    const float* q = a.queries + (ok ? q0 + j : 0) * D;
    qx[j] = ok ? q[0] : 0.f;
    qy[j] = ok && D > 1 ? q[D > 1 ? 1 : 0] : 0.f;
    qz[j] = ok && D > 2 ? q[D > 2 ? 2 : 0] : 0.f;
    thr[j] = 0.f;                                            // read only once the query holds k entries (full)
    cnt[j] = 0;
  }
  unsigned full = 0;                                         // bit j: query j holds k ranked entries and a threshold
#pragma unroll 1
  for (long long t0 = 0; t0 < a.n; t0 += NUFD_TILE) {
    SC_SYNC();                                               // the previous tile has been read
    for (int i = SC_TID; i < NUFD_TILE; i += 256) {
      const bool ok = t0 + i < a.n;
      const float* p = a.data + (ok ? t0 + i : 0) * D;
      L[i] = ok ? p[0] : 0.f;
      if (D > 1) L[NUFD_TILE + i] = ok ? p[D > 1 ? 1 : 0] : 0.f;
      if (D > 2) L[2 * NUFD_TILE + i] = ok ? p[D > 2 ? 2 : 0] : 0.f;
    }
    SC_SYNC();
    const int tn = a.n - t0 < NUFD_TILE ? (int)(a.n - t0) : NUFD_TILE;
#pragma unroll 1
    for (int ch = 0; ch < tn; ch += 64) {
      const int i = ch + lane;
      const bool in = i < tn;
      const float px = L[i], py = D > 1 ? L[NUFD_TILE + i] : 0.f, pz = D > 2 ? L[2 * NUFD_TILE + i] : 0.f;
#pragma unroll
      for (int j = 0; j < NUFD_QPW; ++j) {
        if (q0 + j >= a.m) continue;                         // wave-uniform
        const float dx = qx[j] - px, dy = qy[j] - py, dz = qz[j] - pz;
        float d2 = dx * dx;                                  // fp32, in dimension order
        if (D > 1) d2 = fmaf(dy, dy, d2);
        if (D > 2) d2 = fmaf(dz, dz, d2);
        if (!(d2 == d2)) d2 = __builtin_inff();
        const bool hit = in && (((full >> j) & 1u) ? d2 < thr[j] : true);
        const unsigned long long mk = sc_ballot(hit);
        if (mk == 0ull) continue;                            // wave-uniform
        float* bd = Bd + (wave * NUFD_QPW + j) * NUFD_CAP;
        int* bi = Bi + (wave * NUFD_QPW + j) * NUFD_CAP;
        if (hit) {
          const int o = cnt[j] + sc_popc64(mk & ((1ull << lane) - 1ull));
          if (o < NUFD_CAP) {                                // holds by construction: cnt <= NUFD_CAP - 64 here
            bd[o] = d2;
            bi[o] = (int)(t0 + i);
          }
        }
        cnt[j] += sc_popc64(mk);
        if (cnt[j] > NUFD_CAP - 64) {                        // no room for another 64 candidates
          cnt[j] = nufd_rank_keep(bd, bi, cnt[j], a.k, lane);
          if (cnt[j] == a.k) {
            thr[j] = bd[a.k - 1];
            full |= 1u << j;
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NUFD_QPW; ++j) {
    if (q0 + j >= a.m) continue;                             // wave-uniform
    float* bd = Bd + (wave * NUFD_QPW + j) * NUFD_CAP;
    int* bi = Bi + (wave * NUFD_QPW + j) * NUFD_CAP;
    const int kept = nufd_rank_keep(bd, bi, cnt[j], a.k, lane);
    if (lane < a.k) {                                        // kept == k: the host refuses k > n
      const bool ok = lane < kept;
      a.index[(q0 + j) * a.k + lane] = ok ? (long long)bi[lane] : -1;
      a.d2[(q0 + j) * a.k + lane] = ok ? bd[lane] : __builtin_inff();
    }
  }
}

// --------------------------------------------------------------------------------------------------- weights per point
struct NufdWArgs {
  const float* points;         // [n, D]
  const long long* index;      // [n, k]
  const float* d2;             // [n, k]; read with a radius only
  float* weights;              // [n, n_deriv, k]
  int* flag;                   // [n]
  long long n;
  int k, n_deriv;
  unsigned deriv;              // 2 bits per requested derivative: its coordinate
  int has_radius;
  float r2;
  double lambda;
};

template <int D>
SC_DEVICE bool nufd_diff(const NufdWArgs& a, const long long p, const int m, const double (&c)[3], double (&dx)[3]) {
  const long long e = p * a.k + m;
  const long long q = a.index[e];
  bool keep = q >= 0 && q < a.n;                             // a caller's index: checked before it addresses memory
  if (a.has_radius && m >= 3) keep = keep && a.d2[e] <= a.r2;
  const float* x = a.points + (keep ? q : 0) * D;
#pragma unroll
  for (int i = 0; i < 3; ++i) dx[i] = i < D ? (double)x[i < D ? i : 0] - c[i] : 0.0;   // exact in float64
  return keep;
}

template <int D>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_nufd_weights(const NufdWArgs a) {
  constexpr int R = D + 1;
  const long long p = (long long)SC_BID_X * 256 + SC_TID;
  if (p >= a.n) return;
  double c[3], dx[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = i < D ? (double)a.points[p * D + (i < D ? i : 0)] : 0.0;
  // G = A A^T + lambda I, lower triangle: row 0 of A is ones, row i + 1 the differences of coordinate i
  double G[R][R];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int s = 0; s < R; ++s) G[r][s] = 0.0;
#pragma unroll 1
  for (int m = 0; m < a.k; ++m) {
    if (!nufd_diff<D>(a, p, m, c, dx)) continue;
    G[0][0] += 1.0;
#pragma unroll
    for (int r = 1; r < R; ++r) {
      G[r][0] += dx[r - 1];
#pragma unroll
      for (int s = 1; s <= r; ++s) G[r][s] = fma(dx[r - 1], dx[s - 1], G[r][s]);
    }
  }
  double trace = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    G[r][r] += a.lambda;
    trace += G[r][r];
  }
  // Cholesky G = L L^T in place; a pivot that is not above 2^-40 trace(G) (or is no number) marks the point ill-posed
  bool bad = !(trace == trace) || trace == __builtin_inf();
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int s = 0; s <= r; ++s) {
      double v = G[r][s];
#pragma unroll
      for (int t = 0; t < s; ++t) v -= G[r][t] * G[s][t];
      if (s == r) {
        if (!(v > NUFD_PIVOT * trace)) bad = true;
        G[r][r] = bad ? 1.0 : sqrt(v);
      } else {
        G[r][s] = v / G[s][s];
      }
    }
  }
  a.flag[p] = bad ? 1 : 0;
#pragma unroll 1
  for (int j = 0; j < a.n_deriv; ++j) {
    const int di = (int)((a.deriv >> (2 * j)) & 3u) + 1;     // the row of A this derivative's right-hand side selects
    double y[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {                            // L z = e_di
      double v = r == di ? 1.0 : 0.0;
#pragma unroll
      for (int t = 0; t < r; ++t) v -= G[r][t] * y[t];
      y[r] = v / G[r][r];
    }
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {                       // L^T y = z
      double v = y[r];
#pragma unroll
      for (int t = r + 1; t < R; ++t) v -= G[t][r] * y[t];
      y[r] = v / G[r][r];
    }
    float* w = a.weights + (p * a.n_deriv + j) * a.k;
#pragma unroll 1
    for (int m = 0; m < a.k; ++m) {                          // w = A^T y; a masked neighbour gets 0
      const bool keep = nufd_diff<D>(a, p, m, c, dx);
      double v = y[0];
#pragma unroll
      for (int r = 1; r < R; ++r) v = fma(y[r], dx[r - 1], v);
      w[m] = keep && !bad ? (float)v : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------------ apply, adjoint
struct NufdApplyArgs {
  const float* weights;        // [n, n_deriv, k]
  const long long* index;      // apply: [n, k]
  const long long* col_splits; // adjoint: [n + 1]
  const int* perm;             // adjoint: [n k], entry ids by the point they name, ascending within each point
  const float* in;             // apply: values [batch, n]; adjoint: g_out [n_deriv, batch, n]
  float* out;                  // apply: [n_deriv, batch, n]; adjoint: g_values [batch, n]
  long long n;
  int k, n_deriv, batch;
};

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_nufd_apply(const NufdApplyArgs a) {
  const long long p = (long long)SC_BID_X * 256 + SC_TID;
  const int b = SC_BID_Y;
  if (p >= a.n) return;
  const float* v = a.in + (long long)b * a.n;
  const long long* idx = a.index + p * a.k;
#pragma unroll 1
  for (int j = 0; j < a.n_deriv; ++j) {
    const float* w = a.weights + (p * a.n_deriv + j) * a.k;
    float acc = 0.f;
#pragma unroll 1
    for (int m = 0; m < a.k; ++m) {
      const long long q = idx[m];
      if (q >= 0 && q < a.n) acc = fmaf(w[m], v[q], acc);
    }
    a.out[((long long)j * a.batch + b) * a.n + p] = acc;
  }
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_nufd_adjoint(const NufdApplyArgs a) {
  const long long p = (long long)SC_BID_X * 256 + SC_TID;
  const int b = SC_BID_Y;
  if (p >= a.n) return;
  const long long E = a.n * a.k;
  long long lo = a.col_splits[p], hi = a.col_splits[p + 1];
  lo = lo < 0 ? 0 : (lo > E ? E : lo);
  hi = hi < lo ? lo : (hi > E ? E : hi);
  float acc = 0.f;
#pragma unroll 1
  for (long long t = lo; t < hi; ++t) {
    const long long e = a.perm[t];
    if (e < 0 || e >= E) continue;
    const long long row = e / a.k;
    const int m = (int)(e - row * a.k);
#pragma unroll 1
    for (int j = 0; j < a.n_deriv; ++j)
      acc = fmaf(a.weights[(row * a.n_deriv + j) * a.k + m], a.in[((long long)j * a.batch + b) * a.n + row], acc);
  }
  a.out[(long long)b * a.n + p] = acc;
}
