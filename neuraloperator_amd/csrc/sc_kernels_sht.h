// sc_kernels_sht.h -- the latitude (Legendre) stage of the real spherical-harmonic transforms (RealSHT /
// InverseRealSHT of torch_harmonics, called by neuralop/layers/spherical_convolution.py:206-281).
//
// The longitude stage is the engine's 1-d real plans: their output / input is [lines * nlat, mmax] complex
// interleaved, so one line's nlat x mmax block is contiguous and is read here in place.  Both kernels contract the
// middle axis of a [lines, Q, mmax] complex operand against a REAL fp32 table laid out [lmax][nlat][mmax] (m fastest):
//
//   k_legendre_analysis   c[line, l, m] = sum_k X[line, k, m] * T[l, k, m]      (P = lmax rows out, Q = nlat in)
//   k_legendre_synthesis  X[line, k, m] = sum_l c[line, l, m] * S[l, k, m]      (P = nlat rows out, Q = lmax in)
//
// T[l, k, m] = 2 pi Pbar_l^m(cos theta_k) w_k (analysis), S = Pbar (synthesis).  With a real table each kernel is the
// other's adjoint: the gradient of analysis is synthesis with T, the gradient of synthesis is analysis with S.
//
// Work split: workgroup = 4 waves; lane = one m of a 64-column group (every load and store is one coalesced row of
// m); wave w owns SHT_PB consecutive output rows p; every lane carries SHT_LT lines x SHT_PB rows of complex
// accumulators in registers.  One table value feeds SHT_LT lines, one operand value SHT_PB rows; the four waves of a
// workgroup read the same operand rows (L1 hits).  The loop is latency bound at one wave per SIMD, so each step issues
// the loads of SHT_QU terms before their FMAs.  The zero triangle Pbar_l^m = 0, l < m, is skipped per lane: in
// analysis a lane whose SHT_PB rows all lie below m does not enter the loop (on the diagonal block it reads the
// table's zeros); synthesis starts its sum at l = the first m of the 64-column group (a per-lane start at l = m would
// scatter each load over 64 rows), so only columns m >= 64 save their triangle there.  The output is written in full (zeros for l < m).  Fixed summation order in k
// resp. l, no atomics: two runs give the same bits.
#pragma once
#include "sc_device.h"

#ifndef SHT_LT
#define SHT_LT 4       // lines per lane (scripts may build variants with -DSHT_LT=n)
#endif
#define SHT_PB 4       // output rows per wave
#define SHT_ROWS (4 * SHT_PB)   // output rows per workgroup
#define SHT_QU 8       // summation terms per load batch

struct LegendreArgs {
  long long lines;
  int nlat, lmax, mmax;
};

// SYN = false: analysis (p = l, q = k, triangle on p); SYN = true: synthesis (p = k, q = l, triangle on q)
template <bool SYN>
SC_DEVICE void legendre_contract(const float* __restrict__ in, const float* __restrict__ tab, float* __restrict__ out,
                                 const LegendreArgs& a) {
  const int lane = SC_TID & 63, wave = SC_TID >> 6;
  const int m = SC_BID_Z * 64 + lane;
  const int P = SYN ? a.nlat : a.lmax, Q = SYN ? a.lmax : a.nlat;
  const int p0 = SC_BID_Y * SHT_ROWS + wave * SHT_PB;
  const long long line0 = (long long)SC_BID_X * SHT_LT;
  const long long qs = (long long)a.mmax;                 // operand stride of q (complex elements)
  const long long ls = (long long)Q * a.mmax;             // operand stride of a line
  const long long ts = (long long)a.nlat * a.mmax;        // table stride of l
  // lines past the end read the last line (never outside the buffer) and are not stored
  long long lo[SHT_LT];
#pragma unroll
  for (int j = 0; j < SHT_LT; ++j) lo[j] = (line0 + j < a.lines ? line0 + j : a.lines - 1) * ls;
  float ar[SHT_LT][SHT_PB], ai[SHT_LT][SHT_PB];
#pragma unroll
  for (int j = 0; j < SHT_LT; ++j)
#pragma unroll
    for (int i = 0; i < SHT_PB; ++i) ar[j][i] = ai[j][i] = 0.0f;
  const bool live = m < a.mmax && p0 < P && (SYN || p0 + SHT_PB - 1 >= m);
  if (live) {
    const cf32* x = reinterpret_cast<const cf32*>(in) + m;
    const float* t = tab + m;
    // table offsets of this wave's rows (clamped into the table: rows past P are computed, never stored)
    long long to[SHT_PB];
#pragma unroll
    for (int i = 0; i < SHT_PB; ++i) {
      const long long p = p0 + i < P ? p0 + i : P - 1;
      to[i] = SYN ? p * a.mmax : p * ts;
    }
    const long long tq = SYN ? ts : (long long)a.mmax;    // table stride of q
    // SHT_QU terms per step, all loads issued before the FMAs (the loop is latency bound otherwise); terms past Q
    // read row Q - 1 and are weighted 0.  Rows of a wave below the diagonal (analysis, l < m) read the table's zeros.
    // synthesis starts at the wave's first m: one start for the whole wave keeps every load a coalesced row of m
    // (lanes read the table's zeros for l < m on the way), per-lane starts scatter them over 64 rows
    for (int q = SYN ? SC_BID_Z * 64 : 0; q < Q; q += SHT_QU) {
      cf32 v[SHT_QU][SHT_LT];
      float w[SHT_QU][SHT_PB];
#pragma unroll
      for (int u = 0; u < SHT_QU; ++u) {
        const long long qq = q + u < Q ? q + u : Q - 1;
#pragma unroll
        for (int j = 0; j < SHT_LT; ++j) v[u][j] = x[lo[j] + qq * qs];
#pragma unroll
        for (int i = 0; i < SHT_PB; ++i) w[u][i] = t[to[i] + qq * tq];
      }
#pragma unroll
      for (int u = 0; u < SHT_QU; ++u) {
        const bool in_q = q + u < Q;
#pragma unroll
        for (int i = 0; i < SHT_PB; ++i) {
          const float wi = in_q ? w[u][i] : 0.0f;
#pragma unroll
          for (int j = 0; j < SHT_LT; ++j) {
            ar[j][i] += v[u][j].x * wi;
            ai[j][i] += v[u][j].y * wi;
          }
        }
      }
    }
  }
  if (m >= a.mmax) return;
  cf32* y = reinterpret_cast<cf32*>(out) + m;
#pragma unroll
  for (int j = 0; j < SHT_LT; ++j) {
    if (line0 + j >= a.lines) break;
#pragma unroll
    for (int i = 0; i < SHT_PB; ++i)
      if (p0 + i < P) y[(line0 + j) * P * (long long)a.mmax + (long long)(p0 + i) * a.mmax] = cf_make(ar[j][i], ai[j][i]);
  }
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_legendre_analysis(const float* __restrict__ x, const float* __restrict__ tab, float* __restrict__ c, LegendreArgs a) {
  legendre_contract<false>(x, tab, c, a);
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_legendre_synthesis(const float* __restrict__ c, const float* __restrict__ tab, float* __restrict__ x, LegendreArgs a) {
  legendre_contract<true>(c, tab, x, a);
}
