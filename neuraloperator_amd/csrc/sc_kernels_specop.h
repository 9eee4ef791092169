// sc_kernels_specop.h -- the step between the two transforms of a spectral-derivative operator
// (neuralop/losses/differentiation.py:1167-1345, FourierDiff): one pass that reads every source spectrum once and
// writes every requested output spectrum, with the per-mode multipliers formed on the fly from per-axis tables.
//
//   yhat[g, t, m] = sum over terms j with out_j = t of
//                   coef_j * 1/2 (prod_d A_d[tab_jd][i_d(m)] + prod_d B_d[tab_jd][i_d(m)]) * xhat[g, src_j, m]
//
// xhat is (groups, n_src, k1..kN) complex64 contiguous (a full-spectrum SC_FWD_SCALED plan's output, read in place),
// yhat is addressed by a group stride and an output stride (complex elements), A_d / B_d are [n_tab_d][k_d] complex64.
//
// Work split: a workgroup (4 waves, no barrier, no LDS) owns ONE row of the flattened non-last mode dims, a tile of the
// last axis and a run of `gpw` consecutive groups.  A lane owns the column pair (c0, c0 + 1), c0 even: it forms its
// multipliers G_j(c0), G_j(c0 + 1) of every term ONCE -- the non-last-axis factors are the same for the whole
// workgroup (one row), the last-axis factors are read once per lane -- and keeps them in registers over the groups.
// Rows of up to 128 columns take one wave per tile and spread the four waves over the groups; longer rows put 2 or 4
// waves side by side.  Per group and lane: one 16-byte load per source, one 16-byte store per output, contiguous in
// lane order.  The last kept extent is N/2 + 1 (odd for even N), so consecutive rows alternate between 16-byte and
// 8-byte alignment: a row (or the caller's base) that is only 8-byte aligned moves the pair as two 8-byte accesses,
// and the last column of an odd row as one.
//
// The host sorts the terms by output into "slots": a slot carries its source (-1 = an output without a term, written
// as zeros), FIRST / LAST flags of its output and 1/2 coef.  Slot indices are compile-time (unrolled), so the register
// arrays are never indexed at run time.  Fixed summation order, no atomics: two launches give the same bits.
#pragma once
#include "sc_device.h"

#define SPECOP_SLOTS 12        // terms + term-less outputs of one launch
#define SPECOP_MAX_SRC 3
#define SPECOP_FIRST 1
#define SPECOP_LAST 2

struct SpecopArgs {
  const cf32* a_last;          // [n_tab][kl] tables of the last (contiguous) axis
  const cf32* b_last;
  const cf32* a_row[2];        // tables of the non-last axes in order (unused entries null)
  const cf32* b_row[2];
  long long groups, y_gs, y_os;
  int n_row_axes;              // ndim - 1
  int k_row[2];                // kept extents of the non-last axes
  int kl, rows;                // last kept extent; product of the non-last ones
  int n_src, n_slots, conj;
  int gpw;                     // consecutive groups per workgroup
  int col_waves_log2;          // 0..2: waves side by side along the row
  float coef[SPECOP_SLOTS];    // 1/2 coef_j
  unsigned info[SPECOP_SLOTS]; // one word per slot (one scalar register): see specop_info
};
// bits 0-1 FIRST / LAST of its output, 2-3 source + 1 (0 = none), 4-7 output, 8-15 / 16-23 / 24-31 the table rows of
// the last axis and the two non-last axes
SC_HD unsigned specop_info(const int flags, const int src, const int out, const int tl, const int t0, const int t1) {
  return (unsigned)flags | (unsigned)(src + 1) << 2 | (unsigned)out << 4 | (unsigned)tl << 8 | (unsigned)t0 << 16 |
         (unsigned)t1 << 24;
}

// the column pair at p: one 16-byte access where the address allows it and both columns exist
SC_DEVICE void specop_load2(const cf32* p, const bool v0, const bool v1, cf32& a, cf32& b) {
  a = b = cf_make(0.f, 0.f);
  if (v1 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const sc_f4 q = *reinterpret_cast<const sc_f4*>(p);
    a = cf_make(q.x, q.y);
    b = cf_make(q.z, q.w);
  } else {
    if (v0) a = p[0];
    if (v1) b = p[1];
  }
}

SC_DEVICE void specop_store2(cf32* p, const bool v0, const bool v1, const cf32 a, const cf32 b) {
  if (v1 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    sc_f4 q;
    q.x = a.x;
    q.y = a.y;
    q.z = b.x;
    q.w = b.y;
    *reinterpret_cast<sc_f4*>(p) = q;
  } else {
    if (v0) p[0] = a;
    if (v1) p[1] = b;
  }
}

SC_GLOBAL void SC_LAUNCH_BOUNDS_OCC(256, 4)
k_spectral_op(const float* __restrict__ xhat, float* __restrict__ yhat, const SpecopArgs a) {
  const int lane = SC_TID & 63, wave = SC_TID >> 6;
  const int cw = wave & ((1 << a.col_waves_log2) - 1), gw = wave >> a.col_waves_log2;
  const int grp_waves = 4 >> a.col_waves_log2;
  const int kl = a.kl;
  const int t0 = ((SC_BID_Y << a.col_waves_log2) + cw) * 128;
  if (t0 >= kl) return;                                    // a whole wave past the row's end (no barrier below)
  const int c0 = t0 + 2 * lane;
  const bool v0 = c0 < kl, v1 = c0 + 1 < kl;
  const int row = SC_BID_X;
  int i0 = row, i1 = 0;
  if (a.n_row_axes == 2) {
    i0 = row / a.k_row[1];
    i1 = row - i0 * a.k_row[1];
  }

  // the multipliers of this lane's two columns, formed once
  cf32 g0[SPECOP_SLOTS], g1[SPECOP_SLOTS];
#pragma unroll
  for (int j = 0; j < SPECOP_SLOTS; ++j) {
    g0[j] = g1[j] = cf_make(0.f, 0.f);
    const unsigned inf = a.info[j];
    if (j < a.n_slots && (inf >> 2 & 3) != 0) {
      const int tl = inf >> 8 & 255, tr0 = inf >> 16 & 255, tr1 = inf >> 24;
      cf32 pa = cf_make(a.coef[j], 0.f), pb = pa;
      if (a.n_row_axes >= 1) {
        pa = cf_mul(pa, a.a_row[0][tr0 * a.k_row[0] + i0]);
        pb = cf_mul(pb, a.b_row[0][tr0 * a.k_row[0] + i0]);
      }
      if (a.n_row_axes == 2) {
        pa = cf_mul(pa, a.a_row[1][tr1 * a.k_row[1] + i1]);
        pb = cf_mul(pb, a.b_row[1][tr1 * a.k_row[1] + i1]);
      }
      const cf32* la = a.a_last + tl * kl + c0;
      const cf32* lb = a.b_last + tl * kl + c0;
      if (v0) {
        g0[j] = cf_mul(pa, la[0]);
        cf_mac(g0[j], pb, lb[0]);
      }
      if (v1) {
        g1[j] = cf_mul(pa, la[1]);
        cf_mac(g1[j], pb, lb[1]);
      }
      if (a.conj) {
        g0[j].y = -g0[j].y;
        g1[j].y = -g1[j].y;
      }
    }
  }

  const cf32* X = reinterpret_cast<const cf32*>(xhat) + (long long)row * kl + c0;
  cf32* Y = reinterpret_cast<cf32*>(yhat) + (long long)row * kl + c0;
  const long long img = (long long)a.rows * kl;            // one source spectrum
  const long long g_lo = (long long)SC_BID_Z * a.gpw;
  const long long g_hi = g_lo + a.gpw < a.groups ? g_lo + a.gpw : a.groups;
  for (long long g = g_lo + gw; g < g_hi; g += grp_waves) {
    const cf32 z = cf_make(0.f, 0.f);
    cf32 xa0 = z, xa1 = z, xb0 = z, xb1 = z, xc0 = z, xc1 = z;
    const cf32* xg = X + g * a.n_src * img;
    specop_load2(xg, v0, v1, xa0, xa1);
    if (a.n_src > 1) specop_load2(xg + img, v0, v1, xb0, xb1);
    if (a.n_src > 2) specop_load2(xg + 2 * img, v0, v1, xc0, xc1);
    cf32* yg = Y + g * a.y_gs;
    cf32 acc0 = z, acc1 = z;
#pragma unroll
    for (int j = 0; j < SPECOP_SLOTS; ++j) {
      if (j < a.n_slots) {
        const unsigned inf = a.info[j];
        if (inf & SPECOP_FIRST) acc0 = acc1 = z;
        const int s = (int)(inf >> 2 & 3);                 // source + 1, 0 = none
        if (s != 0) {
          cf_mac(acc0, g0[j], s == 1 ? xa0 : s == 2 ? xb0 : xc0);
          cf_mac(acc1, g1[j], s == 1 ? xa1 : s == 2 ? xb1 : xc1);
        }
        if (inf & SPECOP_LAST) specop_store2(yg + (long long)(inf >> 4 & 15) * a.y_os, v0, v1, acc0, acc1);
      }
    }
  }
}
