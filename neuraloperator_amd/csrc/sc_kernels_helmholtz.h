// sc_kernels_helmholtz.h -- the step between the two transforms of a divergence-free (Helmholtz-Hodge) spectral
// projection (neuralop/layers/spectral_projection.py:6-102): one pass over the spectra of the n_comp = ndim components
// of a vector field that multiplies every mode by its n_comp x n_comp projector, in place if asked.
//
//   per mode m and sign s (+: the mode itself, -: its mirror -k):
//     K_c   = kappa_{sel[c]}                          the wavenumber component c pairs with
//     w     = prod_d keep_d * (1 - prod_d z_d)        keep / z are 0 / 1 flags
//     G_ab  = w (delta_ab - K_a K_b / (sum_c K_c^2 + eps))
//   yhat[g, a, m] = sum_b 1/2 (G+_ab + G-_ab) xhat[g, b, m]
//
// The multiplier does not factor into per-axis tables, but its ingredients do: axis d carries a real fp32 table
// [kept_d][2][3], entry [i][s] = (kappa, keep, z) of row i for s = + and s = -.  xhat is (groups, n_comp, k1..kN)
// complex64 contiguous in a plan's row order, yhat is addressed by a group stride and a component stride.
//
// Work split: that of k_spectral_op (sc_kernels_specop.h).  A workgroup (4 waves, no barrier, no LDS) owns ONE row of
// the flattened non-last mode dims, a tile of the last axis and a run of `gpw` consecutive groups.  A lane owns the
// column pair (c0, c0 + 1), c0 even, forms the n_comp (n_comp + 1) / 2 multipliers of either column ONCE and keeps
// them in registers over the groups.  Rows of up to 128 columns take one wave per tile and spread the four waves over
// the groups; longer rows put 2 or 4 waves side by side.  Per group and lane: one 16-byte load per component, then one
// 16-byte store per component (8-byte accesses where the address is only 8-byte aligned, and for the last column of an
// odd row).  Every load of a group precedes its first store and no two lanes share an element, so yhat == xhat with
// the source's strides is allowed.
//
// Arithmetic of one multiplier, written so that no step cancels (the diagonal is (sum_{c != a} K_c^2 + eps) / den, not
// 1 - K_a^2 / den): n_a = eps + sum_{c != a} K_c^2 by fmaf (n_comp - 1 roundings), den = fmaf(K_a, K_a, n_a) (n_comp),
// q = w / den (n_comp + 1, w exact), G_aa = n_a q (2 n_comp + 1), G_ab = -(K_a K_b) q (n_comp + 3); the half sum of
// the two signs one more; then a product and n_comp - 1 fmaf per real component of an output: N = 3 n_comp + 2
// roundings at most.  Fixed order, no atomics: two launches give the same bits.
#pragma once
#include "sc_device.h"
#include "sc_kernels_specop.h"

struct HelmArgs {
  const float* t_last;         // [kl][2][3] table of the last (contiguous) axis
  const float* t_row[2];       // tables of the non-last axes in order (unused entries null)
  long long groups, y_gs, y_cs;
  int n_row_axes;              // ndim - 1
  int k_row[2];                // kept extents of the non-last axes
  int kl, rows;                // last kept extent; product of the non-last ones
  int sel[3];                  // component -> axis whose kappa it takes (ndim - 1 = the last axis)
  int gpw;                     // consecutive groups per workgroup
  int col_waves_log2;          // 0..2: waves side by side along the row
  float eps;
};

// the upper triangle of one sign's projector: g[0..NC) the diagonal, then (0,1)[, (0,2), (1,2)]
template <int NC>
SC_DEVICE void helm_sign(const float k0, const float k1, const float k2, const float w, const float eps,
                         float (&g)[NC == 2 ? 3 : 6]) {
  if (NC == 2) {
    const float n0 = fmaf(k1, k1, eps), n1 = fmaf(k0, k0, eps);
    const float q = w / fmaf(k0, k0, n0);
    g[0] = n0 * q;
    g[1] = n1 * q;
    g[2] = -(k0 * k1) * q;
  } else {
    const float e0 = fmaf(k0, k0, eps), e1 = fmaf(k1, k1, eps);
    const float n0 = fmaf(k2, k2, e1), n1 = fmaf(k2, k2, e0), n2 = fmaf(k1, k1, e0);
    const float q = w / fmaf(k0, k0, n0);
    g[0] = n0 * q;
    g[1] = n1 * q;
    g[2] = n2 * q;
    g[3] = -(k0 * k1) * q;
    g[4] = -(k0 * k2) * q;
    g[5] = -(k1 * k2) * q;
  }
}

// 1/2 (G+ + G-) of column c: kr / keep_r / z_r the row axes' kappa and flag products of the two signs
template <int NC>
SC_DEVICE void helm_column(const HelmArgs& a, const int c, const float (&kr)[2][2], const float keep_r[2],
                           const float z_r[2], float (&g)[NC == 2 ? 3 : 6]) {
  constexpr int NG = NC == 2 ? 3 : 6;
  float gs[2][NG];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float* t = a.t_last + ((long long)c * 2 + s) * 3;
    const float kl = t[0], w = keep_r[s] * t[1] * (1.f - z_r[s] * t[2]);
    float k[3];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int ax = a.sel[i];
      k[i] = ax == NC - 1 ? kl : ax == 0 ? kr[s][0] : kr[s][1];
    }
    helm_sign<NC>(k[0], k[1], NC == 3 ? k[2] : 0.f, w, a.eps, gs[s]);
  }
#pragma unroll
  for (int j = 0; j < NG; ++j) g[j] = 0.5f * (gs[0][j] + gs[1][j]);
}

// y = G x for one column: G symmetric, g as in helm_sign
template <int NC>
SC_DEVICE void helm_apply(const float (&g)[NC == 2 ? 3 : 6], const cf32 (&x)[NC], cf32 (&y)[NC]) {
  if (NC == 2) {
    y[0] = cf_make(fmaf(g[2], x[1].x, g[0] * x[0].x), fmaf(g[2], x[1].y, g[0] * x[0].y));
    y[1] = cf_make(fmaf(g[1], x[1].x, g[2] * x[0].x), fmaf(g[1], x[1].y, g[2] * x[0].y));
  } else {
    y[0] = cf_make(fmaf(g[4], x[2].x, fmaf(g[3], x[1].x, g[0] * x[0].x)),
                   fmaf(g[4], x[2].y, fmaf(g[3], x[1].y, g[0] * x[0].y)));
    y[1] = cf_make(fmaf(g[5], x[2].x, fmaf(g[1], x[1].x, g[3] * x[0].x)),
                   fmaf(g[5], x[2].y, fmaf(g[1], x[1].y, g[3] * x[0].y)));
    y[2] = cf_make(fmaf(g[2], x[2].x, fmaf(g[5], x[1].x, g[4] * x[0].x)),
                   fmaf(g[2], x[2].y, fmaf(g[5], x[1].y, g[4] * x[0].y)));
  }
}

// xhat and yhat may be the same buffer: no __restrict__
template <int NC>
SC_GLOBAL void SC_LAUNCH_BOUNDS_OCC(256, 4)
k_helmholtz_project(const float* xhat, float* yhat, const HelmArgs a) {
  constexpr int NG = NC == 2 ? 3 : 6;
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

  // the row axes' share of either sign: the same for the whole workgroup
  float kr[2][2], keep_r[2], z_r[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float* r0 = a.t_row[0] + ((long long)i0 * 2 + s) * 3;
    kr[s][0] = r0[0];
    kr[s][1] = 0.f;
    keep_r[s] = r0[1];
    z_r[s] = r0[2];
    if (NC == 3) {
      const float* r1 = a.t_row[1] + ((long long)i1 * 2 + s) * 3;
      kr[s][1] = r1[0];
      keep_r[s] *= r1[1];
      z_r[s] *= r1[2];
    }
  }
  // the multipliers of this lane's two columns, formed once
  float g0[NG], g1[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) g0[j] = g1[j] = 0.f;
  if (v0) helm_column<NC>(a, c0, kr, keep_r, z_r, g0);
  if (v1) helm_column<NC>(a, c0 + 1, kr, keep_r, z_r, g1);

  const cf32* X = reinterpret_cast<const cf32*>(xhat) + (long long)row * kl + c0;
  cf32* Y = reinterpret_cast<cf32*>(yhat) + (long long)row * kl + c0;
  const long long img = (long long)a.rows * kl;            // one component's spectrum
  const long long g_lo = (long long)SC_BID_Z * a.gpw;
  const long long g_hi = g_lo + a.gpw < a.groups ? g_lo + a.gpw : a.groups;
  for (long long g = g_lo + gw; g < g_hi; g += grp_waves) {
    cf32 x0[NC], x1[NC], y0[NC], y1[NC];
    const cf32* xg = X + g * NC * img;
#pragma unroll
    for (int c = 0; c < NC; ++c) specop_load2(xg + c * img, v0, v1, x0[c], x1[c]);
    helm_apply<NC>(g0, x0, y0);
    helm_apply<NC>(g1, x1, y1);
    cf32* yg = Y + g * a.y_gs;
#pragma unroll
    for (int c = 0; c < NC; ++c) specop_store2(yg + c * a.y_cs, v0, v1, y0[c], y1[c]);
  }
}
