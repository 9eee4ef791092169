// sc_kernels_stencil.h -- finite-difference operators and the Lp / H1 data losses in real space
// (neuralop/losses/differentiation.py:11-660, FiniteDiff; neuralop/losses/data_losses.py:21-491, LpLoss / H1Loss).
//
// Every FiniteDiff operator is, along one axis, an N x N matrix D with three interior bands and (non-periodic) two
// one-sided boundary rows of four entries: D, D^T and D^T D are banded with half-width <= 3.  The host cuts each of them
// to a table [N][7] (entry o + 3 of row i multiplies the neighbour i + o) and the kernels below apply such tables:
//
//   k_band_apply        y[g, t, p] = scale[g] * sum_{terms j, out_j = t} coef_j * sum_o T[axis_j][tab_j][i_axis(p)][o]
//                                                                            * s[g, src_j, p + o stride_axis]
//                       with s = u or u - u2 (the fused difference e = x - y) and an identity term (axis -1)
//   k_sobolev_partial   per (line, chunk): num = sum e^2 + sum_j (D_j e)^2, den = sum y^2 + sum_j (D_j y)^2   (H1)
//                                          num = sum |e|^p,                 den = sum |y|^p                  (Lp)
//   k_loss_finish       chunks summed in a fixed order, v_l, dv_l / dnum_l (times the reduction factor), the scalar
//   k_lp_grad           gx[l, i] = dv[l] * gout * p |e_i|^(p-1) sign(e_i)
//
// Fields are handled as 3-d (d0, d1, d2), d2 contiguous, missing leading axes of extent 1.  A workgroup of 4 waves owns
// a tile of BAND_TR rows (axis 1) x BAND_TC columns (axis 2) of one (group, i0) plane: it loads the tile of every source
// with a halo of 3 into LDS ONCE (coalesced rows, the difference u - u2 formed on the way in), and the stencils of the
// last two axes read their neighbours from LDS.  The stencil of axis 0 reads whole rows of the neighbouring planes from
// global memory (coalesced; taps whose table entry is zero -- uniform over the workgroup -- are skipped).  A halo index
// on a periodic axis wraps modulo the extent (right for extents 1, 2, 3, where the offsets alias: the host puts each
// matrix entry into exactly one tap); on a non-periodic axis it is CLAMPED into the line -- its table entry is zero by
// construction, and nothing outside the buffer is read to be multiplied by it.  A wave stores one row segment: 64 lanes,
// 256 contiguous bytes in lane order.  No atomics: every sum runs in a fixed order (per thread in tile order, then an
// LDS tree), so two launches give the same bits.  No register array is indexed at run time (no scratch memory).
#pragma once
#include "sc_device.h"

#define BAND_SLOTS 12          // terms + term-less outputs of one launch
#define BAND_MAX_SRC 3
#define BAND_TC 64             // tile columns = one wave
#define BAND_TR 32             // tile rows: 8 per wave
#define BAND_RPW (BAND_TR / 4)
#define BAND_LW (BAND_TC + 8)  // LDS row: 3 + 64 + 3, padded to 72
#define BAND_LH (BAND_TR + 6)
#define BAND_FIRST 1
#define BAND_LAST 2
#define BAND_AX_IDENT 3
#define BAND_AX_ZERO 4

struct BandGeom {
  int d0, d1, d2;              // extents, d2 contiguous
  int per0, per1, per2;        // periodic flags
  int tiles_r, tiles_c;        // tiles per plane along axis 1 / axis 2
};

struct BandArgs {
  BandGeom g;
  const float* tab[3];         // [n_tab][d][7] per internal axis (null where unused)
  const float* scale;          // optional [groups]
  const float* scale_mul;      // optional [1]: one more multiplier for every group (a loss's grad_output)
  long long y_gs, y_os;        // output strides in floats
  int n_src, n_slots;
  float coef[BAND_SLOTS];
  unsigned info[BAND_SLOTS];   // see band_info
};
// bits 0-1 FIRST / LAST of its output, 2-3 source, 4-7 output, 8-10 axis code (0..2, IDENT, ZERO), 12-19 table row
SC_HD unsigned band_info(const int flags, const int src, const int out, const int axis, const int tab) {
  return (unsigned)flags | (unsigned)src << 2 | (unsigned)out << 4 | (unsigned)axis << 8 | (unsigned)tab << 12;
}

// neighbour index i (-3 .. n + BAND_TR + 2) folded into [0, n): wrapped on a periodic axis, clamped otherwise
SC_DEVICE int band_fold(int i, const int n, const int per) {
  if (per) {
    i %= n;
    return i < 0 ? i + n : i;
  }
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// L[r][c] = p[..] (- q[..]) at rows r0 - 3 + r, columns c0 - 3 + c of the plane at `base`, r < rows, c < BAND_TC + 6
SC_DEVICE void band_load_tile(float* L, const float* __restrict__ p, const float* __restrict__ q, const long long base,
                              const BandGeom& g, const int r0, const int c0, const int rows) {
  for (int idx = SC_TID; idx < rows * BAND_LW; idx += 256) {
    const int r = idx / BAND_LW, c = idx - r * BAND_LW;
    if (c < BAND_TC + 6) {
      const int ri = band_fold(r0 - 3 + r, g.d1, g.per1), ci = band_fold(c0 - 3 + c, g.d2, g.per2);
      const long long off = base + (long long)ri * g.d2 + ci;
      float v = p[off];
      if (q) v -= q[off];
      L[idx] = v;
    }
  }
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_band_apply(const float* __restrict__ u, const float* __restrict__ u2, float* __restrict__ y, const BandArgs a) {
  SC_SHARED float L[BAND_MAX_SRC * BAND_LH * BAND_LW];
  const BandGeom g = a.g;
  long long b = SC_BID_X;
  const int tc = (int)(b % g.tiles_c);
  b /= g.tiles_c;
  const int tr = (int)(b % g.tiles_r);
  b /= g.tiles_r;
  const int i0 = (int)(b % g.d0);
  const long long grp = b / g.d0;
  const int r0 = tr * BAND_TR, c0 = tc * BAND_TC;
  const int rt = g.d1 - r0 < BAND_TR ? g.d1 - r0 : BAND_TR;           // rows of this tile
  const long long plane = (long long)g.d1 * g.d2, img = plane * g.d0;
  for (int s = 0; s < a.n_src; ++s)
    band_load_tile(L + s * (BAND_LH * BAND_LW), u, u2, (grp * a.n_src + s) * img + i0 * plane, g, r0, c0, rt + 6);
  SC_SYNC();

  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int i2 = c0 + lane;
  const bool colok = i2 < g.d2;
  const int i2c = colok ? i2 : g.d2 - 1;
  float sc = a.scale ? a.scale[grp] : 1.f;
  if (a.scale_mul) sc *= a.scale_mul[0];
  float* yp = y + grp * a.y_gs + (long long)i0 * plane + i2;
  float acc[BAND_RPW];
#pragma unroll 1
  for (int j = 0; j < a.n_slots; ++j) {
    const unsigned inf = a.info[j];
    const float coef = a.coef[j];
    const int src = (int)(inf >> 2 & 3), axis = (int)(inf >> 8 & 7), tab = (int)(inf >> 12 & 255);
    if (inf & BAND_FIRST) {
#pragma unroll
      for (int r = 0; r < BAND_RPW; ++r) acc[r] = 0.f;
    }
    const float* Ls = L + src * (BAND_LH * BAND_LW) + 3 * BAND_LW + lane + 3;   // (row 0, this lane's column)
    if (axis == BAND_AX_IDENT) {
#pragma unroll
      for (int r = 0; r < BAND_RPW; ++r) acc[r] = fmaf(coef, Ls[(wave + 4 * r) * BAND_LW], acc[r]);
    } else if (axis == 2) {
      const float* t = a.tab[2] + ((long long)tab * g.d2 + i2c) * 7;
      float c[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) c[k] = coef * t[k];
#pragma unroll
      for (int r = 0; r < BAND_RPW; ++r) {
        const float* row = Ls + (wave + 4 * r) * BAND_LW - 3;
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[r] = fmaf(c[k], row[k], acc[r]);
      }
    } else if (axis == 1) {
#pragma unroll
      for (int r = 0; r < BAND_RPW; ++r) {
        const int rr = wave + 4 * r;
        const int i1c = r0 + rr < g.d1 ? r0 + rr : g.d1 - 1;
        const float* t = a.tab[1] + ((long long)tab * g.d1 + i1c) * 7;      // wave-uniform
        const float* col = Ls + (rr - 3) * BAND_LW;
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[r] = fmaf(coef * t[k], col[k * BAND_LW], acc[r]);
      }
    } else if (axis == 0) {
      const float* t = a.tab[0] + ((long long)tab * g.d0 + i0) * 7;         // workgroup-uniform
#pragma unroll 1
      for (int k = 0; k < 7; ++k) {
        const float ck = coef * t[k];
        if (ck == 0.f) continue;
        const long long off = (grp * a.n_src + src) * img + (long long)band_fold(i0 + k - 3, g.d0, g.per0) * plane + i2;
#pragma unroll
        for (int r = 0; r < BAND_RPW; ++r) {
          const int rr = wave + 4 * r;
          if (colok && rr < rt) {
            const long long o = off + (long long)(r0 + rr) * g.d2;
            float v = u[o];
            if (u2) v -= u2[o];
            acc[r] = fmaf(ck, v, acc[r]);
          }
        }
      }
    }
    if (inf & BAND_LAST) {
      float* yo = yp + (long long)(inf >> 4 & 15) * a.y_os;
#pragma unroll
      for (int r = 0; r < BAND_RPW; ++r) {
        const int rr = wave + 4 * r;
        if (colok && rr < rt) yo[(long long)(r0 + rr) * g.d2] = sc * acc[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- the two data losses
#define SOB_LP_UNIT 1024       // points one pass of a workgroup covers in Lp mode (256 lanes x 4)

struct SobArgs {
  BandGeom g;                  // H1: the field; Lp: unused
  const float* tab[3];         // H1: D of every real axis, [d][7] (null: axis absent)
  long long npts;              // points per line
  long long per_chunk;         // H1: tiles per chunk; Lp: points per chunk (a multiple of SOB_LP_UNIT)
  long long units;             // H1: tiles per line
  int chunks;                  // workgroups per line
  int h1, p, vec;              // vec: 16-byte accesses allowed (npts % 4 == 0, aligned bases)
};

SC_DEVICE float sob_powi(const float a, const int p) {      // a^p, a >= 0, integer p >= 1
  if (p == 1) return a;
  if (p == 2) return a * a;
  float r = a * a;
  for (int i = 2; i < p; ++i) r *= a;
  return r;
}

// fixed-order sum of two values over the 256 threads of a workgroup; the result is valid in thread 0
SC_DEVICE void sob_block_sum2(float* red, float& s0, float& s1) {
  const int t = SC_TID;
  SC_SYNC();
  red[t] = s0;
  red[256 + t] = s1;
  for (int w = 128; w > 0; w >>= 1) {
    SC_SYNC();
    if (t < w) {
      red[t] += red[t + w];
      red[256 + t] += red[256 + t + w];
    }
  }
  SC_SYNC();
  s0 = red[0];
  s1 = red[256];
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_sobolev_partial(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ ws, const SobArgs a) {
  SC_SHARED float L[2 * BAND_LH * BAND_LW];
  SC_SHARED float red[512];
  const long long line = SC_BID_X / a.chunks;
  const int chunk = (int)(SC_BID_X - line * a.chunks);
  const float* xl = x + line * a.npts;
  const float* yl = y + line * a.npts;
  float num = 0.f, den = 0.f;
  if (a.h1) {
    const BandGeom g = a.g;
    const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
    const long long plane = (long long)g.d1 * g.d2;
    float* Le = L + 3 * BAND_LW + lane + 3;
    float* Ly = Le + BAND_LH * BAND_LW;
    const long long t_lo = chunk * a.per_chunk;
    const long long t_hi = t_lo + a.per_chunk < a.units ? t_lo + a.per_chunk : a.units;
#pragma unroll 1
    for (long long tile = t_lo; tile < t_hi; ++tile) {
      long long b = tile;
      const int tc = (int)(b % g.tiles_c);
      b /= g.tiles_c;
      const int tr = (int)(b % g.tiles_r);
      const int i0 = (int)(b / g.tiles_r);
      const int r0 = tr * BAND_TR, c0 = tc * BAND_TC;
      const int rt = g.d1 - r0 < BAND_TR ? g.d1 - r0 : BAND_TR;
      SC_SYNC();                                             // the previous tile has been read
      band_load_tile(L, xl, yl, i0 * plane, g, r0, c0, rt + 6);
      band_load_tile(L + BAND_LH * BAND_LW, yl, nullptr, i0 * plane, g, r0, c0, rt + 6);
      SC_SYNC();
      const int i2 = c0 + lane;
      const bool colok = i2 < g.d2;
      const int i2c = colok ? i2 : g.d2 - 1;
      float c2[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) c2[k] = a.tab[2][(long long)i2c * 7 + k];
#pragma unroll
      for (int r = 0; r < BAND_RPW; ++r) {
        const int rr = wave + 4 * r;
        if (!(colok && rr < rt)) continue;
        const float* re = Le + rr * BAND_LW;
        const float* ry = Ly + rr * BAND_LW;
        float sn = re[0] * re[0], sd = ry[0] * ry[0];
        float de = 0.f, dy = 0.f;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          de = fmaf(c2[k], re[k - 3], de);
          dy = fmaf(c2[k], ry[k - 3], dy);
        }
        sn = fmaf(de, de, sn);
        sd = fmaf(dy, dy, sd);
        if (a.tab[1]) {
          const float* t = a.tab[1] + (long long)(r0 + rr) * 7;           // wave-uniform
          de = dy = 0.f;
#pragma unroll
          for (int k = 0; k < 7; ++k) {
            de = fmaf(t[k], re[(k - 3) * BAND_LW], de);
            dy = fmaf(t[k], ry[(k - 3) * BAND_LW], dy);
          }
          sn = fmaf(de, de, sn);
          sd = fmaf(dy, dy, sd);
        }
        if (a.tab[0]) {
          const float* t = a.tab[0] + (long long)i0 * 7;                   // workgroup-uniform
          de = dy = 0.f;
#pragma unroll 1
          for (int k = 0; k < 7; ++k) {
            const float ck = t[k];
            if (ck == 0.f) continue;
            const long long o = (long long)band_fold(i0 + k - 3, g.d0, g.per0) * plane + (long long)(r0 + rr) * g.d2 + i2;
            const float yv = yl[o];
            de = fmaf(ck, xl[o] - yv, de);
            dy = fmaf(ck, yv, dy);
          }
          sn = fmaf(de, de, sn);
          sd = fmaf(dy, dy, sd);
        }
        num += sn;
        den += sd;
      }
    }
  } else {
    const long long lo = chunk * a.per_chunk;
    const long long hi = lo + a.per_chunk < a.npts ? lo + a.per_chunk : a.npts;
#pragma unroll 1
    for (long long i = lo + 4 * SC_TID; i < hi; i += SOB_LP_UNIT) {
      if (a.vec) {                                           // npts % 4 == 0: all four points exist
        const sc_f4 xv = *reinterpret_cast<const sc_f4*>(xl + i);
        const sc_f4 yv = *reinterpret_cast<const sc_f4*>(yl + i);
        num += sob_powi(fabsf(xv.x - yv.x), a.p) + sob_powi(fabsf(xv.y - yv.y), a.p) +
               sob_powi(fabsf(xv.z - yv.z), a.p) + sob_powi(fabsf(xv.w - yv.w), a.p);
        den += sob_powi(fabsf(yv.x), a.p) + sob_powi(fabsf(yv.y), a.p) + sob_powi(fabsf(yv.z), a.p) +
               sob_powi(fabsf(yv.w), a.p);
      } else {
        for (int k = 0; k < 4; ++k) {
          if (i + k < hi) {
            const float yv = yl[i + k];
            num += sob_powi(fabsf(xl[i + k] - yv), a.p);
            den += sob_powi(fabsf(yv), a.p);
          }
        }
      }
    }
  }
  sob_block_sum2(red, num, den);
  if (SC_TID == 0) {
    float* w = ws + (line * a.chunks + chunk) * 2;
    w[0] = num;
    w[1] = den;
  }
}

struct FinishArgs {
  long long lines;
  int chunks, sub;             // sub: threads that share one line (a power of two <= 256)
  int p, relative, root;       // root: take the p-th root (never with p = 1)
  float konst, eps, factor;    // abs: v = konst num; factor: 1 (sum) or 1 / lines (mean)
};

// ONE workgroup.  256 / sub lines per pass: thread q of a line's `sub` sums chunks q, q + sub, .. in index order, an LDS
// tree adds the sub-sums; then v_l, dv_l; finally the lines are summed the same way into the scalar.
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_loss_finish(const float* __restrict__ ws, float* __restrict__ v, float* __restrict__ dv, float* __restrict__ loss,
              const FinishArgs a) {
  SC_SHARED float red[512];
  const int t = SC_TID, q = t & (a.sub - 1), per_pass = 256 / a.sub;
  const float ip = 1.f / (float)a.p;
  for (long long l0 = 0; l0 < a.lines; l0 += per_pass) {
    const long long l = l0 + t / a.sub;
    float num = 0.f, den = 0.f;
    if (l < a.lines)
      for (int c = q; c < a.chunks; c += a.sub) {
        num += ws[(l * a.chunks + c) * 2];
        den += ws[(l * a.chunks + c) * 2 + 1];
      }
    if (a.sub > 1) {
      SC_SYNC();
      red[t] = num;
      red[256 + t] = den;
      for (int w = a.sub >> 1; w > 0; w >>= 1) {
        SC_SYNC();
        if (q < w) {
          red[t] += red[t + w];
          red[256 + t] += red[256 + t + w];
        }
      }
      num = red[t];
      den = red[256 + t];
    }
    if (q == 0 && l < a.lines) {
      float val, d;
      if (a.relative) {
        if (a.root) {
          const float rn = a.p == 2 ? sqrtf(num) : powf(num, ip);
          const float rd = a.p == 2 ? sqrtf(den) : powf(den, ip);
          val = rn / (rd + a.eps);
          d = val * ip / num;
        } else {
          d = 1.f / (den + a.eps);
          val = num * d;
        }
      } else {
        val = a.konst * num;
        d = a.konst;
        if (a.root) {
          val = a.p == 2 ? sqrtf(val) : powf(val, ip);
          d = val * ip / num;
        }
      }
      v[l] = val;
      dv[l] = d * a.factor;
    }
  }
  SC_SYNC();                                                 // every v[l] of this workgroup is visible
  float s0 = 0.f, s1 = 0.f;
  for (long long l = t; l < a.lines; l += 256) s0 += v[l];
  sob_block_sum2(red, s0, s1);
  if (t == 0) loss[0] = s0 * a.factor;
}

// gx[l, i] = dv[l] * gout * p |e|^(p-1) sign(e), e = x - y; one workgroup per SOB_LP_UNIT points of a line
struct LpGradArgs {
  long long npts, units;       // units: workgroups per line
  int p, vec;
};
SC_DEVICE float sob_dpow(const float e, const int p) {      // |e|^(p-1) sign(e)
  if (p == 2) return e;
  const float s = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
  return p == 1 ? s : s * sob_powi(fabsf(e), p - 1);
}
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_lp_grad(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dv,
          const float* __restrict__ gout, float* __restrict__ gx, const LpGradArgs a) {
  const long long line = SC_BID_X / a.units;
  const long long i = (SC_BID_X - line * a.units) * SOB_LP_UNIT + 4 * SC_TID;
  if (i >= a.npts) return;
  const float s = dv[line] * gout[0] * (float)a.p;
  const long long o = line * a.npts + i;
  if (a.vec) {
    const sc_f4 xv = *reinterpret_cast<const sc_f4*>(x + o);
    const sc_f4 yv = *reinterpret_cast<const sc_f4*>(y + o);
    sc_f4 r;
    r.x = s * sob_dpow(xv.x - yv.x, a.p);
    r.y = s * sob_dpow(xv.y - yv.y, a.p);
    r.z = s * sob_dpow(xv.z - yv.z, a.p);
    r.w = s * sob_dpow(xv.w - yv.w, a.p);
    *reinterpret_cast<sc_f4*>(gx + o) = r;
  } else {
    for (int k = 0; k < 4; ++k)
      if (i + k < a.npts) gx[o + k] = s * sob_dpow(x[o + k] - y[o + k], a.p);
  }
}
