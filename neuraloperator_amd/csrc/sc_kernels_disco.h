// sc_kernels_disco.h -- the equidistant discrete-continuous (DISCO) convolution of the local neural operator
// (neuralop/layers/discrete_continuous_convolution.py, EquidistantDiscreteContinuousConv2d and ...ConvTranspose2d):
//
//   kernel[o, c, i, j] = q sum_k Psi'[k, i, j] weight[o, c, k]        Psi' (K, ph, pw): the basis on the local grid
//   plain class       y = conv2d(x, kernel, bias, stride (sh, sw), padding (padh, padw), groups)       zero padding
//   transpose class   y = conv_transpose2d(x, kernel, bias, stride, padding, output_padding, groups)
//
// Both classes are ONE strided correlation C between a FINE grid (hf x wf, cc_in channels) and a COARSE grid
// (hc x wc, cc_out channels), coarse = C(fine):
//   coarse[b, o, p, q] = sum_{c, i, j} kernel[o, c, i, j] finepad[b, c, sh p + i - padh, sw q + j - padw]
// and its adjoint C^T.  The plain class is y = C x, gx = C^T gout; the transpose class is y = C^T x, gx = C gout; the
// weight is stored (cc_out, cc_in / groups, K) by both.
//
//   k_disco_fold     one thread per (o, c): kernel in the forward layout wf (cc_out, cin_g, taps) and tap-flipped,
//                    channel-transposed wt (cc_in, cout_g, taps) for the adjoint; on the matrix-core route both also in
//                    the round-major layout of k_fdconv_fold
//   k_disco_conv     C, vector ALU: any channel counts and groups, support 1..15 per axis, stride 1..4 per axis.  A
//                    workgroup of 4 waves owns tr x 64 coarse points (tr = 16, 8, 4, 4 for row stride 1..4, so the
//                    input tile (tr - 1) sh + ph rows by 63 sw + pw columns fits DC_LH x DC_LW whatever the stride) and
//                    DC_OCB output channels; per input channel the tile is staged in LDS in coalesced rows, a wave
//                    stores whole row segments in lane order, the bias is added in the store.
//   k_disco_convT    C^T as a gather: a workgroup owns 16 x 64 fine points and DC_OCB fine-grid channels; per coarse
//                    channel it stages the coarse rows / columns any of its points reads; a fine point u sums the taps
//                    t with (u + pad - t) divisible by the stride, reading wt.
//   k_disco_wgrad    per-workgroup partial G[o, c, i, .] = sum gout[b, o, p] finepad[b, c, s p + (i, .) - pad] of one
//                    (o, c, tap row) over a chunk of coarse tiles
//   k_disco_psum     partials summed in index order into G (coalesced over the weight entries)
//   k_disco_wreduce  G projected onto the basis: gw[o, c, k] = q sum_t Psi'[k, t] G[o, c, t];
//                    further workgroups write gbias[o] = sum_{b, p} gout in a fixed order
//   k_disco_mfma     matrix-core route (stride 1, 3 x 3, groups 1, channels 32 / 64 / 128): the body of k_fdconv_mfma
//                    in zeros mode on the DISCO-folded weights, bias in the store; its weight gradient is
//                    k_fdconv_wgrad_mfma followed by k_disco_wreduce
//
// No float atomics, every sum in a fixed order: two launches give the same bits.  No register array is indexed at run
// time.  Nothing outside a buffer is addressed: a coordinate outside a grid is a zero written into LDS.
#pragma once
#include "sc_device.h"
#include "sc_kernels_fdconv.h"

#define DC_MAX_P 15            // support per axis
#define DC_MAX_S 4             // stride per axis
#define DC_TC 64               // tile columns = one wave
#define DC_OCB 8               // output channels of one workgroup
#define DC_LH 30               // LDS rows: (tr - 1) sh + ph <= 30 for tr = 16, 8, 4, 4
#define DC_LW 272              // LDS row: 63 sw + pw <= 267, padded
#define DT_TR 16               // adjoint: fine tile rows
#define DT_LW 80               // adjoint: coarse columns of a tile <= 63 + 14 + 1

struct DcGeom {
  int hf, wf;                  // fine grid
  int hc, wc;                  // coarse grid
  int ph, pw, sh, sw, padh, padw;
  int tr;                      // coarse tile rows (k_disco_conv, k_disco_wgrad)
  int tiles_r, tiles_c;        // tiles of the grid the launch walks
};

struct DcArgs {
  DcGeom g;
  int cc_in, cc_out, groups;   // channels on the fine / coarse grid
  int n_blk;                   // blocks of DC_OCB output channels per group
};

SC_DEVICE int dc_floordiv(const int a, const int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// ------------------------------------------------------------------------------------------------- folded weights
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_disco_fold(const float* __restrict__ w, const float* __restrict__ psi, float* __restrict__ wf, float* __restrict__ wt,
             float* __restrict__ wfm, float* __restrict__ wtm, const int cc_out, const int cin_g, const int cout_g,
             const int nk, const int taps, const float q) {
  const long long i = (long long)SC_BID_X * 256 + SC_TID;
  if (i >= (long long)cc_out * cin_g) return;
  const int o = (int)(i / cin_g), c = (int)(i - (long long)o * cin_g);
  const int grp = o / cout_g, ol = o - grp * cout_g;
  const float* ws = w + i * nk;
  float* f = wf + i * taps;
  float* t = wt + ((long long)(grp * cin_g + c) * cout_g + ol) * taps;
  for (int j = 0; j < taps; ++j) {
    float s = 0.f;
    for (int k = 0; k < nk; ++k) s = fmaf(psi[(long long)k * taps + j], ws[k], s);
    s *= q;
    f[j] = s;
    t[taps - 1 - j] = s;
    if (wfm) {                                               // matrix-core route (groups 1, 9 taps)
      wfm[(((long long)(c / FDM_CK) * 9 + j) * FDM_CK + c % FDM_CK) * cc_out + o] = s;
      wtm[(((long long)(o / FDM_CK) * 9 + (8 - j)) * FDM_CK + o % FDM_CK) * cin_g + c] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------- C, vector ALU
// x (B, cc_in, hf, wf), w = wf of k_disco_fold, y (B, cc_out, hc, wc)
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_disco_conv(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
             float* __restrict__ y, const DcArgs a) {
  SC_SHARED float L[DC_LH * DC_LW];
  const DcGeom g = a.g;
  int b = SC_BID_X;
  const int tc = b % g.tiles_c;
  b /= g.tiles_c;
  const int tr = b % g.tiles_r;
  b /= g.tiles_r;
  const int ob = b % a.n_blk;
  b /= a.n_blk;
  const int grp = b % a.groups;
  const int bb = b / a.groups;
  const int cin_g = a.cc_in / a.groups, cout_g = a.cc_out / a.groups;
  const int row0 = tr * g.tr, col0 = tc * DC_TC;
  const int rt = g.hc - row0 < g.tr ? g.hc - row0 : g.tr;    // rows of this tile
  const int rpw = g.tr >> 2;                                 // rows per wave: 4, 2 or 1
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int o_lo = ob * DC_OCB;
  const int n_o = cout_g - o_lo < DC_OCB ? cout_g - o_lo : DC_OCB;
  const int taps = g.ph * g.pw;
  const int in_rows = (rt - 1) * g.sh + g.ph, in_cols = (DC_TC - 1) * g.sw + g.pw;
  const int row_lo = row0 * g.sh - g.padh, col_lo = col0 * g.sw - g.padw;
  const long long plane = (long long)g.hf * g.wf;
  float acc[DC_OCB][4];
#pragma unroll
  for (int j = 0; j < DC_OCB; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
  const float* Ll = L + wave * g.sh * DC_LW + lane * g.sw;

#pragma unroll 1
  for (int c = 0; c < cin_g; ++c) {
    const float* xc = x + ((long long)bb * a.cc_in + grp * cin_g + c) * plane;
    SC_SYNC();                                               // the previous tile has been read
    for (int idx = SC_TID; idx < in_rows * in_cols; idx += 256) {
      const int r = idx / in_cols, cc = idx - r * in_cols;
      const int ri = row_lo + r, ci = col_lo + cc;
      L[r * DC_LW + cc] = ri >= 0 && ri < g.hf && ci >= 0 && ci < g.wf ? xc[(long long)ri * g.wf + ci] : 0.f;
    }
    SC_SYNC();
    // a value read from LDS serves every output channel of the block
    const float* wp = w + ((long long)(grp * cout_g + o_lo) * cin_g + c) * taps;
#pragma unroll 1
    for (int t1 = 0; t1 < g.ph; ++t1) {
#pragma unroll 1
      for (int t2 = 0; t2 < g.pw; ++t2) {
        float xv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[r] = r < rpw ? Ll[(4 * r * g.sh + t1) * DC_LW + t2] : 0.f;
#pragma unroll
        for (int j = 0; j < DC_OCB; ++j) {
          if (j < n_o) {
            const float wv = wp[(long long)j * cin_g * taps + t1 * g.pw + t2];   // workgroup-uniform
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] = fmaf(wv, xv[r], acc[j][r]);
          }
        }
      }
    }
  }
  const int i2 = col0 + lane;
  const long long oplane = (long long)g.hc * g.wc;
#pragma unroll
  for (int j = 0; j < DC_OCB; ++j) {
    if (j < n_o) {
      const int o = grp * cout_g + o_lo + j;
      const float bv = bias ? bias[o] : 0.f;
      float* yo = y + ((long long)bb * a.cc_out + o) * oplane + i2;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = wave + 4 * r;
        if (r < rpw && i2 < g.wc && rr < rt) yo[(long long)(row0 + rr) * g.wc] = acc[j][r] + bv;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- C^T, a gather
// gc (B, cc_out, hc, wc), w = wt of k_disco_fold (cc_in, cout_g, taps, flipped), y (B, cc_in, hf, wf)
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_disco_convT(const float* __restrict__ gc, const float* __restrict__ w, const float* __restrict__ bias,
              float* __restrict__ y, const DcArgs a) {
  SC_SHARED float L[DC_LH * DT_LW];
  const DcGeom g = a.g;
  int b = SC_BID_X;
  const int tc = b % g.tiles_c;
  b /= g.tiles_c;
  const int tr = b % g.tiles_r;
  b /= g.tiles_r;
  const int cb = b % a.n_blk;
  b /= a.n_blk;
  const int grp = b % a.groups;
  const int bb = b / a.groups;
  const int cin_g = a.cc_in / a.groups, cout_g = a.cc_out / a.groups;
  const int u0 = tr * DT_TR, v0 = tc * DC_TC;
  const int rt = g.hf - u0 < DT_TR ? g.hf - u0 : DT_TR;
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int c_lo = cb * DC_OCB;
  const int n_c = cin_g - c_lo < DC_OCB ? cin_g - c_lo : DC_OCB;
  const int taps = g.ph * g.pw;
  // the coarse rows / columns any point of the tile reads
  const int p_lo = dc_floordiv(u0 + g.padh - (g.ph - 1), g.sh), p_hi = (u0 + rt - 1 + g.padh) / g.sh;
  const int q_lo = dc_floordiv(v0 + g.padw - (g.pw - 1), g.sw), q_hi = (v0 + DC_TC - 1 + g.padw) / g.sw;
  const int rows = p_hi - p_lo + 1, cols = q_hi - q_lo + 1;
  const long long cplane = (long long)g.hc * g.wc;
  const int bvv = v0 + lane + g.padw;
  const int j0 = bvv % g.sw, qb = bvv / g.sw - q_lo;
  float acc[DC_OCB][4];
#pragma unroll
  for (int j = 0; j < DC_OCB; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;

#pragma unroll 1
  for (int o = 0; o < cout_g; ++o) {
    const float* go = gc + ((long long)bb * a.cc_out + grp * cout_g + o) * cplane;
    SC_SYNC();                                               // the previous tile has been read
    for (int idx = SC_TID; idx < rows * cols; idx += 256) {
      const int r = idx / cols, cc = idx - r * cols;
      const int ri = p_lo + r, ci = q_lo + cc;
      L[r * DT_LW + cc] = ri >= 0 && ri < g.hc && ci >= 0 && ci < g.wc ? go[(long long)ri * g.wc + ci] : 0.f;
    }
    SC_SYNC();
    // a value read from LDS serves every channel of the block
    const float* wp = w + ((long long)(grp * cin_g + c_lo) * cout_g + o) * taps + (taps - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ur = wave + 4 * r;                           // wave-uniform
      if (ur < rt) {
        const int bu = u0 + ur + g.padh;
        const int pb = bu / g.sh - p_lo;
#pragma unroll 1
        for (int i = bu % g.sh, m = 0; i < g.ph; i += g.sh, ++m) {
          const float* Lr = L + (pb - m) * DT_LW + qb;
          const float* wr = wp - i * g.pw;                     // flipped: tap (i, j) at taps - 1 - (i pw + j)
#pragma unroll 1
          for (int j = j0, n = 0; j < g.pw; j += g.sw, ++n) {
            const float lv = Lr[-n];
#pragma unroll
            for (int jc = 0; jc < DC_OCB; ++jc)
              if (jc < n_c) acc[jc][r] = fmaf(wr[(long long)jc * cout_g * taps - j], lv, acc[jc][r]);
          }
        }
      }
    }
  }
  const int v = v0 + lane;
  const long long fplane = (long long)g.hf * g.wf;
#pragma unroll
  for (int jc = 0; jc < DC_OCB; ++jc) {
    if (jc < n_c) {
      const int c = grp * cin_g + c_lo + jc;
      const float bv = bias ? bias[c] : 0.f;
      float* yo = y + ((long long)bb * a.cc_in + c) * fplane + v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ur = wave + 4 * r;
        if (v < g.wf && ur < rt) yo[(long long)(u0 + ur) * g.wf] = acc[jc][r] + bv;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- matrix-core route
template <int NOB>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_disco_mfma(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
             float* __restrict__ y, const FdArgs a) {
  fdm_conv<NOB, true>(x, w, bias, y, a);
}

// ------------------------------------------------------------------------------------------------- weight gradient
struct DcWgArgs {
  DcGeom g;                    // tiles of the coarse grid
  int batch, cc_in, cc_out, groups;
  int chunks;
  long long units, per_chunk;  // units = batch x tiles
};

// grid: (((o * cin_g + c) * ph + i) * chunks + chunk); ws ([chunks][cc_out][cin_g][taps]) receives the pw taps of row i
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_disco_wgrad(const float* __restrict__ xf, const float* __restrict__ gc, float* __restrict__ ws, const DcWgArgs a) {
  constexpr int NB = 8;
  SC_SHARED float L[16 * DC_LW];
  SC_SHARED float red[NB * 256];
  const DcGeom g = a.g;
  int b = SC_BID_X;
  const int chunk = b % a.chunks;
  b /= a.chunks;
  const int ti = b % g.ph;
  b /= g.ph;
  const int cin_g = a.cc_in / a.groups, cout_g = a.cc_out / a.groups;
  const int c = b % cin_g;
  const int o = b / cin_g;
  const int grp = o / cout_g;
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int rpw = g.tr >> 2;
  const int in_cols = (DC_TC - 1) * g.sw + g.pw;
  const long long fplane = (long long)g.hf * g.wf, cplane = (long long)g.hc * g.wc;
  float acc[2 * NB];
#pragma unroll
  for (int j = 0; j < 2 * NB; ++j) acc[j] = 0.f;
  const long long u_lo = chunk * a.per_chunk;
  const long long u_hi = u_lo + a.per_chunk < a.units ? u_lo + a.per_chunk : a.units;
#pragma unroll 1
  for (long long unit = u_lo; unit < u_hi; ++unit) {
    long long qq = unit;
    const int tc = (int)(qq % g.tiles_c);
    qq /= g.tiles_c;
    const int tr = (int)(qq % g.tiles_r);
    const int bb = (int)(qq / g.tiles_r);
    const int row0 = tr * g.tr, col0 = tc * DC_TC;
    const int rt = g.hc - row0 < g.tr ? g.hc - row0 : g.tr;
    const int col_lo = col0 * g.sw - g.padw;
    const float* xc = xf + ((long long)bb * a.cc_in + grp * cin_g + c) * fplane;
    SC_SYNC();                                               // the previous tile has been read
    for (int idx = SC_TID; idx < rt * in_cols; idx += 256) { // LDS row r: the fine row coarse row r reads through tap row ti
      const int r = idx / in_cols, cc = idx - r * in_cols;
      const int ri = (row0 + r) * g.sh + ti - g.padh, ci = col_lo + cc;
      L[r * DC_LW + cc] = ri >= 0 && ri < g.hf && ci >= 0 && ci < g.wf ? xc[(long long)ri * g.wf + ci] : 0.f;
    }
    SC_SYNC();
    const int i2 = col0 + lane;
    const float* gp = gc + ((long long)bb * a.cc_out + o) * cplane + i2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = wave + 4 * r;
      if (r >= rpw || rr >= rt) continue;                    // (wave-uniform) LDS rows past the tile were never written
      const float gv = i2 < g.wc ? gp[(long long)(row0 + rr) * g.wc] : 0.f;
      const float* Lr = L + rr * DC_LW + lane * g.sw;
#pragma unroll
      for (int j = 0; j < DC_MAX_P; ++j)
        if (j < g.pw) acc[j] = fmaf(gv, Lr[j], acc[j]);
    }
  }
  float* out = ws + (((long long)chunk * a.cc_out + o) * cin_g + c) * (g.ph * g.pw) + ti * g.pw;
#pragma unroll
  for (int bt = 0; bt < 2; ++bt) {
    SC_SYNC();                                               // the previous batch has been read
#pragma unroll
    for (int j = 0; j < NB; ++j) red[j * 256 + SC_TID] = acc[bt * NB + j];
    fd_block_sum<NB>(red);
    if (SC_TID < NB) {
      const int tap = bt * NB + SC_TID;
      if (tap < g.pw) out[tap] = red[SC_TID * 256];
    }
  }
}

// G[i] = sum_p ws[p][i] in index order of p, written over partial 0 (thread i alone touches entry i of it): coalesced
// over i, so the projection below reads one partial whatever the chunk count
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_disco_psum(float* __restrict__ ws, const long long wn, const int parts) {
  const long long i = (long long)SC_BID_X * 256 + SC_TID;
  if (i >= wn) return;
  float s = 0.f;
  for (int p = 0; p < parts; ++p) s += ws[p * wn + i];
  ws[i] = s;
}

// workgroups [0, w_blocks): one thread per weight entry (o, c, k):  gw = q sum_t psi[k, t] (sum_p ws[p][o, c, t]), p in
// index order.  Workgroups from w_blocks on: gbias[o] = sum over (b, point) of gout[b, o, point], thread t takes the
// points t, t + 256, .. of every batch entry in order, then the tree of fd_block_sum.
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_disco_wreduce(const float* __restrict__ ws, const float* __restrict__ psi, const float* __restrict__ gout,
                float* __restrict__ gw, float* __restrict__ gbias, const long long n_w, const int nk, const int taps,
                const int parts, const float q, const int w_blocks, const int batch, const int c_out,
                const long long pts) {
  SC_SHARED float red[256];
  if (SC_BID_X < w_blocks) {
    const long long i = (long long)SC_BID_X * 256 + SC_TID;
    if (i >= n_w) return;
    const long long oc = i / nk;
    const int k = (int)(i - oc * nk);
    const long long wn = n_w / nk * taps;
    float s = 0.f;
    for (int t = 0; t < taps; ++t) {
      float gt = 0.f;
      for (int p = 0; p < parts; ++p) gt += ws[p * wn + oc * taps + t];
      s = fmaf(psi[(long long)k * taps + t], gt, s);
    }
    gw[i] = q * s;
    return;
  }
  const int o = SC_BID_X - w_blocks;
  float s = 0.f;
  for (int b = 0; b < batch; ++b) {
    const float* gp = gout + ((long long)b * c_out + o) * pts;
    for (long long idx = SC_TID; idx < pts; idx += 256) s += gp[idx];
  }
  red[SC_TID] = s;
  fd_block_sum<1>(red);
  if (SC_TID == 0) gbias[o] = red[0];
}
