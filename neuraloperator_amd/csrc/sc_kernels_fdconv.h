// sc_kernels_fdconv.h -- the finite-difference convolution of the local neural operator
// (neuralop/layers/differential_conv.py:6-101, FiniteDifferenceConvolution):
//
//   y = (conv_pad(x, W) - conv_1x1(x, sum_taps W)) / h          x (B, C_in, d..), W (C_out, C_in / groups, k..k), k odd
//
// The 1 x 1 term is the centre tap, so the layer is ONE convolution with folded weights W' (k_fdconv_fold):
//   W'[.., t] = W[.., t] / h (t != centre),   W'[.., centre] = -(sum over t != centre of W[.., t]) / h
// and its gradients are   gx = adjoint of (pad, conv W'),   gW[.., t] = (G[.., t] - G[.., centre]) / h,
//   G[o, c, t] = sum_{b, p} gout[b, o, p] xpad[b, c, p + t]   (gW[.., centre] = 0 exactly).
//
// Fields are handled as 3-d (d0, d1, d2), d2 contiguous, missing leading axes of extent 1 with one tap.  Padding maps a
// coordinate q outside [0, n) to a source index per axis (fd_map): periodic q mod n (right for extents 1, 2, 3, where
// taps alias), zeros none (0 is written into LDS), replicate clamped, reflect mirrored; nothing outside the buffer is
// ever addressed (a coordinate no padding rule reaches is a zero).
//
//   k_fdconv<ND>           general route, vector ALU: any channel counts, groups, k = 3 / 5 / 7, the four modes.  A
//                          workgroup of 4 waves owns FD_TR x FD_TC points of the last two axes of one output plane and
//                          FD_OCB output channels of one group; per input channel (and, 3-d, per tap of the first axis:
//                          the neighbouring plane) it loads the tile plus its halo into LDS once, in coalesced rows,
//                          and every lane accumulates its column.  A wave stores whole row segments in lane order.
//                          `ext` > 0 computes the FULL correlation on the padded domain (output extents d + 2 ext).
//   k_fdconv_mfma<NOB>     dense 2-d k = 3 route, C_in, C_out in {32, 64, 128}, periodic / zeros: implicit GEMM over
//                          (tap, input channel) on v_mfma_f32_32x32x2_f32 (exact fp32).  Per FDM_CK input channels the
//                          input tile with its halo and the weight slice [tap][channel][C_out] are staged in LDS; the
//                          nine shifted views of the one tile feed the B operand, a wave owns one tile row.
//   k_fdconv_wgrad<K>      per-workgroup partial G of one (o, c, first-axis tap) over a chunk of tiles, vector ALU
//   k_fdconv_wgrad_mfma    the same for a 32 x 32 block of (o, c) on the matrix cores, one partial per wave
//   k_fdconv_wreduce       partials summed in index order, (G_t - G_c) / h
//   k_fdconv_unpad         replicate / reflect data gradient: sums each input point's pre-images in a fixed order
//
// The data gradient for periodic / zeros is k_fdconv / k_fdconv_mfma on gout with the flipped, channel-transposed
// weights (also written by k_fdconv_fold).  No float atomics, every sum in a fixed order: two launches give the same
// bits.  No register array is indexed at run time.
#pragma once
#include "sc_device.h"
#include "sc_kernels_mfma.h"

#define FD_PERIODIC 0
#define FD_ZEROS 1
#define FD_REPLICATE 2
#define FD_REFLECT 3

#define FD_TC 64               // tile columns = one wave
#define FD_TR 16               // tile rows: 4 per wave
#define FD_RPW (FD_TR / 4)
#define FD_OCB 4               // output channels of one workgroup
#define FD_LW (FD_TC + 8)      // LDS row: 3 + 64 + 3, padded to 72
#define FD_LH (FD_TR + 6)

#define FDM_TR 4               // matrix-core route: tile rows = waves
#define FDM_TC 32              // tile columns = the N extent of one matrix tile
#define FDM_CK 8               // input channels staged per round
#define FDM_XH (FDM_TR + 2)
#define FDM_XW 36              // 1 + 32 + 1, padded
#define FDM_XC 224             // floats per staged input channel (6 x 36, padded: the two k rows of a matrix tile 32 banks apart)
#define FDM_WS(co) ((co) + 32) // floats per staged weight row [C_out], padded likewise
#define FDM_GS 130             // wgrad: floats per gout channel in LDS (4 x 32 + 2: bank 2 o + k, conflict-free)
#define FDM_XS 218             // wgrad: floats per x channel in LDS (6 x 36 + 2: bank 26 c + k, conflict-free)

struct FdGeom {
  int d0, d1, d2;              // input extents, d2 contiguous
  int o0, o1, o2;              // output extents: d + 2 ext
  int e0, e1, e2;              // ext per axis (0, or r for the full correlation)
  int k0, k1, k2;              // taps per axis (1 on a missing axis)
  int r0, r1, r2;              // k / 2 per axis
  int mode;
  int tiles_r, tiles_c;        // tiles per output plane
};

struct FdArgs {
  FdGeom g;
  int c_in, c_out, groups;     // of THIS convolution (the data gradient swaps the two counts)
  int n_oblk;                  // blocks of FD_OCB output channels per group
};

// source index of coordinate q on an axis of extent n, or -1: the value is 0
SC_DEVICE int fd_map(int q, const int n, const int mode) {
  if (q >= 0 && q < n) return q;
  if (mode == FD_ZEROS) return -1;
  if (mode == FD_PERIODIC) {
    q %= n;
    return q < 0 ? q + n : q;
  }
  if (mode == FD_REPLICATE) return q < 0 ? 0 : n - 1;
  q = q < 0 ? -q : 2 * (n - 1) - q;
  return q >= 0 && q < n ? q : -1;
}

// L[r][c] = plane value at rows row_lo + r, columns col_lo + c through the index maps, r < rows, c < cols
SC_DEVICE void fd_load_tile(float* L, const int lw, const float* __restrict__ p, const FdGeom& g, const int row_lo,
                            const int col_lo, const int rows, const int cols) {
  for (int idx = SC_TID; idx < rows * lw; idx += 256) {
    const int r = idx / lw, c = idx - r * lw;
    if (c < cols) {
      const int ri = fd_map(row_lo + r, g.d1, g.mode), ci = fd_map(col_lo + c, g.d2, g.mode);
      L[idx] = ri < 0 || ci < 0 ? 0.f : p[(long long)ri * g.d2 + ci];
    }
  }
}

// ------------------------------------------------------------------------------------------------- folded weights
// one thread per (o, c): wf (C_out, cin_g, taps) = W', wt (C_in, cout_g, taps) = W' with the taps reversed and the two
// channel indices exchanged inside each group
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_fdconv_fold(const float* __restrict__ w, float* __restrict__ wf, float* __restrict__ wt, float* __restrict__ wfm,
              float* __restrict__ wtm, const int c_out, const int cin_g, const int cout_g, const int taps,
              const float inv_h) {
  const long long i = (long long)SC_BID_X * 256 + SC_TID;
  if (i >= (long long)c_out * cin_g) return;
  const int o = (int)(i / cin_g), c = (int)(i - (long long)o * cin_g);
  const int grp = o / cout_g, ol = o - grp * cout_g;
  const float* ws = w + i * taps;
  float* f = wf + i * taps;
  float* t = wt + ((long long)(grp * cin_g + c) * cout_g + ol) * taps;
  const int centre = taps / 2;
  float s = 0.f;
  for (int j = 0; j < taps; ++j) {
    if (j == centre) continue;
    const float v = ws[j];
    s += v;
    const float q = v * inv_h;
    f[j] = q;
    t[taps - 1 - j] = q;
  }
  const float q = -s * inv_h;
  f[centre] = q;
  t[centre] = q;
  if (wfm) {                                                 // matrix-core route (groups 1, 9 taps): round-major copies
    for (int j = 0; j < 9; ++j) {                            // [c / 8][tap][c % 8][o] of W', [o / 8][tap][o % 8][c] of its transpose
      wfm[(((long long)(c / FDM_CK) * 9 + j) * FDM_CK + c % FDM_CK) * c_out + o] = f[j];
      wtm[(((long long)(o / FDM_CK) * 9 + j) * FDM_CK + o % FDM_CK) * cin_g + c] = t[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------- general route
template <int ND>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_fdconv(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, const FdArgs a) {
  SC_SHARED float L[FD_LH * FD_LW];
  const FdGeom g = a.g;
  int b = SC_BID_X;
  const int tc = b % g.tiles_c;
  b /= g.tiles_c;
  const int tr = b % g.tiles_r;
  b /= g.tiles_r;
  const int i0 = b % g.o0;
  b /= g.o0;
  const int ob = b % a.n_oblk;
  b /= a.n_oblk;
  const int grp = b % a.groups;
  const int bb = b / a.groups;
  const int cin_g = a.c_in / a.groups, cout_g = a.c_out / a.groups;
  const int row0 = tr * FD_TR, col0 = tc * FD_TC;
  const int rt = g.o1 - row0 < FD_TR ? g.o1 - row0 : FD_TR;           // rows of this tile
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int o_lo = ob * FD_OCB;
  const int n_o = cout_g - o_lo < FD_OCB ? cout_g - o_lo : FD_OCB;
  const int k0 = ND == 3 ? g.k0 : 1, k1 = ND >= 2 ? g.k1 : 1, k2 = g.k2;
  const int taps = k0 * k1 * k2;
  const long long plane = (long long)g.d1 * g.d2, img = plane * g.d0;
  float acc[FD_OCB][FD_RPW];
#pragma unroll
  for (int j = 0; j < FD_OCB; ++j)
#pragma unroll
    for (int r = 0; r < FD_RPW; ++r) acc[j][r] = 0.f;
  const float* Ll = L + wave * FD_LW + lane;

#pragma unroll 1
  for (int c = 0; c < cin_g; ++c) {
    const float* xc = x + ((long long)bb * a.c_in + grp * cin_g + c) * img;
#pragma unroll 1
    for (int t0 = 0; t0 < k0; ++t0) {
      const int p0 = ND == 3 ? fd_map(i0 - g.e0 - g.r0 + t0, g.d0, g.mode) : 0;
      if (p0 < 0) continue;                                  // a plane of zeros (uniform over the workgroup)
      SC_SYNC();                                             // the previous tile has been read
      fd_load_tile(L, FD_LW, xc + p0 * plane, g, row0 - g.e1 - g.r1, col0 - g.e2 - g.r2, rt + 2 * g.r1,
                   FD_TC + 2 * g.r2);
      SC_SYNC();
#pragma unroll
      for (int j = 0; j < FD_OCB; ++j) {
        if (j < n_o) {
          const float* wp = w + ((long long)(grp * cout_g + o_lo + j) * cin_g + c) * taps + t0 * k1 * k2;
#pragma unroll 1
          for (int t1 = 0; t1 < k1; ++t1) {
#pragma unroll 1
            for (int t2 = 0; t2 < k2; ++t2) {
              const float wv = wp[t1 * k2 + t2];               // workgroup-uniform
#pragma unroll
              for (int r = 0; r < FD_RPW; ++r) acc[j][r] = fmaf(wv, Ll[(4 * r + t1) * FD_LW + t2], acc[j][r]);
            }
          }
        }
      }
    }
  }
  const int i2 = col0 + lane;
  const long long oplane = (long long)g.o1 * g.o2;
#pragma unroll
  for (int j = 0; j < FD_OCB; ++j) {
    if (j < n_o) {
      float* yo = y + (((long long)bb * a.c_out + grp * cout_g + o_lo + j) * g.o0 + i0) * oplane + i2;
#pragma unroll
      for (int r = 0; r < FD_RPW; ++r) {
        const int rr = wave + 4 * r;
        if (i2 < g.o2 && rr < rt) yo[(long long)(row0 + rr) * g.o2] = acc[j][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- matrix-core route
// one round of k_fdconv_mfma's operands into registers: channel c0 + c of this thread's tile position, and the weight
// entries SC_TID + 256 j of the round's slice [tap][c % 8][C_out] of the round-major copy (72 C_out contiguous floats)
template <int NOB>
SC_DEVICE void fdm_fetch(float (&xr)[FDM_CK], float (&wr)[9 * NOB], const float* __restrict__ xb,
                         const float* __restrict__ w, const long long xoff, const long long plane, const int c0) {
#pragma unroll
  for (int c = 0; c < FDM_CK; ++c) xr[c] = xoff >= 0 ? xb[(c0 + c) * plane + xoff] : 0.f;
#pragma unroll
  for (int j = 0; j < 9 * NOB; ++j) wr[j] = w[(long long)c0 * (9 * 32 * NOB) + SC_TID + 256 * j];
}

// x (B, C_in, d1, d2), w the round-major folded copy [C_in / 8][9][8][C_out], y (B, C_out, d1, d2); NOB = C_out / 32.  Lane l of a wave supplies
// A[o = l & 31][k = l >> 5] = W'[32 ob + o][c + k][t] and B[k][j = l & 31] = xpad[c + k][row + t1][col0 + j + t2], and
// owns D[o = (v & 3) + 8 (v >> 2) + 4 (l >> 5)][j = l & 31] (sc_kernels_mfma.h).
// BIAS: bias[o] (a null pointer: none) is added in the store -- the discrete-continuous convolution
// (sc_kernels_disco.h) runs this body with its own folded weights; the finite-difference layer has no bias.
template <int NOB, bool BIAS>
SC_DEVICE void fdm_conv(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                        float* __restrict__ y, const FdArgs& a) {
  constexpr int CO = 32 * NOB;
  constexpr int WS = FDM_WS(CO);
  SC_SHARED float Lx[FDM_CK * FDM_XC];
  SC_SHARED float Lw[9 * FDM_CK * WS];
  const FdGeom g = a.g;
  int b = SC_BID_X;
  const int tc = b % g.tiles_c;
  b /= g.tiles_c;
  const int tr = b % g.tiles_r;
  const int bb = b / g.tiles_r;
  const int row0 = tr * FDM_TR, col0 = tc * FDM_TC;
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int lj = lane & 31, lk = lane >> 5;
  const long long plane = (long long)g.d1 * g.d2;
  sc_f32x16 acc[NOB];
#pragma unroll
  for (int u = 0; u < NOB; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[u][v] = 0.f;

  // staging: thread t < 6 x 36 owns ONE position of the input tile (halo included) for every channel and 9 NOB weight
  // entries of a round.  Its source offset is fixed for the workgroup, so the index maps run once, and the next round's
  // values are requested before this round's matrix work and land in registers meanwhile.
  const int pr = SC_TID / FDM_XW, pc = SC_TID - pr * FDM_XW;
  long long xoff = -1;
  if (SC_TID < FDM_XH * FDM_XW && pc < FDM_TC + 2) {
    const int ri = fd_map(row0 - 1 + pr, g.d1, g.mode), ci = fd_map(col0 - 1 + pc, g.d2, g.mode);
    if (ri >= 0 && ci >= 0) xoff = (long long)ri * g.d2 + ci;
  }
  const float* xb = x + (long long)bb * a.c_in * plane;
  float xr[FDM_CK], wr[9 * NOB];
  fdm_fetch<NOB>(xr, wr, xb, w, xoff, plane, 0);
#pragma unroll 1
  for (int c0 = 0; c0 < a.c_in; c0 += FDM_CK) {
    SC_SYNC();                                               // the previous round has been read
    if (SC_TID < FDM_XH * FDM_XW) {
#pragma unroll
      for (int c = 0; c < FDM_CK; ++c) Lx[c * FDM_XC + SC_TID] = xr[c];
    }
#pragma unroll
    for (int j = 0; j < 9 * NOB; ++j) {
      const int idx = SC_TID + 256 * j;                       // row (tap, channel) = idx / CO, a power of two
      Lw[(idx / CO) * WS + (idx & (CO - 1))] = wr[j];
    }
    SC_SYNC();
    if (c0 + FDM_CK < a.c_in) fdm_fetch<NOB>(xr, wr, xb, w, xoff, plane, c0 + FDM_CK);
    // two-level sum: the 72 products of a round form a partial of their own, the rounds are then added -- the chain
    // of roundings an output sees is 72 + C_in / 8 long instead of 9 C_in
    sc_f32x16 part[NOB];
#pragma unroll
    for (int u = 0; u < NOB; ++u)
#pragma unroll
      for (int v = 0; v < 16; ++v) part[u][v] = 0.f;
#pragma unroll
    for (int t1 = 0; t1 < 3; ++t1) {
#pragma unroll
      for (int t2 = 0; t2 < 3; ++t2) {
#pragma unroll
        for (int cc = 0; cc < FDM_CK / 2; ++cc) {
          const int c = 2 * cc + lk;
          const float bv = Lx[c * FDM_XC + (wave + t1) * FDM_XW + lj + t2];
          const float* ap = Lw + ((t1 * 3 + t2) * FDM_CK + c) * WS + lj;
#pragma unroll
          for (int u = 0; u < NOB; ++u) sc_mfma_32x32x2(part[u], ap[32 * u], bv);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NOB; ++u)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[u][v] += part[u][v];
  }
  const int row = row0 + wave, col = col0 + lj;
  if (row < g.d1 && col < g.d2) {
#pragma unroll
    for (int u = 0; u < NOB; ++u) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int o = 32 * u + (v & 3) + 8 * (v >> 2) + 4 * lk;
        float r = acc[u][v];
        if (BIAS) {
          if (bias) r += bias[o];
        }
        y[((long long)bb * a.c_out + o) * plane + (long long)row * g.d2 + col] = r;
      }
    }
  }
}

template <int NOB>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_fdconv_mfma(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, const FdArgs a) {
  fdm_conv<NOB, false>(x, w, nullptr, y, a);
}

// ------------------------------------------------------------------------------------------------- weight gradient
struct FdWgArgs {
  FdGeom g;                    // ext 0: the forward geometry
  int batch, c_in, c_out, groups;
  int chunks;
  long long units, per_chunk;  // units = batch x d0 x tiles (general) or batch x tiles (matrix cores)
};

// fixed-order sum of NB values over the 256 threads of a workgroup: red[j * 256 + t] holds thread t's j-th value on
// entry (written by the caller after a barrier), the sums are red[j * 256] on return
template <int NB>
SC_DEVICE void fd_block_sum(float* red) {
  const int t = SC_TID;
  for (int w = 128; w > 0; w >>= 1) {
    SC_SYNC();
    if (t < w) {
#pragma unroll
      for (int j = 0; j < NB; ++j) red[j * 256 + t] += red[j * 256 + t + w];
    }
  }
  SC_SYNC();
}

// grid: (((o * cin_g + c) * k0 + t0) * chunks + chunk); ws ([chunks][C_out][cin_g][taps]) receives the K1 x K taps of t0
template <int K>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_fdconv_wgrad(const float* __restrict__ x, const float* __restrict__ gout, float* __restrict__ ws, const FdWgArgs a) {
  constexpr int NB = 8;
  SC_SHARED float L[FD_LH * FD_LW];
  SC_SHARED float red[NB * 256];
  const FdGeom g = a.g;
  int b = SC_BID_X;
  const int chunk = b % a.chunks;
  b /= a.chunks;
  const int t0 = b % g.k0;
  b /= g.k0;
  const int cin_g = a.c_in / a.groups, cout_g = a.c_out / a.groups;
  const int c = b % cin_g;
  const int o = b / cin_g;
  const int grp = o / cout_g;
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int k1 = g.k1;                                       // 1 (1-d) or K
  const long long plane = (long long)g.d1 * g.d2, img = plane * g.d0;
  float acc[K * K];
#pragma unroll
  for (int j = 0; j < K * K; ++j) acc[j] = 0.f;
  const float* Ll = L + wave * FD_LW + lane;
  const long long u_lo = chunk * a.per_chunk;
  const long long u_hi = u_lo + a.per_chunk < a.units ? u_lo + a.per_chunk : a.units;
#pragma unroll 1
  for (long long unit = u_lo; unit < u_hi; ++unit) {
    long long q = unit;
    const int tc = (int)(q % g.tiles_c);
    q /= g.tiles_c;
    const int tr = (int)(q % g.tiles_r);
    q /= g.tiles_r;
    const int i0 = (int)(q % g.d0);
    const int bb = (int)(q / g.d0);
    const int p0 = fd_map(i0 - g.r0 + t0, g.d0, g.mode);
    if (p0 < 0) continue;                                    // a plane of zeros (uniform over the workgroup)
    const int row0 = tr * FD_TR, col0 = tc * FD_TC;
    const int rt = g.d1 - row0 < FD_TR ? g.d1 - row0 : FD_TR;
    SC_SYNC();                                               // the previous tile has been read
    fd_load_tile(L, FD_LW, x + ((long long)bb * a.c_in + grp * cin_g + c) * img + p0 * plane, g, row0 - g.r1,
                 col0 - g.r2, rt + 2 * g.r1, FD_TC + 2 * g.r2);
    SC_SYNC();
    const int i2 = col0 + lane;
    const float* gp = gout + ((long long)bb * a.c_out + o) * img + i0 * plane + i2;
#pragma unroll
    for (int r = 0; r < FD_RPW; ++r) {
      const int rr = wave + 4 * r;
      if (rr >= rt) continue;                                // (wave-uniform) LDS rows past the tile were never written
      const float gv = i2 < g.d2 ? gp[(long long)(row0 + rr) * g.d2] : 0.f;
#pragma unroll
      for (int t1 = 0; t1 < K; ++t1) {
        if (t1 < k1) {
#pragma unroll
          for (int t2 = 0; t2 < K; ++t2) acc[t1 * K + t2] = fmaf(gv, Ll[(4 * r + t1) * FD_LW + t2], acc[t1 * K + t2]);
        }
      }
    }
  }
  const int taps = g.k0 * g.k1 * g.k2;
  float* out = ws + (((long long)chunk * a.c_out + o) * cin_g + c) * taps + t0 * (k1 * K);
#pragma unroll
  for (int bt = 0; bt < (K * K + NB - 1) / NB; ++bt) {
    SC_SYNC();                                               // the previous batch has been read
#pragma unroll
    for (int j = 0; j < NB; ++j) red[j * 256 + SC_TID] = bt * NB + j < K * K ? acc[bt * NB + j < K * K ? bt * NB + j : 0] : 0.f;
    fd_block_sum<NB>(red);
    if (SC_TID < NB) {
      const int tap = bt * NB + SC_TID;
      if (tap < k1 * K) out[tap] = red[SC_TID * 256];
    }
  }
}

// the operands of one unit of k_fdconv_wgrad_mfma into registers: thread t < 6 x 36 owns one position of the x tile
// (halo included) for the 32 input channels of the block, and every thread position t & 127 of the gout tile for the
// output channels 2 j + (t >> 7)
SC_DEVICE void fdm_wg_fetch(float (&xr)[32], float (&gr)[16], const float* __restrict__ x,
                            const float* __restrict__ gout, const FdWgArgs& a, const int cb, const int ob,
                            const long long unit) {
  const FdGeom& g = a.g;
  long long q = unit;
  const int tc = (int)(q % g.tiles_c);
  q /= g.tiles_c;
  const int tr = (int)(q % g.tiles_r);
  const int bb = (int)(q / g.tiles_r);
  const int row0 = tr * FDM_TR, col0 = tc * FDM_TC;
  const long long plane = (long long)g.d1 * g.d2;
  const int pr = SC_TID / FDM_XW, pc = SC_TID - pr * FDM_XW;
  long long xoff = -1;
  if (SC_TID < FDM_XH * FDM_XW && pc < FDM_TC + 2) {
    const int ri = fd_map(row0 - 1 + pr, g.d1, g.mode), ci = fd_map(col0 - 1 + pc, g.d2, g.mode);
    if (ri >= 0 && ci >= 0) xoff = (long long)ri * g.d2 + ci;
  }
  const float* xb = x + ((long long)bb * a.c_in + 32 * cb) * plane;
#pragma unroll
  for (int c = 0; c < 32; ++c) xr[c] = xoff >= 0 ? xb[c * plane + xoff] : 0.f;
  const int pos = SC_TID & 127, r = pos >> 5, cc = pos & 31;
  const bool in = row0 + r < g.d1 && col0 + cc < g.d2;
  const float* gb = gout + ((long long)bb * a.c_out + 32 * ob + (SC_TID >> 7)) * plane + (long long)(row0 + r) * g.d2 +
                    col0 + cc;
#pragma unroll
  for (int j = 0; j < 16; ++j) gr[j] = in ? gb[2 * j * plane] : 0.f;
}

// dense 2-d k = 3 on the matrix cores: grid ((ob * (C_in / 32) + cb) * chunks + chunk), a unit = one FDM_TR x FDM_TC
// tile of one batch entry.  Lane l supplies A[o = l & 31][k = l >> 5] = gout[32 ob + o][point 2 kk + k of the wave's
// row] and B[k][c = l & 31] = xpad[32 cb + c][that point + tap]; nine accumulators, one per tap.
// ws ([chunks * 4][C_out][C_in][9]): one partial per wave.
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_fdconv_wgrad_mfma(const float* __restrict__ x, const float* __restrict__ gout, float* __restrict__ ws,
                    const FdWgArgs a) {
  SC_SHARED float Lg[32 * FDM_GS];
  SC_SHARED float Lx[32 * FDM_XS];
  int b = SC_BID_X;
  const int chunk = b % a.chunks;
  b /= a.chunks;
  const int ncb = a.c_in / 32;
  const int cb = b % ncb, ob = b / ncb;
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int lj = lane & 31, lk = lane >> 5;
  sc_f32x16 acc[9];
#pragma unroll
  for (int u = 0; u < 9; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[u][v] = 0.f;
  const long long u_lo = chunk * a.per_chunk;
  const long long u_hi = u_lo + a.per_chunk < a.units ? u_lo + a.per_chunk : a.units;
  // the next unit's operands are requested before this unit's matrix work and land in registers meanwhile
  float xr[32], gr[16];
  if (u_lo < u_hi) fdm_wg_fetch(xr, gr, x, gout, a, cb, ob, u_lo);
#pragma unroll 1
  for (long long unit = u_lo; unit < u_hi; ++unit) {
    SC_SYNC();                                               // the previous tile has been read
    if (SC_TID < FDM_XH * FDM_XW) {
#pragma unroll
      for (int c = 0; c < 32; ++c) Lx[c * FDM_XS + SC_TID] = xr[c];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) Lg[(2 * j + (SC_TID >> 7)) * FDM_GS + (SC_TID & 127)] = gr[j];
    SC_SYNC();
    if (unit + 1 < u_hi) fdm_wg_fetch(xr, gr, x, gout, a, cb, ob, unit + 1);
#pragma unroll 1
    for (int kk = 0; kk < FDM_TC / 2; ++kk) {
      const int p = 2 * kk + lk;
      const float av = Lg[lj * FDM_GS + wave * FDM_TC + p];
      const float* xp = Lx + lj * FDM_XS + wave * FDM_XW + p;
#pragma unroll
      for (int t1 = 0; t1 < 3; ++t1)
#pragma unroll
        for (int t2 = 0; t2 < 3; ++t2) sc_mfma_32x32x2(acc[t1 * 3 + t2], av, xp[t1 * FDM_XW + t2]);
    }
  }
  float* out = ws + ((long long)(chunk * 4 + wave) * a.c_out) * a.c_in * 9;
#pragma unroll
  for (int u = 0; u < 9; ++u) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int o = 32 * ob + (v & 3) + 8 * (v >> 2) + 4 * lk;
      out[((long long)o * a.c_in + 32 * cb + lj) * 9 + u] = acc[u][v];
    }
  }
}

// gw[i, t] = (sum_p ws[p][i][t] - sum_p ws[p][i][centre]) / h in index order of p; the centre tap is exactly 0
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_fdconv_wreduce(const float* __restrict__ ws, float* __restrict__ gw, const long long n, const int taps,
                 const int parts, const float inv_h) {
  const long long i = (long long)SC_BID_X * 256 + SC_TID;
  if (i >= n) return;
  const int t = (int)(i % taps), centre = taps / 2;
  if (t == centre) {
    gw[i] = 0.f;
    return;
  }
  float gt = 0.f, gc = 0.f;
  for (int p = 0; p < parts; ++p) {
    gt += ws[p * n + i];
    gc += ws[p * n + i - t + centre];
  }
  gw[i] = (gt - gc) * inv_h;
}

// ------------------------------------------------------------------------------------------------- replicate / reflect
// gx[l, p] = sum of gpad[l, q] over the padded coordinates q (extents d + 2 r, origin -r) that the padding maps to p,
// per axis the low pad, the point itself, the high pad, in that order.  One thread per input point.
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_fdconv_unpad(const float* __restrict__ gpad, float* __restrict__ gx, const FdGeom g, const long long lines) {
  const long long img = (long long)g.d0 * g.d1 * g.d2;
  const long long i = (long long)SC_BID_X * 256 + SC_TID;
  if (i >= lines * img) return;
  long long q = i;
  const int p2 = (int)(q % g.d2);
  q /= g.d2;
  const int p1 = (int)(q % g.d1);
  q /= g.d1;
  const int p0 = (int)(q % g.d0);
  const long long line = q / g.d0;
  const int P0 = g.d0 + 2 * g.r0, P1 = g.d1 + 2 * g.r1, P2 = g.d2 + 2 * g.r2;
  const float* src = gpad + line * P0 * P1 * P2;
  float s = 0.f;
  for (int j0 = 0; j0 <= 2 * g.r0; ++j0) {
    const int q0 = j0 < g.r0 ? j0 : (j0 == g.r0 ? p0 + g.r0 : g.d0 + j0 - 1);
    if (fd_map(q0 - g.r0, g.d0, g.mode) != p0) continue;
    for (int j1 = 0; j1 <= 2 * g.r1; ++j1) {
      const int q1 = j1 < g.r1 ? j1 : (j1 == g.r1 ? p1 + g.r1 : g.d1 + j1 - 1);
      if (fd_map(q1 - g.r1, g.d1, g.mode) != p1) continue;
      for (int j2 = 0; j2 <= 2 * g.r2; ++j2) {
        const int q2 = j2 < g.r2 ? j2 : (j2 == g.r2 ? p2 + g.r2 : g.d2 + j2 - 1);
        if (fd_map(q2 - g.r2, g.d2, g.mode) != p2) continue;
        s += src[((long long)q0 * P1 + q1) * P2 + q2];
      }
    }
  }
  gx[i] = s;
}
