// sc_kernels_bicubic.h -- the 2-D skip-path resample of the spatially decomposed layer on a ROW RANGE of a global grid.
//
// resample(x, 1.0, [2, 3], output_shape) of neuralop/layers/resample.py:49-52 is F.interpolate(mode="bicubic",
// align_corners=True).  Here one rank holds the global input rows [src_row0, src_row0 + rows_in) (its own shard plus
// the halo rows its output rows read) and produces the global output rows [out_row0, out_row0 + rows_out).  The index
// arithmetic is ATen's (UpSampleBicubic2d.cu): scale = (in - 1) / (out - 1) in fp32 (0 when out == 1, computed on the
// host and passed in), source index scale * dst, taps floor - 1 .. floor + 2 clamped to [0, in - 1] of the GLOBAL grid,
// cubic convolution with A = -0.75, the row pass of each tap row first and the column pass over the four results.
//
//   k_bicubic_rows_fwd  workgroup = (256 output columns, BICUBIC_TY output rows, one image).  A lane owns one output
//                       column: its four column taps and weights stay in registers; walking down the rows it keeps the
//                       row-interpolated values of four consecutive (unclamped) input rows in a register window and
//                       computes each input row's value once per tile.  Input rows are read once per tile (+ 3 halo
//                       rows; the column taps of neighbouring lanes meet in L1), output rows written once.
//   k_bicubic_rows_bwd  deterministic GATHER form of the adjoint (no atomics): workgroup = (256 input columns,
//                       BICUBIC_TR input rows, one image).  Per input row r the workgroup first forms the column-pass
//                       adjoint  t[x] = sum_y wy(y -> r) g[y][x]  for every output column x its input columns are
//                       read by (into LDS), then each lane sums  sum_x wx(x -> i) t[x]  for its input column i.  The
//                       output rows y that read row r are a contiguous range (the floor is monotone): r - 2 <= floor(
//                       scale y) <= r + 1, found by bisection; wy(y -> r) sums the taps that clamp onto r (borders).
//                       Fixed summation order: two runs give the same bits.
#pragma once
#include "sc_device.h"

#define BICUBIC_TY 32          // output rows per forward workgroup
#define BICUBIC_TR 8           // input rows per backward workgroup
#define BICUBIC_LDS_MAX 12288  // floats of column-pass adjoint one backward workgroup stages (48 KiB)

struct BicubicArgs {
  long long images;             // B * C
  int rows_in, w_in;            // the halo'd shard: rows_in global rows from src_row0, w_in columns
  int src_row0, h_in;           // h_in = global input rows
  int out_row0, rows_out;       // this call's output rows (global index of the first)
  int h_out, w_out;             // global output grid
  float sy, sx;                 // (in - 1) / (out - 1) per dim, fp32, 0 when out == 1
};

// cubic convolution coefficients of ATen's get_cubic_upsample_coefficients (A = -0.75)
SC_DEVICE void bicubic_coeffs(const float t, float c[4]) {
  const float A = -0.75f;
  const float x1 = t, x2 = 1.0f - t;
  c[0] = ((A * (x1 + 1.0f) - 5.0f * A) * (x1 + 1.0f) + 8.0f * A) * (x1 + 1.0f) - 4.0f * A;
  c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
  c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  c[3] = ((A * (x2 + 1.0f) - 5.0f * A) * (x2 + 1.0f) + 8.0f * A) * (x2 + 1.0f) - 4.0f * A;
}

// ATen's source coordinate: the ROUNDED fp32 product scale * dst, its floor f and t = real - f.  Kept out of FMA
// contraction: fused, t would be the exact residual of the unrounded product and differ from ATen's by up to
// ulp(real) / 2 (2e-5 relative error at 1024 <-> 2048)
SC_DEVICE float bicubic_real(const float scale, const int dst) {
#ifndef SC_EMU
#pragma clang fp contract(off)
#endif
  return scale * (float)dst;
}

SC_DEVICE float bicubic_t(const float real, const int f) {
#ifndef SC_EMU
#pragma clang fp contract(off)
#endif
  return real - (float)f;
}

SC_DEVICE int bicubic_floor(const float scale, const int dst) { return (int)floorf(bicubic_real(scale, dst)); }

SC_DEVICE int bicubic_clamp(const int v, const int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// summed weight with which destination dst reads source index src (taps that clamp onto src add up)
SC_DEVICE float bicubic_weight(const float scale, const int dst, const int src, const int n_src) {
  const float real = bicubic_real(scale, dst);
  const int f = (int)floorf(real);
  float c[4];
  bicubic_coeffs(bicubic_t(real, f), c);
  float w = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) w += bicubic_clamp(f - 1 + k, n_src) == src ? c[k] : 0.0f;
  return w;
}

// the destinations [lo, hi) in [d0, d1) whose taps read source index src: r - 2 <= floor(scale d) <= r + 1
SC_DEVICE void bicubic_readers(const float scale, const int src, const int d0, const int d1, int& lo, int& hi) {
  int a = d0, b = d1;                                   // first d with floor >= src - 2
  while (a < b) {
    const int m = (a + b) >> 1;
    if (bicubic_floor(scale, m) >= src - 2) b = m; else a = m + 1;
  }
  lo = a;
  b = d1;                                               // first d with floor > src + 1
  while (a < b) {
    const int m = (a + b) >> 1;
    if (bicubic_floor(scale, m) > src + 1) b = m; else a = m + 1;
  }
  hi = a;
}

// row pass of unclamped global input row j (the local row is clamped into the shard as well: never outside the buffer)
SC_DEVICE float bicubic_row(const float* xi, const BicubicArgs& g, const int j, const int ix[4], const float cx[4]) {
  const int lr = bicubic_clamp(bicubic_clamp(j, g.h_in) - g.src_row0, g.rows_in);
  const float* row = xi + (long long)lr * g.w_in;
  return row[ix[0]] * cx[0] + row[ix[1]] * cx[1] + row[ix[2]] * cx[2] + row[ix[3]] * cx[3];
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_bicubic_rows_fwd(const float* __restrict__ x, float* __restrict__ y, BicubicArgs g) {
  const int ox = SC_BID_X * 256 + SC_TID;
  const int y0 = SC_BID_Y * BICUBIC_TY;
  const long long img = SC_BID_Z;
  if (ox >= g.w_out) return;
  const float* xi = x + img * g.rows_in * (long long)g.w_in;
  float* yi = y + img * g.rows_out * (long long)g.w_out;
  const float rx = bicubic_real(g.sx, ox);
  const int fx = (int)floorf(rx);
  float cx[4];
  bicubic_coeffs(bicubic_t(rx, fx), cx);
  int ix[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ix[k] = bicubic_clamp(fx - 1 + k, g.w_in);
  const int y1 = y0 + BICUBIC_TY < g.rows_out ? y0 + BICUBIC_TY : g.rows_out;
  int wb = 0;                                           // unclamped input row of h0
  float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, h3 = 0.0f;
  bool have = false;
  for (int oy = y0; oy < y1; ++oy) {
    const float ry = bicubic_real(g.sy, g.out_row0 + oy);
    const int fy = (int)floorf(ry);
    if (!have || fy - 1 - wb >= 4) {
      wb = fy - 1;
      h0 = bicubic_row(xi, g, wb, ix, cx);
      h1 = bicubic_row(xi, g, wb + 1, ix, cx);
      h2 = bicubic_row(xi, g, wb + 2, ix, cx);
      h3 = bicubic_row(xi, g, wb + 3, ix, cx);
      have = true;
    } else {
      while (wb < fy - 1) {
        h0 = h1;
        h1 = h2;
        h2 = h3;
        h3 = bicubic_row(xi, g, wb + 4, ix, cx);
        ++wb;
      }
    }
    float cy[4];
    bicubic_coeffs(bicubic_t(ry, fy), cy);
    yi[(long long)oy * g.w_out + ox] = h0 * cy[0] + h1 * cy[1] + h2 * cy[2] + h3 * cy[3];
  }
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_bicubic_rows_bwd(const float* __restrict__ gy, float* __restrict__ gx, BicubicArgs g) {
  SC_SHARED float t[BICUBIC_LDS_MAX];
  const int tid = SC_TID;
  const int c0 = SC_BID_X * 256;
  const int c1 = c0 + 256 < g.w_in ? c0 + 256 : g.w_in;
  const int r0 = SC_BID_Y * BICUBIC_TR;
  const int r1 = r0 + BICUBIC_TR < g.rows_in ? r0 + BICUBIC_TR : g.rows_in;
  const long long img = SC_BID_Z;
  const float* gyi = gy + img * g.rows_out * (long long)g.w_out;
  float* gxi = gx + img * g.rows_in * (long long)g.w_in;
  // output columns read by any input column of this block, and by this lane's column
  int xa, xb, xe, xf;
  bicubic_readers(g.sx, c0, 0, g.w_out, xa, xb);
  bicubic_readers(g.sx, c1 - 1, 0, g.w_out, xe, xf);
  const int xlo = xa, nx = (xf - xa) < BICUBIC_LDS_MAX ? (xf - xa) : BICUBIC_LDS_MAX;   // host guarantees the bound
  const int ci = c0 + tid;
  int ilo = 0, ihi = 0;
  if (ci < c1) bicubic_readers(g.sx, ci, 0, g.w_out, ilo, ihi);
  if (ilo < xlo) ilo = xlo;
  if (ihi > xlo + nx) ihi = xlo + nx;
  for (int lr = r0; lr < r1; ++lr) {
    const int r = g.src_row0 + lr;                      // global input row
    int ya, yb;
    bicubic_readers(g.sy, r, g.out_row0, g.out_row0 + g.rows_out, ya, yb);
    for (int j = tid; j < nx; j += 256) {
      const int ox = xlo + j;
      float s = 0.0f;
      for (int oy = ya; oy < yb; ++oy)
        s += bicubic_weight(g.sy, oy, r, g.h_in) * gyi[(long long)(oy - g.out_row0) * g.w_out + ox];
      t[j] = s;
    }
    SC_SYNC();
    if (ci < c1) {
      float s = 0.0f;
      for (int ox = ilo; ox < ihi; ++ox) s += bicubic_weight(g.sx, ox, ci, g.w_in) * t[ox - xlo];
      gxi[(long long)lr * g.w_in + ci] = s;
    }
    SC_SYNC();
  }
}
