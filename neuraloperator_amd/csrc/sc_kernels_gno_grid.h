// sc_kernels_gno_grid.h -- the fixed-radius search of the graph neural operator layer over a uniform cell grid: the
// second route beside k_radius (sc_kernels_gno.h), with the same bytes out.
//
//   k_grid_bounds / k_grid_params    min / max per axis over the finite data points (two-stage tree, no atomics); one
//                       thread then writes lo[3], inv_h[3], G[3] and the cell count into the workspace header -- the host
//                       learns none of it
//   k_grid_zero / k_grid_hist<D>     cell histogram (integer atomics)
//   k_grid_scan_sums / k_grid_scan   exclusive scan of the histogram over as many cells as the header holds: totals of
//                       4096-cell blocks, then every block adds the totals in front of it to its own scan
//   k_grid_scatter<D>   slot scatter into cell order: coordinates as structure of arrays plus the original index; the
//                       order inside a cell is whatever the atomics give, the row ordering below makes the result
//                       independent of it.  Points with a non-finite coordinate join no cell
//   k_grid_query<D, FILL>   16 lanes per query, 16 queries per workgroup: the 3^D cells around the query's cell (the
//                       cells along the last axis are contiguous in cell order: 3^(D-1) ranges).  Count pass: deg[m].
//                       Fill pass: a row of at most GNO_GRID_STAGE hits is staged in LDS, ranked (position = number of
//                       smaller indices) and written in ascending data index with its weights; a longer row is written
//                       unordered into the UPPER halves of its own int64 slots and listed for
//   k_grid_order_long<D>    one workgroup per listed row: ranks the upper halves into the lower halves, then widens
//                       every slot in place and writes the weights
//
// The hit test is gno_grid_d2<D>: dx * dx, then fmaf in dimension order, on the same fp32 inputs as k_radius -- d2 and
// the decision d2 <= r2 are bit-identical, and the weights are that expression evaluated again once the order is known.
// No float atomic, no register array indexed at run time.  Everything read from the workspace that becomes an address
// or a loop bound (grid sizes, cell starts, slots, point indices, listed rows) is clamped to its valid range first.
#pragma once
#include "sc_kernels_gno.h"

#define GNO_GRID_MARGIN 0.00390625      // 2^-8: cells are h = (r + 2^-62) (1 + 2^-8) wide or wider
#define GNO_GRID_SLACK 2.168404344971009e-19  // 2^-62: what fl(d^2) <= fl(r^2) can hide when squares underflow
#define GNO_GRID_CAP1 8192              // cells per axis at most, d = 1 / 2 / 3: at most 2^13, 2^20, 2^21 cells
#define GNO_GRID_CAP2 1024
#define GNO_GRID_CAP3 128
#define GNO_GRID_LANES 16               // lanes that share one query
#define GNO_GRID_QPB (256 / GNO_GRID_LANES)
#define GNO_GRID_STAGE 128              // hits of one row ordered on chip; longer rows take k_grid_order_long
#define GNO_GRID_RB 256                 // workgroups of the bounds reduction at most
#define GNO_GRID_SCAN_BLOCK (256 * GNO_SCAN_PT)  // cells per workgroup of the cell scan

struct GridHead {                       // first 64 bytes of the workspace, written by k_grid_params
  float lo[3], inv[3];
  int G[3];
  int ncell, nlong;                     // nlong: rows listed for k_grid_order_long (zeroed by the fill pass)
  int pad[5];
};

struct GridArgs {
  const float* data;                    // [n, D]
  const float* queries;                 // [m, D]
  long long n, m, E;
  float r2;
  double h;                             // least cell width
  int dim, cap, nb;                     // nb: workgroups of k_grid_bounds / k_grid_order_long
  int cells;                            // cells at most: what cnt and start hold (gno_grid_cells_max)
  GridHead* head;
  float* part;                          // [GNO_GRID_RB, 6]
  int* bsum;                            // [cells_max / GNO_GRID_SCAN_BLOCK]
  int* cnt;                             // [cells_max]
  int* start;                           // [cells_max + 1]
  float *sx, *sy, *sz;                  // [n] each: the points in cell order
  int* sidx;                            // [n]: their data index
  int* longrows;                        // [m]
  int* deg;                             // count pass: [m]
  const long long* splits;              // fill pass: [m + 1]
  long long* index;                     // fill pass: [E]
  float* weights;                       // fill pass, optional: [E]
};

SC_DEVICE bool gno_finite(const float x) { return fabsf(x) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

template <int D>
SC_DEVICE float gno_grid_d2(const float qx, const float qy, const float qz, const float px, const float py,
                            const float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  float d2 = dx * dx;                                        // fp32, in dimension order: k_radius's expression
  if (D > 1) d2 = fmaf(dy, dy, d2);
  if (D > 2) d2 = fmaf(dz, dz, d2);
  return d2;
}

// the cell of a coordinate along one axis, for data points and queries alike: every step is monotone in x.  tf: the
// floor before the clamp (a query whose tf lies two or more cells outside [0, G] has no neighbour)
SC_DEVICE int gno_grid_cell(const float x, const float lo, const float inv, const int G, float& tf) {
  tf = floorf((x - lo) * inv);
  return tf >= (float)(G - 1) ? G - 1 : (tf > 0.f ? (int)tf : 0);
}

struct GridDims {
  float lo0, lo1, lo2, inv0, inv1, inv2;
  int G0, G1, G2;
};
SC_DEVICE int gno_clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }
SC_DEVICE GridDims gno_grid_dims(const GridHead* h, const int cap) {
  GridDims g;
  g.lo0 = h->lo[0]; g.lo1 = h->lo[1]; g.lo2 = h->lo[2];
  g.inv0 = h->inv[0]; g.inv1 = h->inv[1]; g.inv2 = h->inv[2];
  g.G0 = gno_clampi(h->G[0], 1, cap);
  g.G1 = gno_clampi(h->G[1], 1, cap);
  g.G2 = gno_clampi(h->G[2], 1, cap);
  return g;
}
// cells the scan and the zero fill cover: the header's count, never more than the caps allow
SC_DEVICE int gno_grid_ncell(const GridArgs& a) {
  const GridDims g = gno_grid_dims(a.head, a.cap);
  const long long c = (long long)g.G0 * (a.dim > 1 ? g.G1 : 1) * (a.dim > 2 ? g.G2 : 1);
  return c > a.cells ? a.cells : (int)c;
}

// ----------------------------------------------------------------------------------------------- bounds and parameters
// S: [6][256] in LDS; on return S[j * 256] holds min (j < 3) / max (j >= 3) of the 256 entries of row j
SC_DEVICE void gno_grid_tree(float* S, const int t) {
  for (int o = 128; o > 0; o >>= 1) {
    SC_SYNC();
    if (t < o) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        S[j * 256 + t] = fminf(S[j * 256 + t], S[j * 256 + t + o]);
        S[(3 + j) * 256 + t] = fmaxf(S[(3 + j) * 256 + t], S[(3 + j) * 256 + t + o]);
      }
    }
  }
  SC_SYNC();
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_bounds(const GridArgs a) {
  SC_SHARED float S[6 * 256];
  const int t = SC_TID, D = a.dim;
  const float inf = __builtin_inff();
  float n0 = inf, n1 = inf, n2 = inf, x0 = -inf, x1 = -inf, x2 = -inf;
#pragma unroll 1
  for (long long i = (long long)SC_BID_X * 256 + t; i < a.n; i += (long long)a.nb * 256) {
    const float* p = a.data + i * D;
    const float px = p[0], py = D > 1 ? p[1] : 0.f, pz = D > 2 ? p[2] : 0.f;
    if (!(gno_finite(px) && gno_finite(py) && gno_finite(pz))) continue;    // such a point joins no cell
    n0 = fminf(n0, px); x0 = fmaxf(x0, px);
    n1 = fminf(n1, py); x1 = fmaxf(x1, py);
    n2 = fminf(n2, pz); x2 = fmaxf(x2, pz);
  }
  S[t] = n0; S[256 + t] = n1; S[512 + t] = n2;
  S[768 + t] = x0; S[1024 + t] = x1; S[1280 + t] = x2;
  gno_grid_tree(S, t);
  if (t < 6) a.part[SC_BID_X * 6 + t] = S[t * 256];
}

// ONE workgroup: the partial bounds of k_grid_bounds, then thread 0 writes the header.  Per axis, in double:
//   G = clamp(floor(extent / h) + 1, 1, cap), halved while the grid exceeds the descriptor's cell budget,
//   cell width w = max(h, extent / G),  inv = (float)(1 / w);
// an axis of zero extent, an axis past the dimension, a set without a finite point and an extent so wide that x - lo
// could overflow fp32 get G = 1 and inv = 0 (every finite point then lies in cell 0)
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_params(const GridArgs a) {
  SC_SHARED float S[6 * 256];
  const int t = SC_TID;
  const float inf = __builtin_inff();
  const bool in = t < a.nb && t < GNO_GRID_RB;
#pragma unroll
  for (int j = 0; j < 6; ++j) S[j * 256 + t] = in ? a.part[t * 6 + j] : (j < 3 ? inf : -inf);
  gno_grid_tree(S, t);
  if (t != 0) return;
  int G0 = 1, G1 = 1, G2 = 1;
  for (int k = 0; k < a.dim && k < 3; ++k) {
    const float lo = S[k * 256], hi = S[(3 + k) * 256];
    int G = 1;
    if (lo <= hi) {                                          // false without a finite point
      const double ext = (double)hi - (double)lo;
      if (ext > 0.0 && ext + a.h < 3.0e38) {
        const double g = floor(ext / a.h) + 1.0;
        G = g >= (double)a.cap ? a.cap : (int)g;
        if (G < 1) G = 1;
      }
    }
    if (k == 0) G0 = G;
    else if (k == 1) G1 = G;
    else G2 = G;
  }
  // the cell budget of this descriptor: halve the longest axis until the grid fits (wider cells stay correct)
  while ((long long)G0 * G1 * G2 > a.cells) {
    if (G0 >= G1 && G0 >= G2) G0 = (G0 + 1) / 2;
    else if (G1 >= G2) G1 = (G1 + 1) / 2;
    else G2 = (G2 + 1) / 2;
  }
  for (int k = 0; k < 3; ++k) {
    float lo = S[k * 256];
    const float hi = S[(3 + k) * 256];
    const int G = k == 0 ? G0 : (k == 1 ? G1 : G2);
    float inv = 0.f;
    if (!(lo <= hi)) lo = 0.f;
    if (G > 1) {
      const double wc = ((double)hi - (double)lo) / (double)G;
      inv = (float)(1.0 / (wc > a.h ? wc : a.h));
    }
    a.head->lo[k] = lo;
    a.head->inv[k] = inv;
    a.head->G[k] = G;
  }
  a.head->ncell = G0 * G1 * G2;
  a.head->nlong = 0;
}

// --------------------------------------------------------------------------------------------------------------- binning
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_zero(const GridArgs a) {
  const int ncell = gno_grid_ncell(a);
  const long long base = (long long)SC_BID_X * GNO_GRID_SCAN_BLOCK;
  for (int k = 0; k < GNO_SCAN_PT; ++k) {
    const long long i = base + k * 256 + SC_TID;
    if (i < ncell) a.cnt[i] = 0;
  }
}

// the cell of data point i, or -1 for a point with a non-finite coordinate
template <int D>
SC_DEVICE int gno_grid_point_cell(const GridArgs& a, const GridDims& g, const long long i, float& px, float& py,
                                  float& pz) {
  const float* p = a.data + i * D;
  px = p[0];
  py = D > 1 ? p[D > 1 ? 1 : 0] : 0.f;
  pz = D > 2 ? p[D > 2 ? 2 : 0] : 0.f;
  if (!(gno_finite(px) && gno_finite(py) && gno_finite(pz))) return -1;
  float tf;
  int c = gno_grid_cell(px, g.lo0, g.inv0, g.G0, tf);
  if (D > 1) c = c * g.G1 + gno_grid_cell(py, g.lo1, g.inv1, g.G1, tf);
  if (D > 2) c = c * g.G2 + gno_grid_cell(pz, g.lo2, g.inv2, g.G2, tf);
  return c < a.cells ? c : a.cells - 1;
}

template <int D>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_hist(const GridArgs a) {
  const long long i = (long long)SC_BID_X * 256 + SC_TID;
  if (i >= a.n) return;
  const GridDims g = gno_grid_dims(a.head, a.cap);
  float px, py, pz;
  const int c = gno_grid_point_cell<D>(a, g, i, px, py, pz);
  if (c >= 0) SC_ATOMIC_ADD_I32(a.cnt + c, 1);
}

// bsum[b] = cnt[b * 4096] + .. over the block's cells
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_scan_sums(const GridArgs a) {
  SC_SHARED int S[256];
  const int t = SC_TID, ncell = gno_grid_ncell(a);
  if ((long long)SC_BID_X * GNO_GRID_SCAN_BLOCK >= ncell) return;   // the whole workgroup: k_grid_scan skips it too
  const long long lo = (long long)SC_BID_X * GNO_GRID_SCAN_BLOCK + (long long)t * GNO_SCAN_PT;
  int s = 0;
  for (int k = 0; k < GNO_SCAN_PT; ++k)
    if (lo + k < ncell) s += a.cnt[lo + k];
  S[t] = s;
  for (int o = 128; o > 0; o >>= 1) {
    SC_SYNC();
    if (t < o) S[t] += S[t + o];
  }
  SC_SYNC();
  if (t == 0) a.bsum[SC_BID_X] = S[0];
}

// start[i] = cnt[0] + .. + cnt[i - 1], i = 0 .. ncell: every workgroup adds the totals of the blocks in front of it
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_scan(const GridArgs a) {
  SC_SHARED int S[256];
  const int t = SC_TID, ncell = gno_grid_ncell(a), b = SC_BID_X;
  if ((long long)b * GNO_GRID_SCAN_BLOCK >= ncell) return;   // the whole workgroup
  int off = 0;
  for (int j = t; j < b; j += 256) off += a.bsum[j];
  S[t] = off;
  for (int o = 128; o > 0; o >>= 1) {
    SC_SYNC();
    if (t < o) S[t] += S[t + o];
  }
  SC_SYNC();
  off = S[0];
  const long long lo = (long long)b * GNO_GRID_SCAN_BLOCK + (long long)t * GNO_SCAN_PT;
  int s = 0;
  for (int k = 0; k < GNO_SCAN_PT; ++k)
    if (lo + k < ncell) s += a.cnt[lo + k];
  SC_SYNC();                                                 // S[0] has been read
  S[t] = s;
  for (int o = 1; o < 256; o <<= 1) {
    SC_SYNC();
    const int v = t >= o ? S[t - o] : 0;
    SC_SYNC();
    S[t] += v;
  }
  int run = off + S[t] - s;
  for (int k = 0; k < GNO_SCAN_PT; ++k)
    if (lo + k < ncell) {
      a.start[lo + k] = run;
      run += a.cnt[lo + k];
      if (lo + k == ncell - 1) a.start[ncell] = run;
    }
}

// the counters run back down to zero: the point that finds `old` in its cell's counter takes slot start + old - 1
template <int D>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_scatter(const GridArgs a) {
  const long long i = (long long)SC_BID_X * 256 + SC_TID;
  if (i >= a.n) return;
  const GridDims g = gno_grid_dims(a.head, a.cap);
  float px, py, pz;
  const int c = gno_grid_point_cell<D>(a, g, i, px, py, pz);
  if (c < 0) return;
  const long long o = (long long)a.start[c] + SC_ATOMIC_ADD_I32(a.cnt + c, -1) - 1;
  if (o < 0 || o >= a.n) return;
  a.sx[o] = px;
  if (D > 1) a.sy[o] = py;
  if (D > 2) a.sz[o] = pz;
  a.sidx[o] = (int)i;
}

// -------------------------------------------------------------------------------------------------------- count and fill
template <int D, bool FILL>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_query(const GridArgs a) {
  SC_SHARED int C[256];                                      // count pass: hits per lane; fill pass: C[g] = hits so far
  SC_SHARED int S[FILL ? GNO_GRID_QPB * GNO_GRID_STAGE : 1];
  const int grp = SC_TID / GNO_GRID_LANES, gl = SC_TID % GNO_GRID_LANES;
  const long long q = (long long)SC_BID_X * GNO_GRID_QPB + grp;
  const bool inq = q < a.m;
  const float* qp = a.queries + (inq ? q : 0) * D;
  const float qx = inq ? qp[0] : 0.f;
  const float qy = inq && D > 1 ? qp[D > 1 ? 1 : 0] : 0.f;
  const float qz = inq && D > 2 ? qp[D > 2 ? 2 : 0] : 0.f;
  const GridDims g = gno_grid_dims(a.head, a.cap);
  const int n = (int)a.n;
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
  const int c0 = gno_grid_cell(qx, g.lo0, g.inv0, g.G0, t0);
  const int c1 = D > 1 ? gno_grid_cell(qy, g.lo1, g.inv1, g.G1, t1) : 0;
  const int c2 = D > 2 ? gno_grid_cell(qz, g.lo2, g.inv2, g.G2, t2) : 0;
  // a query with a non-finite coordinate has no neighbour; nor has one whose cell before the clamp lies two or more
  // outside [0, G] on some axis (data cells before the clamp lie in [0, G], a kept pair differs by at most 1)
  bool walk = inq && gno_finite(qx) && gno_finite(qy) && gno_finite(qz);
  walk = walk && !(t0 < -1.5f || t0 > (float)g.G0 + 1.5f);
  if (D > 1) walk = walk && !(t1 < -1.5f || t1 > (float)g.G1 + 1.5f);
  if (D > 2) walk = walk && !(t2 < -1.5f || t2 > (float)g.G2 + 1.5f);
  long long lo = 0, hi = 0;
  if (FILL && inq) gno_segment(a.splits, q, a.E, lo, hi);
  const long long len = hi - lo;
  const bool staged = len <= GNO_GRID_STAGE;
  int* ihalf = (int*)a.index;                                // the row's int64 slots as pairs of int32 (little endian)
  int hits = 0;
  if (FILL) {
    if (gl == 0) C[grp] = 0;
    SC_SYNC();
  }
  if (walk) {
    const int x0 = c0 > 0 ? c0 - 1 : 0, x1 = c0 + 1 < g.G0 ? c0 + 1 : g.G0 - 1;
    const int y0 = c1 > 0 ? c1 - 1 : 0, y1 = c1 + 1 < g.G1 ? c1 + 1 : g.G1 - 1;
    const int z0 = c2 > 0 ? c2 - 1 : 0, z1 = c2 + 1 < g.G2 ? c2 + 1 : g.G2 - 1;
    // the last axis runs fastest in cell order: its up to three cells are one range of the sorted points
    const int u0 = D == 1 ? 0 : x0, u1 = D == 1 ? 0 : x1;
    const int v0 = D == 3 ? y0 : 0, v1 = D == 3 ? y1 : 0;
    const int w0 = D == 1 ? x0 : (D == 2 ? y0 : z0), w1 = D == 1 ? x1 : (D == 2 ? y1 : z1);
    const int GW = D == 1 ? g.G0 : (D == 2 ? g.G1 : g.G2);
#pragma unroll 1
    for (int u = u0; u <= u1; ++u) {
#pragma unroll 1
      for (int v = v0; v <= v1; ++v) {
        const int row = D == 1 ? 0 : (D == 2 ? u : u * g.G1 + v);
        int s = a.start[gno_clampi(row * GW + w0, 0, a.cells)];
        int e = a.start[gno_clampi(row * GW + w1 + 1, 0, a.cells)];
        s = gno_clampi(s, 0, n);
        e = gno_clampi(e, s, n);
#pragma unroll 1
        for (int i = s + gl; i < e; i += GNO_GRID_LANES) {
          const float d2 = gno_grid_d2<D>(qx, qy, qz, a.sx[i], D > 1 ? a.sy[i] : 0.f, D > 2 ? a.sz[i] : 0.f);
          if (!(d2 <= a.r2)) continue;
          if (!FILL) {
            ++hits;
            continue;
          }
          const int j = a.sidx[i];
          if (j < 0 || j >= n) continue;
          const int pos = SC_ATOMIC_ADD_I32(&C[grp], 1);     // any order: the ranking below fixes it
          if (pos >= len) continue;
          if (staged) S[grp * GNO_GRID_STAGE + pos] = j;
          else ihalf[2 * (lo + pos) + 1] = j;
        }
      }
    }
  }
  if (!FILL) {
    C[SC_TID] = hits;
    SC_SYNC();
    if (gl == 0 && inq) {
      int s = 0;
      for (int k = 0; k < GNO_GRID_LANES; ++k) s += C[grp * GNO_GRID_LANES + k];
      a.deg[q] = s;
    }
    return;
  }
  SC_SYNC();
  if (len <= 0) return;
  if (!staged) {
    if (gl == 0) {
      const int p = SC_ATOMIC_ADD_I32(&a.head->nlong, 1);
      if (p >= 0 && p < a.m) a.longrows[p] = (int)q;
    }
    return;
  }
  const int* row = S + grp * GNO_GRID_STAGE;
  for (int k = gl; k < (int)len; k += GNO_GRID_LANES) {
    const int j = row[k];
    int rank = 0;
    for (int t = 0; t < (int)len; ++t) rank += row[t] < j ? 1 : 0;
    a.index[lo + rank] = j;
    if (a.weights) {
      float d2 = 0.f;
      if (j >= 0 && j < n) {
        const float* p = a.data + (long long)j * D;
        d2 = gno_grid_d2<D>(qx, qy, qz, p[0], D > 1 ? p[D > 1 ? 1 : 0] : 0.f, D > 2 ? p[D > 2 ? 2 : 0] : 0.f);
      }
      a.weights[lo + rank] = d2 == 0.f ? GNO_ZERO_D2 : d2;
    }
  }
}

// rows longer than GNO_GRID_STAGE: phase A ranks the unordered indices (upper halves of the row's int64 slots) into
// the lower halves, phase B widens every slot in place (each thread reads and writes its own slots only)
template <int D>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_grid_order_long(const GridArgs a) {
  const int t = SC_TID;
  int nlong = a.head->nlong;
  nlong = nlong < 0 ? 0 : (nlong > a.m ? (int)a.m : nlong);
  int* ihalf = (int*)a.index;
#pragma unroll 1
  for (int r = SC_BID_X; r < nlong; r += a.nb) {             // uniform over the workgroup
    const long long q = a.longrows[r];
    long long lo = 0, hi = 0;
    if (q >= 0 && q < a.m) gno_segment(a.splits, q, a.E, lo, hi);
    const long long len = hi - lo;
    int* row = ihalf + 2 * lo;
#pragma unroll 1
    for (long long k = t; k < len; k += 256) {
      const int j = row[2 * k + 1];
      long long rank = 0;
      for (long long s = 0; s < len; ++s) rank += row[2 * s + 1] < j ? 1 : 0;
      row[2 * rank] = j;
    }
    SC_SYNC();
    const float* qp = a.queries + (q >= 0 && q < a.m ? q : 0) * D;
    const float qx = qp[0], qy = D > 1 ? qp[D > 1 ? 1 : 0] : 0.f, qz = D > 2 ? qp[D > 2 ? 2 : 0] : 0.f;
#pragma unroll 1
    for (long long k = t; k < len; k += 256) {
      const int j = row[2 * k];
      row[2 * k + 1] = j < 0 ? -1 : 0;
      if (a.weights) {
        float d2 = 0.f;
        if (j >= 0 && j < a.n) {
          const float* p = a.data + (long long)j * D;
          d2 = gno_grid_d2<D>(qx, qy, qz, p[0], D > 1 ? p[D > 1 ? 1 : 0] : 0.f, D > 2 ? p[D > 2 ? 2 : 0] : 0.f);
        }
        a.weights[lo + k] = d2 == 0.f ? GNO_ZERO_D2 : d2;
      }
    }
    SC_SYNC();
  }
}
