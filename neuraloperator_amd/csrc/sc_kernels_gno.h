// sc_kernels_gno.h -- the graph neural operator layer (neuralop/layers/neighbor_search.py:84-119 native_neighbor_search,
// segment_csr.py:8-98, integral_transform.py:155-227, gno_block.py:237-250).
//
//   k_radius<D, FILL>   fixed-radius search by brute force over LDS tiles of the data points: count pass (deg[m]) and fill
//                       pass (neighbors_index, squared distances), each query's neighbours in ascending data index
//   k_scan_i32          exclusive scan int32[count] -> int64[count + 1] (row splits / column splits), one workgroup
//   k_csr_hist / k_csr_slot / k_csr_sortcols     CSR transpose: column histogram + row of every edge, slot fill, and one
//                       wave per column that ranks its slice, so the result does not depend on the order of the atomics
//   k_csr_reduce        out[b, i, c] = s_i sum_{k in [rs[i], rs[i+1])} K[(b,) e, c] F[b, gather(e), c] w[e] scale(e),
//                       e = perm[k] or k: the fused kernel integral, and with perm / row_of_edge its transposed form
//   k_csr_edge_grad     gK[(b,) e, c] = s_i w[e] (sum_b) g[b, i, c] F[b, idx[e], c]
//   k_edge_lift<BWD>    H[(b,) e, c] = act(Py[(b,) idx[e], c] + Px[row(e), c] + bias[c]) and gPre = gH act'(pre)
//
// The CSR kernels share one mapping: a workgroup of 4 waves, ONE WAVE PER ROW (times batch); lanes run along the
// contiguous channel axis.  With c < 64 channels the wave is cut into 64 / cp2 groups of cp2 lanes (cp2 = c rounded up
// to a power of two): group s walks edges lo + s, lo + s + groups, .. and the groups' partial sums are added in group
// order through LDS.  With c > 64 the wave walks its segment once per 64 channels.  A row however long is walked by its
// one wave in order -- nothing is split across workgroups, there is no second pass and no float atomic: two launches give
// the same bits.  Integer atomics appear only in the transpose (histogram, slot counters), whose output is made
// order-independent by the ranking pass.  Every index read from a caller's array (neighbour index, perm, row of edge,
// splits) is range-checked before it addresses memory: IntegralTransform accepts user-built neighbour dicts.
// No register array is indexed at run time (no scratch memory).
#pragma once
#include "sc_device.h"

#define GNO_TILE 1024          // data points per LDS tile (structure of arrays: 3 x 4 KiB)
#define GNO_QPW 8              // queries a wave carries through one pass over the tiles
#define GNO_QPB (4 * GNO_QPW)  // queries per workgroup
#define GNO_SCAN_PT 16         // consecutive items per thread of the scan
#define GNO_ZERO_D2 1e-14f     // squared eps of the reference's zero-distance replacement (neighbor_search.py:105-111)

struct RadiusArgs {
  const float* data;           // [n, D]
  const float* queries;        // [m, D]
  long long n, m, E;           // E: length of index / weights (fill pass)
  float r2;
  int* deg;                    // count pass: [m]
  const long long* splits;     // fill pass: [m + 1]
  long long* index;            // fill pass: [E]
  float* weights;              // fill pass, optional: [E]
};

template <int D, bool FILL>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_radius(const RadiusArgs a) {
  SC_SHARED float L[3 * GNO_TILE];
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const long long q0 = (long long)SC_BID_X * GNO_QPB + wave * GNO_QPW;
  float qx[GNO_QPW], qy[GNO_QPW], qz[GNO_QPW];
  long long pos[GNO_QPW];
#pragma unroll
  for (int j = 0; j < GNO_QPW; ++j) {
    const bool ok = q0 + j < a.m;
    const float* q = a.queries + (ok ? q0 + j : 0) * D;
    qx[j] = ok ? q[0] : 0.f;
    qy[j] = ok && D > 1 ? q[D > 1 ? 1 : 0] : 0.f;
    qz[j] = ok && D > 2 ? q[D > 2 ? 2 : 0] : 0.f;
    pos[j] = FILL && ok ? a.splits[q0 + j] : 0;
  }
#pragma unroll 1
  for (long long t0 = 0; t0 < a.n; t0 += GNO_TILE) {
    SC_SYNC();                                               // the previous tile has been read
    for (int i = SC_TID; i < GNO_TILE; i += 256) {
      const bool ok = t0 + i < a.n;
      const float* p = a.data + (ok ? t0 + i : 0) * D;
      L[i] = ok ? p[0] : 0.f;
      if (D > 1) L[GNO_TILE + i] = ok ? p[D > 1 ? 1 : 0] : 0.f;
      if (D > 2) L[2 * GNO_TILE + i] = ok ? p[D > 2 ? 2 : 0] : 0.f;
    }
    SC_SYNC();
    const int tn = a.n - t0 < GNO_TILE ? (int)(a.n - t0) : GNO_TILE;
#pragma unroll 1
    for (int ch = 0; ch < tn; ch += 64) {
      const int i = ch + lane;
      const bool in = i < tn;
      const float px = L[i], py = D > 1 ? L[GNO_TILE + i] : 0.f, pz = D > 2 ? L[2 * GNO_TILE + i] : 0.f;
#pragma unroll
      for (int j = 0; j < GNO_QPW; ++j) {
        if (q0 + j >= a.m) continue;                         // wave-uniform
        const float dx = qx[j] - px, dy = qy[j] - py, dz = qz[j] - pz;
        float d2 = dx * dx;                                  // fp32, in dimension order
        if (D > 1) d2 = fmaf(dy, dy, d2);
        if (D > 2) d2 = fmaf(dz, dz, d2);
        const bool hit = in && d2 <= a.r2;
        const unsigned long long mk = sc_ballot(hit);
        if (FILL && hit) {                                   // ascending data index: tiles, chunks and lanes in order
          const long long o = pos[j] + sc_popc64(mk & ((1ull << lane) - 1ull));
          if (o >= 0 && o < a.E) {
            a.index[o] = t0 + i;
            if (a.weights) a.weights[o] = d2 == 0.f ? GNO_ZERO_D2 : d2;
          }
        }
        pos[j] += sc_popc64(mk);
      }
    }
  }
  if (!FILL && lane == 0) {
#pragma unroll
    for (int j = 0; j < GNO_QPW; ++j)
      if (q0 + j < a.m) a.deg[q0 + j] = (int)pos[j];
  }
}

// out[i] = in[0] + .. + in[i - 1], i = 0 .. count (out[count] = the total); ONE workgroup
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_scan_i32(const int* __restrict__ in, long long* __restrict__ out,
                                                const long long count) {
  SC_SHARED long long S[256];
  const int t = SC_TID;
  long long carry = 0;
#pragma unroll 1
  for (long long base = 0; base < count; base += 256 * GNO_SCAN_PT) {
    const long long lo = base + (long long)t * GNO_SCAN_PT;
    long long s = 0;
    for (int k = 0; k < GNO_SCAN_PT; ++k)
      if (lo + k < count) s += in[lo + k];
    SC_SYNC();                                               // S of the previous pass has been read
    S[t] = s;
    for (int o = 1; o < 256; o <<= 1) {
      SC_SYNC();
      const long long v = t >= o ? S[t - o] : 0;
      SC_SYNC();
      S[t] += v;
    }
    SC_SYNC();
    long long run = carry + S[t] - s;
    for (int k = 0; k < GNO_SCAN_PT; ++k)
      if (lo + k < count) {
        out[lo + k] = run;
        run += in[lo + k];
      }
    carry += S[255];
  }
  if (t == 0) out[count] = carry;
}

// ------------------------------------------------------------------------------------------------------ CSR transpose
// p[0 .. count) = v: the counters and the perm fill of the transpose are plain launches, not memset operations, so that a
// backward pass recorded into a graph replays them like every other kernel of the step
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_fill_i32(int* __restrict__ p, const long long count, const int v) {
  const long long i = (long long)SC_BID_X * 256 + SC_TID;
  if (i < count) p[i] = v;
}

struct CsrTArgs {
  const long long* splits;     // [rows + 1]
  const long long* index;      // [E]
  long long rows, cols, E;
  int* cnt;                    // [cols]: histogram, then slot counters
  const long long* col_splits; // [cols + 1]
  int* tmp;                    // [E]: edge ids grouped by column, any order
  int* perm;                   // [E]: the same, ascending within each column
  int* row_of_edge;            // [E]
};

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_csr_hist(const CsrTArgs a) {
  const long long e = (long long)SC_BID_X * 256 + SC_TID;
  if (e >= a.E) return;
  long long lo = 0, hi = a.rows;                             // the last row whose split is <= e
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (a.splits[mid] <= e) lo = mid;
    else hi = mid;
  }
  a.row_of_edge[e] = (int)lo;
  const long long j = a.index[e];
  if (j >= 0 && j < a.cols) SC_ATOMIC_ADD_I32(a.cnt + j, 1);
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_csr_slot(const CsrTArgs a) {
  const long long e = (long long)SC_BID_X * 256 + SC_TID;
  if (e >= a.E) return;
  const long long j = a.index[e];
  if (j < 0 || j >= a.cols) return;
  const long long o = a.col_splits[j] + SC_ATOMIC_ADD_I32(a.cnt + j, 1);
  if (o >= 0 && o < a.E) a.tmp[o] = (int)e;
}

// one wave per column: perm[lo + rank of v among the column's edge ids] = v (the ids are distinct)
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_csr_sortcols(const CsrTArgs a) {
  const int lane = SC_TID & 63;
  const long long j = (long long)SC_BID_X * 4 + (SC_TID >> 6);
  if (j >= a.cols) return;
  const long long lo = a.col_splits[j], hi = a.col_splits[j + 1];
  if (lo < 0 || hi > a.E) return;
  const int* s = a.tmp + lo;
  const long long len = hi - lo;
  for (long long k = lane; k < len; k += 64) {
    const int v = s[k];
    long long rank = 0;
    for (long long t = 0; t < len; ++t) rank += s[t] < v ? 1 : 0;
    a.perm[lo + rank] = v;
  }
}

// --------------------------------------------------------------------------------- reduce, edge gradient, first layer
struct CsrArgs {
  const long long* splits;     // [rows + 1]: the segments this launch walks
  const int* perm;             // optional [E]: position k of a segment holds edge perm[k]
  const long long* g64;        // optional [E]: row of F that edge e reads (a neighbour index) ...
  const int* g32;              // ... or the same as int32 (row_of_edge); neither: e itself
  const long long* ssplits;    // optional [nS + 1]: edge e is scaled by 1 / (ssplits[r + 1] - ssplits[r]), r = g32[e]
  const float* K;              // [(b,) E, c]
  const float* F;              // optional [b, nF, c]; edge_grad: may be null
  const float* w;              // optional [E]
  const float* g;              // edge_grad: [b, rows, c]
  float* out;                  // reduce: [b, rows, c]; edge_grad: gK [(b,) E, c]
  long long rows, E, nF, nS;
  long long K_bs, F_bs;        // batch strides in floats, 0 = shared by the batch
  int c, cp2, batch, mean;
};

SC_DEVICE long long gno_row_of(const CsrArgs& a, const long long e) {
  return a.g64 ? a.g64[e] : (a.g32 ? (long long)a.g32[e] : e);
}
SC_DEVICE void gno_segment(const long long* splits, const long long i, const long long E, long long& lo, long long& hi) {
  lo = splits[i];
  hi = splits[i + 1];
  lo = lo < 0 ? 0 : (lo > E ? E : lo);
  hi = hi < lo ? lo : (hi > E ? E : hi);
}

SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_csr_reduce(const CsrArgs a) {
  SC_SHARED float red[256];
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const long long item = (long long)SC_BID_X * 4 + wave;
  if (item >= a.rows * a.batch) return;                      // wave-uniform
  const long long b = item / a.rows, i = item - b * a.rows;
  long long lo, hi;
  gno_segment(a.splits, i, a.E, lo, hi);
  const int groups = 64 / a.cp2, sub = lane / a.cp2, ci = lane - sub * a.cp2;
  const float* Kb = a.K + b * a.K_bs;
  const float* Fb = a.F ? a.F + b * a.F_bs : nullptr;
#pragma unroll 1
  for (int c0 = 0; c0 < a.c; c0 += 64) {
    const int cc = c0 + ci;
    const bool ok = cc < a.c;
    float acc = 0.f;
#pragma unroll 1
    for (long long k = lo + sub; k < hi; k += groups) {
      const long long e = a.perm ? (long long)a.perm[k] : k;
      if (e < 0 || e >= a.E || !ok) continue;
      float v = Kb[e * a.c + cc];
      if (Fb) {
        const long long r = gno_row_of(a, e);
        v = r >= 0 && r < a.nF ? v * Fb[r * a.c + cc] : 0.f;
      }
      if (a.w) v *= a.w[e];
      if (a.ssplits) {
        const long long r = a.g32[e];
        const long long d = r >= 0 && r < a.nS ? a.ssplits[r + 1] - a.ssplits[r] : 0;
        v = d > 0 ? v / (float)d : 0.f;
      }
      acc += v;
    }
    if (groups > 1) {                                        // the groups' sums in group order
      red[SC_TID] = acc;
      SC_WAVE_SYNC();
      if (sub == 0) {
        acc = red[wave * 64 + ci];
        for (int s = 1; s < groups; ++s) acc += red[wave * 64 + s * a.cp2 + ci];
      }
      SC_WAVE_SYNC();
    }
    if (sub == 0 && ok) a.out[item * a.c + cc] = a.mean ? (hi > lo ? acc / (float)(hi - lo) : 0.f) : acc;
  }
}

// one wave per ROW (not per batch entry): with K shared by the batch the sum over b stays inside the lane
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_csr_edge_grad(const CsrArgs a) {
  const int lane = SC_TID & 63;
  const long long i = (long long)SC_BID_X * 4 + (SC_TID >> 6);
  if (i >= a.rows) return;
  long long lo, hi;
  gno_segment(a.splits, i, a.E, lo, hi);
  const int groups = 64 / a.cp2, sub = lane / a.cp2, ci = lane - sub * a.cp2;
  const float s = a.mean && hi > lo ? 1.f / (float)(hi - lo) : 1.f;
#pragma unroll 1
  for (int c0 = 0; c0 < a.c; c0 += 64) {
    const int cc = c0 + ci;
    if (cc >= a.c) continue;
#pragma unroll 1
    for (long long e = lo + sub; e < hi; e += groups) {
      const long long r = gno_row_of(a, e);
      const bool rok = !a.F || (r >= 0 && r < a.nF);
      const float sw = a.w ? s * a.w[e] : s;
      float sum = 0.f;
      for (int b = 0; b < a.batch; ++b) {
        float v = a.g[(b * a.rows + i) * a.c + cc];
        if (a.F) v = rok ? v * a.F[b * a.F_bs + r * a.c + cc] : 0.f;
        if (a.K_bs) a.out[b * a.K_bs + e * a.c + cc] = sw * v;
        else sum += v;
      }
      if (!a.K_bs) a.out[e * a.c + cc] = sw * sum;
    }
  }
}

struct LiftArgs {
  const long long* splits;     // [rows + 1]
  const long long* index;      // [E]
  const float* Py;             // [(b,) nPy, c]
  const float* Px;             // [rows, c]
  const float* bias;           // optional [c]
  const float* gH;             // backward: [(b,) E, c]
  float* out;                  // H or gPre: [(b,) E, c]
  long long rows, E, nPy, Py_bs;
  int c, cp2, batch, gelu;
};

template <bool BWD>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_edge_lift(const LiftArgs a) {
  const int lane = SC_TID & 63;
  const long long i = (long long)SC_BID_X * 4 + (SC_TID >> 6);
  if (i >= a.rows) return;
  long long lo, hi;
  gno_segment(a.splits, i, a.E, lo, hi);
  const int groups = 64 / a.cp2, sub = lane / a.cp2, ci = lane - sub * a.cp2;
#pragma unroll 1
  for (int c0 = 0; c0 < a.c; c0 += 64) {
    const int cc = c0 + ci;
    if (cc >= a.c) continue;
    const float base = a.Px[i * a.c + cc] + (a.bias ? a.bias[cc] : 0.f);
#pragma unroll 1
    for (long long e = lo + sub; e < hi; e += groups) {
      const long long j = a.index[e];
      const bool jok = j >= 0 && j < a.nPy;
      for (int b = 0; b < a.batch; ++b) {
        const long long o = (b * a.E + e) * a.c + cc;
        float r = 0.f;
        if (jok) {
          const float pre = a.Py[b * a.Py_bs + j * a.c + cc] + base;
          if (BWD) {
            float gl = 1.f, gr = 1.f;
            if (a.gelu) sc_gelu_both(pre, gl, gr);
            r = a.gH[o] * gr;
          } else {
            r = a.gelu ? sc_gelu(pre) : pre;
          }
        }
        a.out[o] = r;
      }
    }
  }
}
