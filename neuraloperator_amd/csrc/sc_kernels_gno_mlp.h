// sc_kernels_gno_mlp.h -- the kernel MLP of the graph neural operator layer over CHUNKS of edges (the fused route of
// IntegralTransform; the network is LinearChannelMLP with GELU, channel_mlp.py, applied to the edge features of
// integral_transform.py:158-191).  Layer 0 stays split by points (Py, Px, bias0: sc_kernels_gno.h k_edge_lift); layers
// 1 .. L-1 are W_l [c_{l+1} x c_l] with b_l, GELU after every layer but the last.  A chunk holds S edges (S a multiple
// of EMLP_ROWS) times the batch: row = b S + (e - e0), so a tile of EMLP_ROWS rows lies inside one batch entry.
//
//   k_emlp_gemm<NOB>   C = epi(A B + bias) on v_mfma_f32_32x32x2_f32 (exact fp32, k ascending), 128 rows per workgroup,
//                      32 per wave, 32 NOB columns, both operands through LDS (A's row stride 33), after
//                      k_dsp_gemm_mfma.  A is a buffer, or -- the first GEMM of the forward chain -- formed in the load
//                      path: gelu(Py[(b,) idx[e]] + (Px[row(e)] + bias0)), row(e) by one binary search in splits per row
//                      of the tile; an idx[e] outside [0, n_py) gives a zero row, as in k_edge_lift.  B is W^T (forward:
//                      B[k][j] = W[j][k]) or W (data gradient).  Epilogues: + bias; gelu(+ bias), optionally keeping the
//                      pre-activation; times gelu'(z) of a stored pre-activation (in place over z: an element is read
//                      and written by the same lane).  Any widths: operands are zero-padded while staged, stores guarded.
//   k_emlp_lift        backward only: z_0 and h_0 = gelu(z_0) of the chunk (the forward chain never stores either)
//   k_emlp_wgrad<NOB>  parts[s][o][i] = sum_{rows of slice s} delta[row][o] h[row][i] and parts_b[s][o], a wave per
//                      (slice, 32 o, 32 NOB i) walking its rows two at a time, after k_dsp_wgrad_mfma
//   k_emlp_wreduce     gW += sum_s parts[s], gb += sum_s parts_b[s], slices ascending: chunks accumulate in chunk order
//   k_emlp_rows        gPx[row] += sum of delta_0 over the row's edges inside the window [e0, e1), batch summed in the lane
//   k_emlp_cols        gPy[(b,) col] += sum of delta_0 over the column's edges inside the window: perm is ascending inside
//                      a column, so they are one sub-range of its slice; the wave of the column's FIRST edge in the
//                      window (one binary search) sums it, the waves of its other edges leave
//
// No float atomics; a row of gPx / gPy / gW is added to by one wave per launch and launches are stream ordered, so two
// calls give the same bits.  Every index read from a caller's array (splits, index, col_splits, perm) is range-checked
// before it addresses memory.  No register array is indexed at run time (no scratch memory).
#pragma once
#include "sc_device.h"
#include "sc_kernels_mfma.h"
#include "sc_kernels_gno.h"

#define EMLP_ROWS 128          // rows per workgroup of the GEMM (32 to a wave): the row tile
#define EMLP_RC 32             // reduction values staged in LDS per round
#define EMLP_WG_PAIRS 4        // row pairs in flight per trip of the weight gradient
#define EMLP_EPI_BIAS 0
#define EMLP_EPI_GELU 1
#define EMLP_EPI_DGELU 2

// the largest i in [0, rows) with splits[i] <= e (rows >= 1); the caller checks e < splits[i + 1]
SC_DEVICE long long emlp_row_of(const long long* splits, const long long rows, const long long e) {
  long long lo = 0, hi = rows;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (splits[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct EmlpGemmArgs {
  const float* A;              // rows b S + r at A + b a_bs + r lda; null: the lifted layer formed while loading
  const long long* splits;     // lift: [rows + 1]
  const long long* index;      // lift: [E]
  const float* Py;             // lift: [(b,) nPy, Kd]
  const float* Px;             // lift: [rows, Kd]
  const float* bias0;          // lift, optional: [Kd]
  const float* W;              // transb: [N][ldw] (B = W^T), else [Kd][ldw]
  const float* bias;           // optional [N]
  float* C;                    // b c_bs + r ldc
  float* Z;                    // b z_bs + r ldz: GELU keeps z here (optional), DGELU reads it
  long long a_bs, c_bs, z_bs, rows, E, nPy, Py_bs, e0;
  int lda, ldw, ldc, ldz, Kd, N, transb, epi, tiles, nvalid;
};

template <int NOB>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_emlp_gemm(const EmlpGemmArgs a) {
  constexpr int BW = 32 * NOB + 1;
  SC_SHARED float as[EMLP_ROWS * (EMLP_RC + 1)];
  SC_SHARED float bs[EMLP_RC * BW];
  SC_SHARED long long prow[EMLP_ROWS];
  SC_SHARED long long pcol[EMLP_ROWS];
  const int lane = SC_TID & 63, wave = SC_TID >> 6;
  const int b = SC_BID_X / a.tiles, rl0 = (SC_BID_X - b * a.tiles) * EMLP_ROWS;
  const int col0 = SC_BID_Y * 32 * NOB;
  if (!a.A && SC_TID < EMLP_ROWS) {
    const long long e = a.e0 + rl0 + SC_TID;
    long long px = -1, py = -1;
    if (rl0 + SC_TID < a.nvalid && e >= 0 && e < a.E && a.rows > 0) {
      const long long i = emlp_row_of(a.splits, a.rows, e);
      const long long j = a.index[e];
      if (a.splits[i] <= e && e < a.splits[i + 1] && j >= 0 && j < a.nPy) {
        px = i;
        py = j;
      }
    }
    prow[SC_TID] = px;
    pcol[SC_TID] = py;
  }
  sc_f32x16 acc[NOB];
#pragma unroll
  for (int u = 0; u < NOB; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[u][v] = 0.f;
#pragma unroll 1
  for (int r0 = 0; r0 < a.Kd; r0 += EMLP_RC) {
    SC_SYNC();
    if (a.A) {
#pragma unroll 4
      for (int t = SC_TID; t < EMLP_ROWS * EMLP_RC; t += 256) {
        const int r = t >> 5, k = r0 + (t & 31);
        as[r * (EMLP_RC + 1) + (t & 31)] =
            rl0 + r < a.nvalid && k < a.Kd ? a.A[b * a.a_bs + (size_t)(rl0 + r) * a.lda + k] : 0.f;
      }
    } else {
#pragma unroll 2
      for (int t = SC_TID; t < EMLP_ROWS * EMLP_RC; t += 256) {
        const int r = t >> 5, k = r0 + (t & 31);
        const long long px = prow[r], py = pcol[r];
        float h = 0.f;
        if (px >= 0 && k < a.Kd) {
          const float base = a.Px[px * a.Kd + k] + (a.bias0 ? a.bias0[k] : 0.f);
          h = sc_gelu(a.Py[b * a.Py_bs + py * a.Kd + k] + base);
        }
        as[r * (EMLP_RC + 1) + (t & 31)] = h;
      }
    }
    if (a.transb) {
#pragma unroll 4
      for (int t = SC_TID; t < EMLP_RC * 32 * NOB; t += 256) {
        const int j = t >> 5, rr = t & 31;
        bs[rr * BW + j] = col0 + j < a.N && r0 + rr < a.Kd ? a.W[(size_t)(col0 + j) * a.ldw + r0 + rr] : 0.f;
      }
    } else {
#pragma unroll 4
      for (int t = SC_TID; t < EMLP_RC * 32 * NOB; t += 256) {
        const int rr = t / (32 * NOB), j = t - rr * (32 * NOB);
        bs[rr * BW + j] = col0 + j < a.N && r0 + rr < a.Kd ? a.W[(size_t)(r0 + rr) * a.ldw + col0 + j] : 0.f;
      }
    }
    SC_SYNC();
    const float* ap = as + (wave * 32 + (lane & 31)) * (EMLP_RC + 1) + (lane >> 5);
    const float* bp = bs + (lane >> 5) * BW + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < EMLP_RC / 2; ++kk) {
      const float av = ap[2 * kk];
#pragma unroll
      for (int u = 0; u < NOB; ++u) sc_mfma_32x32x2(acc[u], av, bp[2 * kk * BW + 32 * u]);
    }
  }
#pragma unroll
  for (int u = 0; u < NOB; ++u) {
    const int col = col0 + 32 * u + (lane & 31);
    const float bv = a.bias && col < a.N ? a.bias[col] : 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int rl = rl0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
      if (rl >= a.nvalid || col >= a.N) continue;
      const size_t o = b * a.c_bs + (size_t)rl * a.ldc + col;
      if (a.epi == EMLP_EPI_BIAS) {
        a.C[o] = acc[u][v] + bv;
      } else if (a.epi == EMLP_EPI_GELU) {
        const float z = acc[u][v] + bv;
        if (a.Z) a.Z[b * a.z_bs + (size_t)rl * a.ldz + col] = z;
        a.C[o] = sc_gelu(z);
      } else {
        float gl, gr;
        sc_gelu_both(a.Z[b * a.z_bs + (size_t)rl * a.ldz + col], gl, gr);
        a.C[o] = acc[u][v] * gr;
      }
    }
  }
}

// ---- backward: the lifted layer of the chunk ---------------------------------------------------------------------------
struct EmlpLiftArgs {
  const long long* splits;
  const long long* index;
  const float* Py;
  const float* Px;
  const float* bias0;
  float* Z0;                   // [b][S][c]
  float* H0;                   // [b][S][c]
  long long rows, E, nPy, Py_bs, e0;
  int c, batch, S, nvalid;
};

// one wave per edge of the window; a row without a valid neighbour is zero in both
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_emlp_lift(const EmlpLiftArgs a) {
  const int lane = SC_TID & 63;
  const long long rl = (long long)SC_BID_X * 4 + (SC_TID >> 6);
  if (rl >= a.nvalid) return;
  const long long e = a.e0 + rl;
  long long px = -1, py = -1;
  if (e >= 0 && e < a.E && a.rows > 0) {
    const long long i = emlp_row_of(a.splits, a.rows, e);
    const long long j = a.index[e];
    if (a.splits[i] <= e && e < a.splits[i + 1] && j >= 0 && j < a.nPy) {
      px = i;
      py = j;
    }
  }
#pragma unroll 1
  for (int cc = lane; cc < a.c; cc += 64) {
    const float base = px >= 0 ? a.Px[px * a.c + cc] + (a.bias0 ? a.bias0[cc] : 0.f) : 0.f;
    for (int b = 0; b < a.batch; ++b) {
      const size_t o = ((size_t)b * a.S + rl) * a.c + cc;
      const float z = px >= 0 ? a.Py[b * a.Py_bs + py * a.c + cc] + base : 0.f;
      a.Z0[o] = z;
      a.H0[o] = px >= 0 ? sc_gelu(z) : 0.f;
    }
  }
}

// ---- backward: weight and bias gradient --------------------------------------------------------------------------------
struct EmlpWgArgs {
  const float* D;              // delta: row b S + r at D + b d_bs + r ldd, [co] wide
  const float* H;              // the layer's input: b h_bs + r ldh, [ci] wide
  float* parts;                // [slices][co][ci]
  float* parts_b;              // [slices][co]
  long long d_bs, h_bs, total, per_slice;      // total = batch S rows, cut into slices of per_slice (even)
  int ldd, ldh, co, ci, S, nvalid, slices;
};

template <int NOB>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_emlp_wgrad(const EmlpWgArgs a) {
  SC_SHARED float red[256];
  const int lane = SC_TID & 63, wave = SC_UNIFORM(SC_TID >> 6);
  const int ots = (a.co + 31) / 32, its = (a.ci + 32 * NOB - 1) / (32 * NOB);
  const long long job = (long long)SC_BID_X * 4 + wave;
  if (job >= (long long)a.slices * ots * its) return;        // wave-uniform
  const int it = (int)(job % its), ot = (int)((job / its) % ots), s = (int)(job / ((long long)its * ots));
  const long long r_lo = (long long)s * a.per_slice;
  const long long r_hi = r_lo + a.per_slice < a.total ? r_lo + a.per_slice : a.total;
  const int oc = ot * 32 + (lane & 31), ic0 = it * 32 * NOB + (lane & 31);
  sc_f32x16 acc[NOB];
#pragma unroll
  for (int u = 0; u < NOB; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[u][v] = 0.f;
  float bsum = 0.f;
#pragma unroll 1
  for (long long base = r_lo; base < r_hi; base += 2 * EMLP_WG_PAIRS) {
    float av[EMLP_WG_PAIRS], bv[EMLP_WG_PAIRS][NOB];
#pragma unroll
    for (int t = 0; t < EMLP_WG_PAIRS; ++t) {
      const long long row = base + 2 * t + (lane >> 5);
      const long long b = row / a.S, r = row - b * a.S;
      const bool ok = row < r_hi && r < a.nvalid;
      av[t] = ok && oc < a.co ? a.D[b * a.d_bs + r * a.ldd + oc] : 0.f;
#pragma unroll
      for (int u = 0; u < NOB; ++u) bv[t][u] = ok && ic0 + 32 * u < a.ci ? a.H[b * a.h_bs + r * a.ldh + ic0 + 32 * u] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < EMLP_WG_PAIRS; ++t) {
      bsum += av[t];
#pragma unroll
      for (int u = 0; u < NOB; ++u) sc_mfma_32x32x2(acc[u], av[t], bv[t][u]);
    }
  }
#pragma unroll
  for (int u = 0; u < NOB; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int o = ot * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5), i = ic0 + 32 * u;
      if (o < a.co && i < a.ci) a.parts[((size_t)s * a.co + o) * a.ci + i] = acc[u][v];
    }
  if (it == 0) {                                             // even rows of the slice, then odd rows
    red[SC_TID] = bsum;
    SC_WAVE_SYNC();
    if (lane < 32 && oc < a.co) a.parts_b[(size_t)s * a.co + oc] = red[wave * 64 + lane] + red[wave * 64 + lane + 32];
  }
}

// gw[t] += sum_s parts[s][t] and gb[o] += sum_s parts_b[s][o], slices ascending
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_emlp_wreduce(const float* __restrict__ parts, const float* __restrict__ parts_b,
                                                    float* __restrict__ gw, float* __restrict__ gb, const int co,
                                                    const int ci, const int slices) {
  const long long wn = (long long)co * ci, t = (long long)SC_BID_X * 256 + SC_TID;
  if (t < wn) {
    if (!gw) return;
    float acc = 0.f;
    for (int s = 0; s < slices; ++s) acc += parts[(size_t)s * wn + t];
    gw[t] += acc;
  } else if (t < wn + co && gb) {
    const int o = (int)(t - wn);
    float acc = 0.f;
    for (int s = 0; s < slices; ++s) acc += parts_b[(size_t)s * co + o];
    gb[o] += acc;
  }
}

// ---- backward: the two windowed reduces of delta_0 ---------------------------------------------------------------------
struct EmlpRedArgs {
  const long long* splits;     // rows: [rows + 1]; cols: col_splits [nPy + 1]
  const long long* index;      // [E]
  const int* perm;             // cols: [E]
  const float* D0;             // [b][S][c]
  float* out;                  // rows: gPx [rows][c]; cols: gPy [(b,) nPy][c]
  long long rows, E, nPy, out_bs, e0, e1;
  int c, batch, S, waves;
};

// waves stride over the rows that hold the window's first and last edge and those between; a row cut by the window's end
// is finished by the next chunk's launch
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_emlp_rows(const EmlpRedArgs a) {
  const int lane = SC_TID & 63;
  const long long w = (long long)SC_BID_X * 4 + (SC_TID >> 6);
  const long long r_lo = emlp_row_of(a.splits, a.rows, a.e0), r_hi = emlp_row_of(a.splits, a.rows, a.e1 - 1);
#pragma unroll 1
  for (long long r = r_lo + w; r <= r_hi; r += a.waves) {
    long long lo, hi;
    gno_segment(a.splits, r, a.E, lo, hi);
    lo = lo < a.e0 ? a.e0 : lo;
    hi = hi > a.e1 ? a.e1 : hi;
    if (lo >= hi) continue;
#pragma unroll 1
    for (int cc = lane; cc < a.c; cc += 64) {
      float acc = 0.f;
#pragma unroll 1
      for (long long e = lo; e < hi; ++e) {
        const long long j = a.index[e];
        if (j < 0 || j >= a.nPy) continue;
        float s = a.D0[(size_t)(e - a.e0) * a.c + cc];
        for (int b = 1; b < a.batch; ++b) s += a.D0[((size_t)b * a.S + (e - a.e0)) * a.c + cc];
        acc += s;
      }
      a.out[r * a.c + cc] += acc;
    }
  }
}

// one wave per edge of the window; the wave whose edge is the first of its column inside the window sums the column
SC_GLOBAL void SC_LAUNCH_BOUNDS(256) k_emlp_cols(const EmlpRedArgs a) {
  const int lane = SC_TID & 63;
  const long long e = a.e0 + (long long)SC_BID_X * 4 + (SC_TID >> 6);
  if (e >= a.e1) return;
  const long long j = a.index[e];
  if (j < 0 || j >= a.nPy) return;
  long long lo, hi;
  gno_segment(a.splits, j, a.E, lo, hi);
  long long k0 = lo, k1 = hi;                                // the first k in [lo, hi) with perm[k] >= e0
  while (k0 < k1) {
    const long long mid = (k0 + k1) >> 1;
    if ((long long)a.perm[mid] < a.e0) k0 = mid + 1;
    else k1 = mid;
  }
  if (k0 >= hi || (long long)a.perm[k0] != e) return;
#pragma unroll 1
  for (int cc = lane; cc < a.c; cc += 64) {
    for (int b = 0; b < a.batch; ++b) {
      float acc = 0.f;
#pragma unroll 1
      for (long long k = k0; k < hi; ++k) {
        const long long ee = a.perm[k];
        if (ee < a.e0 || ee >= a.e1) break;
        acc += a.D0[((size_t)b * a.S + (ee - a.e0)) * a.c + cc];
      }
      a.out[b * a.out_bs + j * a.c + cc] += acc;
    }
  }
}
