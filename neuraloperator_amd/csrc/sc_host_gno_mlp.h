// sc_host_gno_mlp.h -- host side of the chunked kernel MLP of the GNO layer (kernels: sc_kernels_gno_mlp.h).  One call
// walks the edges in chunks of S = chunk_edges; every launch of every chunk goes to the caller's stream in order and
// nothing waits for the device.  The workspace is a function of the descriptor's widths, batch and chunk size alone:
//   H_i, Z_i  [batch][S][widths[i]]  for the hidden layers i = 0 .. L-2   (the forward call uses H_1 .. H_{L-2} only)
//   parts     [slices][max_l widths[l] (widths[l-1] + 1)]                 (backward: partial weight / bias gradients)
// It does not grow with the edge count.  A bad descriptor is refused before any launch.
#pragma once
#include "sc_host_common.h"
#include "sc_kernels_gno_mlp.h"
#include "sc_host_gno.h"

#define EMLP_WS_TARGET ((size_t)128 << 20)  // the default chunk fills about this many bytes of H_i / Z_i
#define EMLP_MAX_SLICES 32

struct EmlpPlan {
  long long S, total, per_slice;
  int L, slices;
  size_t h_off[SC_EDGE_MLP_MAX_LAYERS], z_off[SC_EDGE_MLP_MAX_LAYERS], parts_off, parts_b_off, floats;
};

static int emlp_plan(const sc_edge_mlp_desc* d, EmlpPlan* p) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->n_layers >= 2 && d->n_layers <= SC_EDGE_MLP_MAX_LAYERS, "edge mlp: 2 to 8 layers");
  for (int i = 0; i < d->n_layers; ++i)
    SC_CHECK_ARG(d->widths[i] >= 1 && d->widths[i] <= SC_EDGE_MLP_MAX_WIDTH, "edge mlp: widths of 1 to 512");
  SC_CHECK_ARG(d->rows >= 0 && d->n_edges >= 0 && d->n_py >= 0, "edge mlp: negative count");
  SC_CHECK_ARG(d->rows < GNO_MAX && d->n_edges < GNO_MAX && d->n_py < GNO_MAX, "edge mlp: count out of range");
  SC_CHECK_ARG(d->n_splits == d->rows + 1, "edge mlp: splits must hold rows + 1 entries");
  SC_CHECK_ARG(d->batch >= 1 && d->batch <= (1 << 16), "edge mlp: 1 to 65536 batch entries");
  SC_CHECK_ARG(d->py_batch_stride >= 0, "edge mlp: negative batch stride");
  SC_CHECK_ARG(d->chunk_edges >= 0 && d->chunk_edges % SC_EDGE_MLP_TILE == 0 && d->chunk_edges <= (1 << 22),
               "edge mlp: chunk_edges must be a multiple of the row tile (128), at most 2^22");
  const int L = d->n_layers;
  size_t hidden = 0;                                         // floats of H_i and Z_i per edge of the chunk
  for (int i = 0; i + 1 < L; ++i) hidden += (size_t)2 * d->batch * d->widths[i];
  long long S = d->chunk_edges;
  if (S == 0) {
    S = (long long)(EMLP_WS_TARGET / sizeof(float) / hidden) / SC_EDGE_MLP_TILE * SC_EDGE_MLP_TILE;
    S = S < SC_EDGE_MLP_TILE ? SC_EDGE_MLP_TILE : (S > (1 << 18) ? (1 << 18) : S);
  }
  SC_CHECK_ARG(S * d->batch < GNO_MAX / 4, "edge mlp: chunk times batch out of range");
  p->S = S;
  p->L = L;
  p->total = S * d->batch;
  long long want = p->total / SC_EDGE_MLP_TILE;
  want = want > EMLP_MAX_SLICES ? EMLP_MAX_SLICES : want;
  p->per_slice = (p->total + want - 1) / want;
  p->per_slice += p->per_slice & 1;
  p->slices = (int)((p->total + p->per_slice - 1) / p->per_slice);
  size_t off = 0, wmax = 0;
  for (int i = 0; i + 1 < L; ++i) {
    p->h_off[i] = off;
    off += (size_t)p->total * d->widths[i];
    p->z_off[i] = off;
    off += (size_t)p->total * d->widths[i];
    const size_t w = (size_t)d->widths[i + 1] * d->widths[i];
    wmax = w > wmax ? w : wmax;
  }
  p->parts_off = off;
  off += (size_t)p->slices * wmax;
  p->parts_b_off = off;
  off += (size_t)p->slices * SC_EDGE_MLP_MAX_WIDTH;
  p->floats = off;
  return 0;
}

extern "C" size_t sc_edge_mlp_workspace_bytes(const sc_edge_mlp_desc* d) {
  EmlpPlan p;
  if (emlp_plan(d, &p)) return 0;
  return p.floats * sizeof(float);
}

static int emlp_zero(float* p, const long long n, sc_stream_t st) {
  SC_LAUNCH(k_fill_i32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int*)p, n, 0);
  return sc_check_launch("k_fill_i32");
}

static int emlp_gemm_launch(const EmlpGemmArgs& g, const int batch, sc_stream_t st) {
  const int nob = g.N > 64 ? 4 : (g.N > 32 ? 2 : 1);
  const dim3 grid((unsigned)(batch * g.tiles), (unsigned)((g.N + 32 * nob - 1) / (32 * nob)));
  if (nob == 4) SC_LAUNCH(k_emlp_gemm<4>, grid, dim3(256), 0, st, g);
  else if (nob == 2) SC_LAUNCH(k_emlp_gemm<2>, grid, dim3(256), 0, st, g);
  else SC_LAUNCH(k_emlp_gemm<1>, grid, dim3(256), 0, st, g);
  return sc_check_launch("k_emlp_gemm");
}

// the checks both calls share; *empty: a valid problem without an edge
static int emlp_check(const sc_edge_mlp_desc* d, EmlpPlan* p, const float* Py, const float* Px, const float* const* W,
                      const void* ws, const size_t ws_bytes, bool* empty) {
  if (int e = emlp_plan(d, p)) return e;
  *empty = d->rows == 0 || d->n_edges == 0;
  if (*empty) return 0;
  SC_CHECK_ARG(d->splits && d->index && Py && Px && W && ws, "null argument");
  for (int l = 0; l + 1 < d->n_layers; ++l) SC_CHECK_ARG(W[l], "null argument");
  SC_CHECK_ARG(ws_bytes >= p->floats * sizeof(float), "edge mlp: workspace too small");
  return 0;
}

static void emlp_lift_source(EmlpGemmArgs* g, const sc_edge_mlp_desc* d, const float* Py, const float* Px,
                             const float* bias0) {
  g->A = nullptr;
  g->splits = (const long long*)d->splits;
  g->index = (const long long*)d->index;
  g->Py = Py;
  g->Px = Px;
  g->bias0 = bias0;
  g->rows = d->rows;
  g->E = d->n_edges;
  g->nPy = d->n_py;
  g->Py_bs = d->py_batch_stride;
}

extern "C" int sc_edge_mlp_forward(const sc_edge_mlp_desc* d, const float* Py, const float* Px, const float* bias0,
                                   const float* const* W, const float* const* b, float* K, void* ws, size_t ws_bytes,
                                   void* stream) {
  EmlpPlan p;
  bool empty;
  if (int e = emlp_check(d, &p, Py, Px, W, ws, ws_bytes, &empty)) return e;
  if (empty) return 0;
  SC_CHECK_ARG(K, "null argument");
  sc_stream_t st = (sc_stream_t)stream;
  float* base = (float*)ws;
  const int L = p.L, c_out = d->widths[L - 1];
  for (long long e0 = 0; e0 < d->n_edges; e0 += p.S) {
    const long long nvalid = d->n_edges - e0 < p.S ? d->n_edges - e0 : p.S;
    for (int l = 1; l < L; ++l) {
      EmlpGemmArgs g;
      std::memset(&g, 0, sizeof(g));
      const int ci = d->widths[l - 1], co = d->widths[l];
      if (l == 1) {
        emlp_lift_source(&g, d, Py, Px, bias0);
      } else {
        g.A = base + p.h_off[l - 1];
        g.a_bs = p.S * ci;
        g.lda = ci;
      }
      g.W = W[l - 1];
      g.ldw = ci;
      g.transb = 1;
      g.bias = b ? b[l - 1] : nullptr;
      g.Kd = ci;
      g.N = co;
      g.e0 = e0;
      g.nvalid = (int)nvalid;
      g.tiles = (int)((nvalid + EMLP_ROWS - 1) / EMLP_ROWS);
      if (l == L - 1) {
        g.C = K + (size_t)e0 * c_out;
        g.c_bs = d->n_edges * c_out;
        g.ldc = c_out;
        g.epi = EMLP_EPI_BIAS;
      } else {
        g.C = base + p.h_off[l];
        g.c_bs = p.S * co;
        g.ldc = co;
        g.epi = EMLP_EPI_GELU;
      }
      if (int e = emlp_gemm_launch(g, d->batch, st)) return e;
    }
  }
  return 0;
}

extern "C" int sc_edge_mlp_backward(const sc_edge_mlp_desc* d, const float* Py, const float* Px, const float* bias0,
                                    const float* const* W, const float* const* b, const float* gK, float* gPy,
                                    float* gPx, float* const* gW, float* const* gb, void* ws, size_t ws_bytes,
                                    void* stream) {
  EmlpPlan p;
  bool empty;
  if (int e = emlp_check(d, &p, Py, Px, W, ws, ws_bytes, &empty)) return e;
  SC_CHECK_ARG(gW && gb, "null argument");
  sc_stream_t st = (sc_stream_t)stream;
  const int L = p.L, c1 = d->widths[0], c_out = d->widths[L - 1];
  const bool pyb = d->py_batch_stride != 0;
  // the gradients are this call's to fill: chunks add into them.  A kernel, not a memset: the zeros are then ordered
  // with the adds as launches are, in a captured graph too
  if (gPy && d->n_py)
    if (int e = emlp_zero(gPy, (long long)(pyb ? d->batch : 1) * d->n_py * c1, st)) return e;
  if (gPx && d->rows)
    if (int e = emlp_zero(gPx, (long long)d->rows * c1, st)) return e;
  for (int l = 1; l < L; ++l) {
    if (gW[l - 1])
      if (int e = emlp_zero(gW[l - 1], (long long)d->widths[l] * d->widths[l - 1], st)) return e;
    if (gb[l - 1])
      if (int e = emlp_zero(gb[l - 1], d->widths[l], st)) return e;
  }
  if (empty) return 0;
  SC_CHECK_ARG(gK && (!gPy || (d->col_splits && d->perm)), "null argument");
  SC_CHECK_ARG(pyb || d->batch == 1, "edge mlp: a batch needs batched Py");
  float* base = (float*)ws;
  for (long long e0 = 0; e0 < d->n_edges; e0 += p.S) {
    const long long nvalid = d->n_edges - e0 < p.S ? d->n_edges - e0 : p.S;
    const int tiles = (int)((nvalid + EMLP_ROWS - 1) / EMLP_ROWS);
    {
      EmlpLiftArgs a;
      std::memset(&a, 0, sizeof(a));
      a.splits = (const long long*)d->splits;
      a.index = (const long long*)d->index;
      a.Py = Py;
      a.Px = Px;
      a.bias0 = bias0;
      a.Z0 = base + p.z_off[0];
      a.H0 = base + p.h_off[0];
      a.rows = d->rows;
      a.E = d->n_edges;
      a.nPy = d->n_py;
      a.Py_bs = d->py_batch_stride;
      a.e0 = e0;
      a.c = c1;
      a.batch = d->batch;
      a.S = (int)p.S;
      a.nvalid = (int)nvalid;
      SC_LAUNCH(k_emlp_lift, dim3((unsigned)((nvalid + 3) / 4)), dim3(256), 0, st, a);
      if (int e = sc_check_launch("k_emlp_lift")) return e;
    }
    // the chain again, keeping the pre-activations
    for (int l = 1; l + 1 < L; ++l) {
      EmlpGemmArgs g;
      std::memset(&g, 0, sizeof(g));
      const int ci = d->widths[l - 1], co = d->widths[l];
      g.A = base + p.h_off[l - 1];
      g.a_bs = p.S * ci;
      g.lda = ci;
      g.W = W[l - 1];
      g.ldw = ci;
      g.transb = 1;
      g.bias = b ? b[l - 1] : nullptr;
      g.Kd = ci;
      g.N = co;
      g.e0 = e0;
      g.nvalid = (int)nvalid;
      g.tiles = tiles;
      g.C = base + p.h_off[l];
      g.c_bs = p.S * co;
      g.ldc = co;
      g.Z = base + p.z_off[l];
      g.z_bs = p.S * co;
      g.ldz = co;
      g.epi = EMLP_EPI_GELU;
      if (int e = emlp_gemm_launch(g, d->batch, st)) return e;
    }
    // delta_{L-1} is the chunk's rows of gK; delta_{l-1} replaces z_{l-1} in place
    for (int l = L - 1; l >= 1; --l) {
      const int ci = d->widths[l - 1], co = d->widths[l];
      const float* D = l == L - 1 ? gK + (size_t)e0 * c_out : base + p.z_off[l];
      const long long d_bs = l == L - 1 ? d->n_edges * c_out : p.S * co;
      if (gW[l - 1] || gb[l - 1]) {
        EmlpWgArgs a;
        std::memset(&a, 0, sizeof(a));
        a.D = D;
        a.d_bs = d_bs;
        a.ldd = co;
        a.H = base + p.h_off[l - 1];
        a.h_bs = p.S * ci;
        a.ldh = ci;
        a.parts = base + p.parts_off;
        a.parts_b = base + p.parts_b_off;
        a.total = p.total;
        a.per_slice = p.per_slice;
        a.co = co;
        a.ci = ci;
        a.S = (int)p.S;
        a.nvalid = (int)nvalid;
        a.slices = p.slices;
        const int nob = ci > 64 ? 4 : (ci > 32 ? 2 : 1);
        const long long jobs = (long long)p.slices * ((co + 31) / 32) * ((ci + 32 * nob - 1) / (32 * nob));
        const dim3 grid((unsigned)((jobs + 3) / 4));
        if (nob == 4) SC_LAUNCH(k_emlp_wgrad<4>, grid, dim3(256), 0, st, a);
        else if (nob == 2) SC_LAUNCH(k_emlp_wgrad<2>, grid, dim3(256), 0, st, a);
        else SC_LAUNCH(k_emlp_wgrad<1>, grid, dim3(256), 0, st, a);
        if (int e = sc_check_launch("k_emlp_wgrad")) return e;
        const long long n = (long long)co * ci + co;
        SC_LAUNCH(k_emlp_wreduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)a.parts,
                  (const float*)a.parts_b, gW[l - 1], gb[l - 1], co, ci, p.slices);
        if (int e = sc_check_launch("k_emlp_wreduce")) return e;
      }
      EmlpGemmArgs g;
      std::memset(&g, 0, sizeof(g));
      g.A = D;
      g.a_bs = d_bs;
      g.lda = co;
      g.W = W[l - 1];
      g.ldw = ci;
      g.transb = 0;
      g.Kd = co;
      g.N = ci;
      g.e0 = e0;
      g.nvalid = (int)nvalid;
      g.tiles = tiles;
      g.C = base + p.z_off[l - 1];
      g.c_bs = p.S * ci;
      g.ldc = ci;
      g.Z = g.C;
      g.z_bs = g.c_bs;
      g.ldz = ci;
      g.epi = EMLP_EPI_DGELU;
      if (int e = emlp_gemm_launch(g, d->batch, st)) return e;
    }
    EmlpRedArgs r;
    std::memset(&r, 0, sizeof(r));
    r.index = (const long long*)d->index;
    r.D0 = base + p.z_off[0];
    r.rows = d->rows;
    r.E = d->n_edges;
    r.nPy = d->n_py;
    r.e0 = e0;
    r.e1 = e0 + nvalid;
    r.c = c1;
    r.batch = d->batch;
    r.S = (int)p.S;
    if (gPx) {
      r.splits = (const long long*)d->splits;
      r.out = gPx;
      const unsigned wgs = (unsigned)((nvalid + 3) / 4 < 2048 ? (nvalid + 3) / 4 : 2048);
      r.waves = (int)wgs * 4;
      SC_LAUNCH(k_emlp_rows, dim3(wgs), dim3(256), 0, st, r);
      if (int e = sc_check_launch("k_emlp_rows")) return e;
    }
    if (gPy) {
      r.splits = (const long long*)d->col_splits;
      r.perm = d->perm;
      r.out = gPy;
      r.out_bs = d->n_py * c1;
      SC_LAUNCH(k_emlp_cols, dim3((unsigned)((nvalid + 3) / 4)), dim3(256), 0, st, r);
      if (int e = sc_check_launch("k_emlp_cols")) return e;
    }
  }
  return 0;
}
