// sc_host_gno.h -- host side of the graph neural operator entry points (kernels: sc_kernels_gno.h).  Every entry point
// refuses a bad descriptor before any launch; a valid empty problem (no queries, no data points, no edges) returns
// success without a launch, after zero-filling whatever output it owes.
#pragma once
#include "sc_host_common.h"
#include "sc_kernels_gno.h"

#define GNO_MAX (((int64_t)1 << 31) - 1)

static int gno_cp2(const int c) {
  int p = 1;
  while (p < c && p < 64) p <<= 1;
  return p;
}

static int gno_radius_check(const sc_radius_desc* d, const float* data, const float* queries) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->d >= 1 && d->d <= 3, "radius search: d must be 1, 2 or 3");
  SC_CHECK_ARG(d->n >= 0 && d->m >= 0, "radius search: negative point count");
  SC_CHECK_ARG(d->n < GNO_MAX && d->m < GNO_MAX, "radius search: point count out of range");
  SC_CHECK_ARG(d->radius >= 0.0 && d->radius == d->radius, "radius search: the radius must be a number >= 0");
  SC_CHECK_ARG((data || d->n == 0) && (queries || d->m == 0), "null argument");
  return 0;
}

template <bool FILL>
static void gno_radius_launch(const int dim, const RadiusArgs& a, sc_stream_t st) {
  const dim3 grid((unsigned)((a.m + GNO_QPB - 1) / GNO_QPB));
  if (dim == 1) SC_LAUNCH((k_radius<1, FILL>), grid, dim3(256), 0, st, a);
  else if (dim == 2) SC_LAUNCH((k_radius<2, FILL>), grid, dim3(256), 0, st, a);
  else SC_LAUNCH((k_radius<3, FILL>), grid, dim3(256), 0, st, a);
}

extern "C" int sc_radius_count(const sc_radius_desc* d, const float* data, const float* queries, int32_t* deg,
                               int64_t* row_splits, void* stream) {
  if (int e = gno_radius_check(d, data, queries)) return e;
  SC_CHECK_ARG(row_splits && (deg || d->m == 0), "null argument");
  if (d->m == 0 || d->n == 0) {
    SC_CHECK_HIP(hipMemsetAsync(row_splits, 0, (size_t)(d->m + 1) * sizeof(int64_t), (sc_stream_t)stream));
    if (d->m) SC_CHECK_HIP(hipMemsetAsync(deg, 0, (size_t)d->m * sizeof(int32_t), (sc_stream_t)stream));
    return 0;
  }
  RadiusArgs a;
  std::memset(&a, 0, sizeof(a));
  a.data = data;
  a.queries = queries;
  a.n = d->n;
  a.m = d->m;
  a.r2 = (float)(d->radius * d->radius);
  a.deg = deg;
  gno_radius_launch<false>(d->d, a, (sc_stream_t)stream);
  if (int e = sc_check_launch("k_radius (count)")) return e;
  SC_LAUNCH(k_scan_i32, dim3(1), dim3(256), 0, (sc_stream_t)stream, (const int*)deg, (long long*)row_splits,
            (long long)d->m);
  return sc_check_launch("k_scan_i32");
}

extern "C" int sc_radius_fill(const sc_radius_desc* d, const float* data, const float* queries, const int64_t* row_splits,
                              int64_t n_edges, int64_t* index, float* weights, void* stream) {
  if (int e = gno_radius_check(d, data, queries)) return e;
  SC_CHECK_ARG(n_edges >= 0 && n_edges < GNO_MAX, "radius search: edge count out of range");
  SC_CHECK_ARG(row_splits, "null argument");
  if (d->m == 0 || d->n == 0 || n_edges == 0) return 0;
  SC_CHECK_ARG(index && (weights || !d->return_norm), "null argument");
  RadiusArgs a;
  std::memset(&a, 0, sizeof(a));
  a.data = data;
  a.queries = queries;
  a.n = d->n;
  a.m = d->m;
  a.E = n_edges;
  a.r2 = (float)(d->radius * d->radius);
  a.splits = (const long long*)row_splits;
  a.index = (long long*)index;
  a.weights = d->return_norm ? weights : nullptr;
  gno_radius_launch<true>(d->d, a, (sc_stream_t)stream);
  return sc_check_launch("k_radius (fill)");
}

static int gno_csr_check(const sc_csr_desc* d) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->rows >= 0 && d->cols >= 0 && d->n_edges >= 0, "csr transpose: negative count");
  SC_CHECK_ARG(d->rows < GNO_MAX && d->cols < GNO_MAX && d->n_edges < GNO_MAX, "csr transpose: count out of range");
  SC_CHECK_ARG(d->n_splits == d->rows + 1, "csr transpose: row_splits must hold rows + 1 entries");
  return 0;
}

extern "C" size_t sc_csr_transpose_workspace_bytes(const sc_csr_desc* d) {
  if (gno_csr_check(d)) return 0;
  return (size_t)(d->cols + d->n_edges + 1) * sizeof(int32_t);
}

extern "C" int sc_csr_transpose(const sc_csr_desc* d, const int64_t* row_splits, const int64_t* index,
                                int64_t* col_splits, int32_t* perm, int32_t* row_of_edge, void* ws, size_t ws_bytes,
                                void* stream) {
  if (int e = gno_csr_check(d)) return e;
  SC_CHECK_ARG(col_splits, "null argument");
  sc_stream_t st = (sc_stream_t)stream;
  if (d->n_edges == 0 || d->cols == 0 || d->rows == 0) {
    SC_CHECK_HIP(hipMemsetAsync(col_splits, 0, (size_t)(d->cols + 1) * sizeof(int64_t), st));
    return 0;
  }
  SC_CHECK_ARG(row_splits && index && perm && row_of_edge && ws, "null argument");
  SC_CHECK_ARG(ws_bytes >= sc_csr_transpose_workspace_bytes(d), "csr transpose: workspace too small");
  CsrTArgs a;
  std::memset(&a, 0, sizeof(a));
  a.splits = (const long long*)row_splits;
  a.index = (const long long*)index;
  a.rows = d->rows;
  a.cols = d->cols;
  a.E = d->n_edges;
  a.cnt = (int*)ws;
  a.tmp = a.cnt + d->cols;
  a.col_splits = (const long long*)col_splits;
  a.perm = perm;
  a.row_of_edge = row_of_edge;
  const dim3 eg((unsigned)((a.E + 255) / 256));
  const dim3 cg((unsigned)((a.cols + 255) / 256));
  SC_LAUNCH(k_fill_i32, cg, dim3(256), 0, st, a.cnt, (long long)a.cols, 0);
  if (int e = sc_check_launch("k_fill_i32")) return e;
  SC_LAUNCH(k_csr_hist, eg, dim3(256), 0, st, a);
  if (int e = sc_check_launch("k_csr_hist")) return e;
  SC_LAUNCH(k_scan_i32, dim3(1), dim3(256), 0, st, (const int*)a.cnt, (long long*)col_splits, (long long)d->cols);
  if (int e = sc_check_launch("k_scan_i32")) return e;
  SC_LAUNCH(k_fill_i32, cg, dim3(256), 0, st, a.cnt, (long long)a.cols, 0);
  if (int e = sc_check_launch("k_fill_i32")) return e;
  // an edge whose index lies outside [0, cols) joins no column: its slots at the end of perm keep this fill
  SC_LAUNCH(k_fill_i32, eg, dim3(256), 0, st, (int*)perm, (long long)a.E, -1);
  if (int e = sc_check_launch("k_fill_i32")) return e;
  SC_LAUNCH(k_csr_slot, eg, dim3(256), 0, st, a);
  if (int e = sc_check_launch("k_csr_slot")) return e;
  SC_LAUNCH(k_csr_sortcols, dim3((unsigned)((a.cols + 3) / 4)), dim3(256), 0, st, a);
  return sc_check_launch("k_csr_sortcols");
}

// the checks sc_csr_reduce and sc_csr_edge_grad share; fills the kernel arguments
static int gno_reduce_args(const sc_csr_reduce_desc* d, CsrArgs* a) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->rows >= 0 && d->n_edges >= 0 && d->n_f >= 0 && d->n_scale_rows >= 0, "csr reduce: negative count");
  SC_CHECK_ARG(d->rows < GNO_MAX && d->n_edges < GNO_MAX && d->n_f < GNO_MAX && d->n_scale_rows < GNO_MAX,
               "csr reduce: count out of range");
  SC_CHECK_ARG(d->n_splits == d->rows + 1, "csr reduce: splits must hold rows + 1 entries");
  SC_CHECK_ARG(d->channels >= 1 && d->channels <= (1 << 16), "csr reduce: 1 to 65536 channels");
  SC_CHECK_ARG(d->batch >= 1 && d->batch <= (1 << 16), "csr reduce: 1 to 65536 batch entries");
  SC_CHECK_ARG(d->rows * d->batch < GNO_MAX, "csr reduce: too many rows for one launch");
  SC_CHECK_ARG(d->k_batch_stride >= 0 && d->f_batch_stride >= 0, "csr reduce: negative batch stride");
  SC_CHECK_ARG(d->splits, "null argument");
  SC_CHECK_ARG(!(d->gather64 && d->gather32) || d->scale_splits, "csr reduce: one gather array");
  SC_CHECK_ARG(!d->scale_splits || d->gather32, "csr reduce: the edge scale needs the row of every edge");
  std::memset(a, 0, sizeof(*a));
  a->splits = (const long long*)d->splits;
  a->perm = d->perm;
  a->g64 = (const long long*)d->gather64;
  a->g32 = d->gather32;
  a->ssplits = (const long long*)d->scale_splits;
  a->w = d->w;
  a->rows = d->rows;
  a->E = d->n_edges;
  a->nF = d->n_f;
  a->nS = d->n_scale_rows;
  a->K_bs = d->k_batch_stride;
  a->F_bs = d->f_batch_stride;
  a->c = d->channels;
  a->cp2 = gno_cp2(d->channels);
  a->batch = d->batch;
  a->mean = d->mean ? 1 : 0;
  return 0;
}

extern "C" int sc_csr_reduce(const sc_csr_reduce_desc* d, const float* K, const float* F, float* out, void* stream) {
  CsrArgs a;
  if (int e = gno_reduce_args(d, &a)) return e;
  if (d->rows == 0) return 0;
  SC_CHECK_ARG(out, "null argument");
  if (d->n_edges == 0) {
    SC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)d->rows * d->batch * d->channels * sizeof(float), (sc_stream_t)stream));
    return 0;
  }
  SC_CHECK_ARG(K, "null argument");
  a.K = K;
  a.F = F;
  a.out = out;
  SC_LAUNCH(k_csr_reduce, dim3((unsigned)((d->rows * d->batch + 3) / 4)), dim3(256), 0, (sc_stream_t)stream, a);
  return sc_check_launch("k_csr_reduce");
}

extern "C" int sc_csr_edge_grad(const sc_csr_reduce_desc* d, const float* g, const float* F, float* gK, void* stream) {
  CsrArgs a;
  if (int e = gno_reduce_args(d, &a)) return e;
  SC_CHECK_ARG(!d->perm && !d->scale_splits, "csr edge grad: rows of the graph itself, no indirection");
  if (d->rows == 0 || d->n_edges == 0) return 0;
  SC_CHECK_ARG(g && gK, "null argument");
  a.g = g;
  a.F = F;
  a.out = gK;
  SC_LAUNCH(k_csr_edge_grad, dim3((unsigned)((d->rows + 3) / 4)), dim3(256), 0, (sc_stream_t)stream, a);
  return sc_check_launch("k_csr_edge_grad");
}

static int gno_lift(const sc_edge_lift_desc* d, const float* Py, const float* Px, const float* bias, const float* gH,
                    float* out, const bool bwd, void* stream) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->rows >= 0 && d->n_edges >= 0 && d->n_py >= 0, "edge lift: negative count");
  SC_CHECK_ARG(d->rows < GNO_MAX && d->n_edges < GNO_MAX && d->n_py < GNO_MAX, "edge lift: count out of range");
  SC_CHECK_ARG(d->n_splits == d->rows + 1, "edge lift: splits must hold rows + 1 entries");
  SC_CHECK_ARG(d->channels >= 1 && d->channels <= (1 << 16), "edge lift: 1 to 65536 channels");
  SC_CHECK_ARG(d->batch >= 1 && d->batch <= (1 << 16), "edge lift: 1 to 65536 batch entries");
  SC_CHECK_ARG(d->py_batch_stride >= 0, "edge lift: negative batch stride");
  SC_CHECK_ARG(d->act == SC_LIFT_IDENTITY || d->act == SC_LIFT_GELU, "edge lift: unknown activation");
  SC_CHECK_ARG(d->splits && d->index, "null argument");
  if (d->rows == 0 || d->n_edges == 0) return 0;
  SC_CHECK_ARG(Py && Px && out && (gH || !bwd), "null argument");
  LiftArgs a;
  std::memset(&a, 0, sizeof(a));
  a.splits = (const long long*)d->splits;
  a.index = (const long long*)d->index;
  a.Py = Py;
  a.Px = Px;
  a.bias = bias;
  a.gH = gH;
  a.out = out;
  a.rows = d->rows;
  a.E = d->n_edges;
  a.nPy = d->n_py;
  a.Py_bs = d->py_batch_stride;
  a.c = d->channels;
  a.cp2 = gno_cp2(d->channels);
  a.batch = d->batch;
  a.gelu = d->act == SC_LIFT_GELU;
  const dim3 grid((unsigned)((d->rows + 3) / 4));
  if (bwd) SC_LAUNCH(k_edge_lift<true>, grid, dim3(256), 0, (sc_stream_t)stream, a);
  else SC_LAUNCH(k_edge_lift<false>, grid, dim3(256), 0, (sc_stream_t)stream, a);
  return sc_check_launch(bwd ? "k_edge_lift<bwd>" : "k_edge_lift");
}

extern "C" int sc_edge_lift(const sc_edge_lift_desc* d, const float* Py, const float* Px, const float* bias, float* H,
                            void* stream) {
  return gno_lift(d, Py, Px, bias, nullptr, H, false, stream);
}

extern "C" int sc_edge_lift_bwd(const sc_edge_lift_desc* d, const float* Py, const float* Px, const float* bias,
                                const float* gH, float* gPre, void* stream) {
  return gno_lift(d, Py, Px, bias, gH, gPre, true, stream);
}
