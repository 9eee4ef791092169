// sc_host_gno_grid.h -- host side of the cell-grid route of the fixed-radius search (kernels: sc_kernels_gno_grid.h).
// Same descriptor, same refusals and same bytes out as sc_radius_count / sc_radius_fill; the grid lives in a workspace
// whose size depends on the descriptor alone, and the host reads nothing back from it.
#pragma once
#include "sc_host_gno.h"
#include "sc_kernels_gno_grid.h"

// cells the workspace holds: four per data point, in whole scan blocks, at least one block and at most the caps' product
static int64_t gno_grid_cells_max(const sc_radius_desc* d) {
  const int64_t cap = d->d == 1 ? GNO_GRID_CAP1 : (d->d == 2 ? (int64_t)GNO_GRID_CAP2 * GNO_GRID_CAP2
                                                             : (int64_t)GNO_GRID_CAP3 * GNO_GRID_CAP3 * GNO_GRID_CAP3);
  int64_t c = (4 * d->n + GNO_GRID_SCAN_BLOCK - 1) / GNO_GRID_SCAN_BLOCK * GNO_GRID_SCAN_BLOCK;
  if (c < GNO_GRID_SCAN_BLOCK) c = GNO_GRID_SCAN_BLOCK;
  return c < cap ? c : cap;
}

// r2 = inf keeps every pair of finite points and pairs with an infinite coordinate too: one cell, which is the
// brute-force kernel -- the grid entry points hand such a radius to it
static bool gno_grid_r2_overflows(const sc_radius_desc* d) {
  const float r2 = (float)(d->radius * d->radius);
  return !(r2 <= 3.4028234663852886e38f);
}

extern "C" size_t sc_radius_grid_workspace_bytes(const sc_radius_desc* d) {
  static const float some = 0.f;                             // the size does not depend on the pointers
  if (gno_radius_check(d, &some, &some)) return 0;
  const int64_t cells = gno_grid_cells_max(d);
  return sizeof(GridHead) + sizeof(float) * 6 * GNO_GRID_RB + sizeof(int32_t) * (size_t)(cells / GNO_GRID_SCAN_BLOCK + 1) +
         sizeof(int32_t) * (size_t)(2 * cells + 2) + (size_t)d->n * 16 + (size_t)d->m * 4;
}

// the kernel arguments of both passes: the workspace cut into its arrays
static void gno_grid_args(const sc_radius_desc* d, const float* data, const float* queries, void* ws, GridArgs* a) {
  std::memset(a, 0, sizeof(*a));
  a->data = data;
  a->queries = queries;
  a->n = d->n;
  a->m = d->m;
  a->r2 = (float)(d->radius * d->radius);
  a->h = (d->radius + GNO_GRID_SLACK) * (1.0 + GNO_GRID_MARGIN);
  a->dim = d->d;
  a->cap = d->d == 1 ? GNO_GRID_CAP1 : (d->d == 2 ? GNO_GRID_CAP2 : GNO_GRID_CAP3);
  a->cells = (int)gno_grid_cells_max(d);
  char* p = (char*)ws;
  a->head = (GridHead*)p;
  p += sizeof(GridHead);
  a->part = (float*)p;
  p += sizeof(float) * 6 * GNO_GRID_RB;
  a->bsum = (int*)p;
  p += sizeof(int32_t) * (size_t)(a->cells / GNO_GRID_SCAN_BLOCK + 1);
  a->cnt = (int*)p;
  p += sizeof(int32_t) * (size_t)a->cells;
  a->start = (int*)p;
  p += sizeof(int32_t) * (size_t)(a->cells + 2);
  a->sx = (float*)p;
  a->sy = a->sx + d->n;
  a->sz = a->sy + d->n;
  a->sidx = (int*)(a->sz + d->n);
  a->longrows = a->sidx + d->n;
}

#define GNO_GRID_LAUNCH_D(kernel, dim, grid, st, a)                          \
  do {                                                                       \
    if ((dim) == 1) SC_LAUNCH((kernel<1>), grid, dim3(256), 0, st, a);       \
    else if ((dim) == 2) SC_LAUNCH((kernel<2>), grid, dim3(256), 0, st, a);  \
    else SC_LAUNCH((kernel<3>), grid, dim3(256), 0, st, a);                  \
  } while (0)

template <bool FILL>
static void gno_grid_query_launch(const int dim, const GridArgs& a, sc_stream_t st) {
  const dim3 grid((unsigned)((a.m + GNO_GRID_QPB - 1) / GNO_GRID_QPB));
  if (dim == 1) SC_LAUNCH((k_grid_query<1, FILL>), grid, dim3(256), 0, st, a);
  else if (dim == 2) SC_LAUNCH((k_grid_query<2, FILL>), grid, dim3(256), 0, st, a);
  else SC_LAUNCH((k_grid_query<3, FILL>), grid, dim3(256), 0, st, a);
}

extern "C" int sc_radius_grid_count(const sc_radius_desc* d, const float* data, const float* queries, int32_t* deg,
                                    int64_t* row_splits, void* ws, size_t ws_bytes, void* stream) {
  if (int e = gno_radius_check(d, data, queries)) return e;
  SC_CHECK_ARG(row_splits && (deg || d->m == 0), "null argument");
  sc_stream_t st = (sc_stream_t)stream;
  if (d->m == 0 || d->n == 0) {
    SC_CHECK_HIP(hipMemsetAsync(row_splits, 0, (size_t)(d->m + 1) * sizeof(int64_t), st));
    if (d->m) SC_CHECK_HIP(hipMemsetAsync(deg, 0, (size_t)d->m * sizeof(int32_t), st));
    return 0;
  }
  SC_CHECK_ARG(ws, "null argument");
  SC_CHECK_ARG(ws_bytes >= sc_radius_grid_workspace_bytes(d), "radius search: grid workspace too small");
  if (gno_grid_r2_overflows(d)) return sc_radius_count(d, data, queries, deg, row_splits, stream);
  GridArgs a;
  gno_grid_args(d, data, queries, ws, &a);
  a.deg = deg;
  const int64_t pb = (d->n + 255) / 256;
  a.nb = (int)(pb < GNO_GRID_RB ? pb : GNO_GRID_RB);
  const dim3 pg((unsigned)pb), cg((unsigned)(a.cells / GNO_GRID_SCAN_BLOCK));
  SC_LAUNCH(k_grid_bounds, dim3((unsigned)a.nb), dim3(256), 0, st, a);
  if (int e = sc_check_launch("k_grid_bounds")) return e;
  SC_LAUNCH(k_grid_params, dim3(1), dim3(256), 0, st, a);
  if (int e = sc_check_launch("k_grid_params")) return e;
  SC_LAUNCH(k_grid_zero, cg, dim3(256), 0, st, a);
  if (int e = sc_check_launch("k_grid_zero")) return e;
  GNO_GRID_LAUNCH_D(k_grid_hist, d->d, pg, st, a);
  if (int e = sc_check_launch("k_grid_hist")) return e;
  SC_LAUNCH(k_grid_scan_sums, cg, dim3(256), 0, st, a);
  if (int e = sc_check_launch("k_grid_scan_sums")) return e;
  SC_LAUNCH(k_grid_scan, cg, dim3(256), 0, st, a);
  if (int e = sc_check_launch("k_grid_scan")) return e;
  GNO_GRID_LAUNCH_D(k_grid_scatter, d->d, pg, st, a);
  if (int e = sc_check_launch("k_grid_scatter")) return e;
  gno_grid_query_launch<false>(d->d, a, st);
  if (int e = sc_check_launch("k_grid_query (count)")) return e;
  SC_LAUNCH(k_scan_i32, dim3(1), dim3(256), 0, st, (const int*)deg, (long long*)row_splits, (long long)d->m);
  return sc_check_launch("k_scan_i32");
}

extern "C" int sc_radius_grid_fill(const sc_radius_desc* d, const float* data, const float* queries,
                                   const int64_t* row_splits, int64_t n_edges, int64_t* index, float* weights, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (int e = gno_radius_check(d, data, queries)) return e;
  SC_CHECK_ARG(n_edges >= 0 && n_edges < GNO_MAX, "radius search: edge count out of range");
  SC_CHECK_ARG(row_splits, "null argument");
  if (d->m == 0 || d->n == 0 || n_edges == 0) return 0;
  SC_CHECK_ARG(index && (weights || !d->return_norm), "null argument");
  SC_CHECK_ARG(ws, "null argument");
  SC_CHECK_ARG(ws_bytes >= sc_radius_grid_workspace_bytes(d), "radius search: grid workspace too small");
  if (gno_grid_r2_overflows(d)) return sc_radius_fill(d, data, queries, row_splits, n_edges, index, weights, stream);
  sc_stream_t st = (sc_stream_t)stream;
  GridArgs a;
  gno_grid_args(d, data, queries, ws, &a);
  a.E = n_edges;
  a.splits = (const long long*)row_splits;
  a.index = (long long*)index;
  a.weights = d->return_norm ? weights : nullptr;
  a.nb = (int)(d->m < 512 ? d->m : 512);
  SC_LAUNCH(k_fill_i32, dim3(1), dim3(256), 0, st, &a.head->nlong, (long long)1, 0);
  if (int e = sc_check_launch("k_fill_i32")) return e;
  gno_grid_query_launch<true>(d->d, a, st);
  if (int e = sc_check_launch("k_grid_query (fill)")) return e;
  GNO_GRID_LAUNCH_D(k_grid_order_long, d->d, dim3((unsigned)a.nb), st, a);
  return sc_check_launch("k_grid_order_long");
}
