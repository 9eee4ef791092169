// sc_host_fdconv.h -- host side of the finite-difference convolution entry points (kernels: sc_kernels_fdconv.h).
// Every entry point refuses a bad descriptor before any launch.  The route is a function of the descriptor alone
// (sc_fdconv_path), and so are the chunk counts of the weight gradient: the same call gives the same bits anywhere.
#pragma once
#include "sc_host_common.h"
#include "sc_kernels_fdconv.h"

#define FD_MAX_ELEMS ((int64_t)1 << 40)
#define FD_MAX_GRID (((int64_t)1 << 31) - 1)

struct FdPlan {
  int nd, k, r, mode, groups, path;
  int d[3];                    // internal extents, missing leading axes 1
  int kk[3], rr[3];            // taps / halo per internal axis
  int64_t batch, c_in, c_out;
  int64_t taps, wn;            // taps per (o, c); floats of one weight copy
  int64_t chunks, parts;       // weight gradient: workgroups per (o, c) job, partial sums per weight entry
  int64_t pad_img;             // points of one padded image (replicate / reflect data gradient), else 0
  float inv_h;
};

static bool fd_mfma_channels(const int64_t c) { return c == 32 || c == 64 || c == 128; }

static int fd_plan(const sc_fdconv_desc* d, FdPlan* p) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->ndim >= 1 && d->ndim <= 3, "fdconv: 1 to 3 spatial dimensions");
  SC_CHECK_ARG(d->k % 2 == 1, "fdconv: the kernel size must be odd");
  SC_CHECK_ARG(d->k >= 3 && d->k <= 7, "fdconv: kernel sizes 3, 5 and 7");
  SC_CHECK_ARG(d->padding >= SC_FDCONV_PERIODIC && d->padding <= SC_FDCONV_REFLECT, "fdconv: unknown padding mode");
  SC_CHECK_ARG(d->batch >= 1 && d->c_in >= 1 && d->c_out >= 1, "fdconv: batch and channel counts must be positive");
  SC_CHECK_ARG(d->groups >= 1 && d->c_in % d->groups == 0 && d->c_out % d->groups == 0,
               "fdconv: groups must divide both channel counts");
  SC_CHECK_ARG(d->inv_h == d->inv_h, "fdconv: 1 / grid_width is not a number");
  std::memset(p, 0, sizeof(*p));
  p->nd = d->ndim;
  p->k = d->k;
  p->r = d->k / 2;
  p->mode = d->padding;
  p->groups = d->groups;
  p->batch = d->batch;
  p->c_in = d->c_in;
  p->c_out = d->c_out;
  p->inv_h = d->inv_h;
  int64_t pts = 1, ppts = 1;
  p->taps = 1;
  for (int i = 0; i < 3; ++i) {
    p->d[i] = 1;
    p->kk[i] = 1;
  }
  for (int i = 0; i < d->ndim; ++i) {
    const int64_t n = d->dims[i];
    SC_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 30), "fdconv: extent out of range");
    SC_CHECK_ARG(d->padding != SC_FDCONV_REFLECT || n > p->r, "fdconv: reflect padding needs extents above k / 2");
    SC_CHECK_ARG(d->padding != SC_FDCONV_PERIODIC || n >= p->r, "fdconv: periodic padding needs extents of at least k / 2");
    const int ax = 3 - d->ndim + i;
    p->d[ax] = (int)n;
    p->kk[ax] = p->k;
    p->rr[ax] = p->r;
    p->taps *= p->k;
    pts *= n;
    ppts *= n + 2 * p->r;
    SC_CHECK_ARG(ppts < FD_MAX_ELEMS, "fdconv: too many points");
  }
  const int64_t cmax = d->c_in > d->c_out ? d->c_in : d->c_out;
  SC_CHECK_ARG(cmax < ((int64_t)1 << 20) && d->batch < ((int64_t)1 << 30) && d->batch * cmax * ppts < FD_MAX_ELEMS,
               "fdconv: tensor too large");
  p->wn = d->c_out * (d->c_in / d->groups) * p->taps;
  SC_CHECK_ARG(p->wn < ((int64_t)1 << 31), "fdconv: weight too large");
  const bool dense = d->ndim == 2 && d->k == 3 && d->groups == 1 && fd_mfma_channels(d->c_in) &&
                     fd_mfma_channels(d->c_out) &&
                     (d->padding == SC_FDCONV_PERIODIC || d->padding == SC_FDCONV_ZEROS);
  p->path = dense ? SC_FDCONV_PATH_MFMA : SC_FDCONV_PATH_GENERAL;
  const bool padded_grad = d->padding == SC_FDCONV_REPLICATE || d->padding == SC_FDCONV_REFLECT;
  p->pad_img = padded_grad ? ppts : 0;
  // launches: every grid below 2^31 workgroups
  const int64_t tr = dense ? FDM_TR : FD_TR, tc = dense ? FDM_TC : FD_TC;
  const int ext = padded_grad ? p->r : 0;                    // the largest output any launch tiles
  const int64_t tiles = ((p->d[1] + 2 * (p->nd >= 2 ? ext : 0) + tr - 1) / tr) * ((p->d[2] + 2 * ext + tc - 1) / tc);
  const int64_t planes = p->d[0] + 2 * (p->nd == 3 ? ext : 0);
  SC_CHECK_ARG(d->batch * cmax * planes * tiles < FD_MAX_GRID, "fdconv: too many workgroups for one launch");
  const int64_t units = d->batch * (dense ? 1 : p->d[0]) * (((p->d[1] + tr - 1) / tr) * ((p->d[2] + tc - 1) / tc));
  // the general route has one job per (o, c, first-axis tap): split each into chunks only until about 1024 workgroups
  const int64_t jobs = d->c_out * (d->c_in / d->groups) * p->kk[0];
  const int64_t want = dense ? 64 : (jobs >= 1024 ? 1 : (1024 / jobs < 32 ? 1024 / jobs : 32));
  p->chunks = units < want ? units : want;
  p->parts = dense ? 4 * p->chunks : p->chunks;
  SC_CHECK_ARG(p->wn * p->kk[0] * p->chunks < FD_MAX_GRID, "fdconv: too many workgroups for one launch");
  return 0;
}

// floats: W' | W' flipped and transposed | their round-major copies (matrix-core route) | weight-gradient partials |
// padded data gradient
static int64_t fd_wcopies(const FdPlan& p) { return p.path == SC_FDCONV_PATH_MFMA ? 4 : 2; }
static size_t fd_ws_floats(const FdPlan& p) {
  return (size_t)(fd_wcopies(p) * p.wn + p.parts * p.wn + p.batch * p.c_in * p.pad_img);
}

extern "C" int sc_fdconv_path(const sc_fdconv_desc* d) {
  FdPlan p;
  if (fd_plan(d, &p)) return 0;
  return p.path;
}

extern "C" size_t sc_fdconv_workspace_bytes(const sc_fdconv_desc* d) {
  FdPlan p;
  if (fd_plan(d, &p)) return 0;
  return fd_ws_floats(p) * sizeof(float);
}

// the forward call reads the folded weights only
extern "C" size_t sc_fdconv_forward_workspace_bytes(const sc_fdconv_desc* d) {
  FdPlan p;
  if (fd_plan(d, &p)) return 0;
  return (size_t)(fd_wcopies(p) * p.wn) * sizeof(float);
}

static void fd_geom(const FdPlan& p, const int mode, const int ext, const int tr, const int tc, FdGeom* g) {
  std::memset(g, 0, sizeof(*g));
  g->d0 = p.d[0];
  g->d1 = p.d[1];
  g->d2 = p.d[2];
  g->k0 = p.kk[0];
  g->k1 = p.kk[1];
  g->k2 = p.kk[2];
  g->r0 = p.rr[0];
  g->r1 = p.rr[1];
  g->r2 = p.rr[2];
  g->e0 = p.rr[0] ? ext : 0;
  g->e1 = p.rr[1] ? ext : 0;
  g->e2 = p.rr[2] ? ext : 0;
  g->o0 = g->d0 + 2 * g->e0;
  g->o1 = g->d1 + 2 * g->e1;
  g->o2 = g->d2 + 2 * g->e2;
  g->mode = mode;
  g->tiles_r = (g->o1 + tr - 1) / tr;
  g->tiles_c = (g->o2 + tc - 1) / tc;
}

static int fd_fold(const FdPlan& p, const float* w, float* ws, sc_stream_t st) {
  const int64_t n = p.c_out * (p.c_in / p.groups);
  const bool mx = p.path == SC_FDCONV_PATH_MFMA;
  SC_LAUNCH(k_fdconv_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, ws, ws + p.wn,
            mx ? ws + 2 * p.wn : (float*)nullptr, mx ? ws + 3 * p.wn : (float*)nullptr, (int)p.c_out,
            (int)(p.c_in / p.groups), (int)(p.c_out / p.groups), (int)p.taps, p.inv_h);
  return sc_check_launch("k_fdconv_fold");
}

// y = conv(pad(x), w) with c_in -> c_out channels of this call; ext > 0: the full correlation, zeros outside x
static int fd_conv(const FdPlan& p, const int path, const int mode, const int ext, const int64_t c_in,
                   const int64_t c_out, const float* x, const float* w, float* y, sc_stream_t st) {
  FdArgs a;
  std::memset(&a, 0, sizeof(a));
  a.c_in = (int)c_in;
  a.c_out = (int)c_out;
  a.groups = p.groups;
  if (path == SC_FDCONV_PATH_MFMA) {
    fd_geom(p, mode, 0, FDM_TR, FDM_TC, &a.g);
    const dim3 grid((unsigned)(p.batch * a.g.tiles_r * a.g.tiles_c));
    if (c_out == 32) SC_LAUNCH(k_fdconv_mfma<1>, grid, dim3(256), 0, st, x, w, y, a);
    else if (c_out == 64) SC_LAUNCH(k_fdconv_mfma<2>, grid, dim3(256), 0, st, x, w, y, a);
    else SC_LAUNCH(k_fdconv_mfma<4>, grid, dim3(256), 0, st, x, w, y, a);
    return sc_check_launch("k_fdconv_mfma");
  }
  fd_geom(p, mode, ext, FD_TR, FD_TC, &a.g);
  const int64_t cout_g = c_out / p.groups;
  a.n_oblk = (int)((cout_g + FD_OCB - 1) / FD_OCB);
  const dim3 grid((unsigned)(p.batch * p.groups * a.n_oblk * a.g.o0 * a.g.tiles_r * a.g.tiles_c));
  if (p.nd == 1) SC_LAUNCH(k_fdconv<1>, grid, dim3(256), 0, st, x, w, y, a);
  else if (p.nd == 2) SC_LAUNCH(k_fdconv<2>, grid, dim3(256), 0, st, x, w, y, a);
  else SC_LAUNCH(k_fdconv<3>, grid, dim3(256), 0, st, x, w, y, a);
  return sc_check_launch("k_fdconv");
}

extern "C" int sc_fdconv_forward(const sc_fdconv_desc* d, const float* x, const float* w, float* y, void* ws,
                                 size_t ws_bytes, void* stream) {
  FdPlan p;
  if (int e = fd_plan(d, &p)) return e;
  SC_CHECK_ARG(x && w && y && ws, "null argument");
  SC_CHECK_ARG(ws_bytes >= (size_t)(fd_wcopies(p) * p.wn) * sizeof(float), "fdconv: workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  float* wf = (float*)ws;
  if (int e = fd_fold(p, w, wf, st)) return e;
  return fd_conv(p, p.path, p.mode, 0, p.c_in, p.c_out, x, p.path == SC_FDCONV_PATH_MFMA ? wf + 2 * p.wn : wf, y, st);
}

extern "C" int sc_fdconv_backward(const sc_fdconv_desc* d, const float* x, const float* w, const float* gout, float* gx,
                                  float* gw, void* ws, size_t ws_bytes, void* stream) {
  FdPlan p;
  if (int e = fd_plan(d, &p)) return e;
  SC_CHECK_ARG(gx || gw, "fdconv: neither gradient is wanted");
  SC_CHECK_ARG(gout && ws && (w || !gx) && (x || !gw), "null argument");
  SC_CHECK_ARG(ws_bytes >= fd_ws_floats(p) * sizeof(float), "fdconv: workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  float* wf = (float*)ws;
  float* wt = wf + p.wn;
  float* parts = wf + fd_wcopies(p) * p.wn;
  float* gpad = parts + p.parts * p.wn;
  if (gx) {
    if (int e = fd_fold(p, w, wf, st)) return e;
    if (p.pad_img) {                                         // replicate / reflect: padded domain, then the pre-images
      if (int e = fd_conv(p, SC_FDCONV_PATH_GENERAL, FD_ZEROS, p.r, p.c_out, p.c_in, gout, wt, gpad, st)) return e;
      FdGeom g;
      fd_geom(p, p.mode, 0, FD_TR, FD_TC, &g);
      const int64_t lines = p.batch * p.c_in, n = lines * g.d0 * g.d1 * g.d2;
      SC_LAUNCH(k_fdconv_unpad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)gpad, gx, g,
                (long long)lines);
      if (int e = sc_check_launch("k_fdconv_unpad")) return e;
    } else {
      if (int e = fd_conv(p, p.path, p.mode, 0, p.c_out, p.c_in, gout, p.path == SC_FDCONV_PATH_MFMA ? wf + 3 * p.wn : wt,
                          gx, st))
        return e;
    }
  }
  if (gw) {
    FdWgArgs a;
    std::memset(&a, 0, sizeof(a));
    a.batch = (int)p.batch;
    a.c_in = (int)p.c_in;
    a.c_out = (int)p.c_out;
    a.groups = p.groups;
    a.chunks = (int)p.chunks;
    if (p.path == SC_FDCONV_PATH_MFMA) {
      fd_geom(p, p.mode, 0, FDM_TR, FDM_TC, &a.g);
      a.units = p.batch * a.g.tiles_r * a.g.tiles_c;
      a.per_chunk = (a.units + a.chunks - 1) / a.chunks;
      const dim3 grid((unsigned)((p.c_out / 32) * (p.c_in / 32) * p.chunks));
      SC_LAUNCH(k_fdconv_wgrad_mfma, grid, dim3(256), 0, st, x, gout, parts, a);
      if (int e = sc_check_launch("k_fdconv_wgrad_mfma")) return e;
    } else {
      fd_geom(p, p.mode, 0, FD_TR, FD_TC, &a.g);
      a.units = p.batch * a.g.d0 * a.g.tiles_r * a.g.tiles_c;
      a.per_chunk = (a.units + a.chunks - 1) / a.chunks;
      const dim3 grid((unsigned)(p.c_out * (p.c_in / p.groups) * a.g.k0 * p.chunks));
      if (p.k == 3) SC_LAUNCH(k_fdconv_wgrad<3>, grid, dim3(256), 0, st, x, gout, parts, a);
      else if (p.k == 5) SC_LAUNCH(k_fdconv_wgrad<5>, grid, dim3(256), 0, st, x, gout, parts, a);
      else SC_LAUNCH(k_fdconv_wgrad<7>, grid, dim3(256), 0, st, x, gout, parts, a);
      if (int e = sc_check_launch("k_fdconv_wgrad")) return e;
    }
    SC_LAUNCH(k_fdconv_wreduce, dim3((unsigned)((p.wn + 255) / 256)), dim3(256), 0, st, (const float*)parts, gw,
              (long long)p.wn, (int)p.taps, (int)p.parts, p.inv_h);
    if (int e = sc_check_launch("k_fdconv_wreduce")) return e;
  }
  return 0;
}
