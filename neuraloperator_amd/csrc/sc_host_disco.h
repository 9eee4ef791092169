// sc_host_disco.h -- host side of the equidistant discrete-continuous convolution entry points (kernels:
// sc_kernels_disco.h).  Every entry point refuses a bad descriptor before any launch.  The route is a function of the
// descriptor alone (sc_disco_path), and so are the chunk counts of the weight gradient: the same call gives the same
// bits anywhere.
#pragma once
#include <cmath>

#include "sc_host_common.h"
#include "sc_host_fdconv.h"
#include "sc_kernels_disco.h"

struct DcPlan {
  int path, transposed, groups, nk;
  int hf, wf, hc, wc;          // fine / coarse grid of the underlying correlation
  int ph, pw, sh, sw, padh, padw, tr;
  int64_t batch, cc_in, cc_out;  // channels on the fine / coarse grid
  int64_t c_out, out_pts;      // of the layer's output (bias, gbias)
  int64_t taps, wn, nw;        // taps per (o, c); floats of one folded copy; weight entries
  int64_t chunks, parts;
  float q;
};

static int dc_plan(const sc_disco_desc* d, DcPlan* p) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->transposed == 0 || d->transposed == 1, "disco: transposed is 0 or 1");
  SC_CHECK_ARG(d->batch >= 1 && d->c_in >= 1 && d->c_out >= 1, "disco: batch and channel counts must be positive");
  SC_CHECK_ARG(d->groups >= 1 && d->c_in % d->groups == 0 && d->c_out % d->groups == 0,
               "disco: groups must divide both channel counts");
  SC_CHECK_ARG(d->basis >= 1 && d->basis <= 4096, "disco: 1 to 4096 basis functions");
  SC_CHECK_ARG(d->ph >= 1 && d->ph <= DC_MAX_P && d->pw >= 1 && d->pw <= DC_MAX_P, "disco: support 1 to 15 per axis");
  SC_CHECK_ARG(d->sh >= 1 && d->sh <= DC_MAX_S && d->sw >= 1 && d->sw <= DC_MAX_S, "disco: stride 1 to 4 per axis");
  SC_CHECK_ARG(d->pad_h >= 0 && d->pad_h < d->ph && d->pad_w >= 0 && d->pad_w < d->pw,
               "disco: padding from 0 to support - 1");
  SC_CHECK_ARG(std::isfinite(d->q_weight), "disco: the quadrature weight is not finite");
  const int64_t lim = (int64_t)1 << 30;
  SC_CHECK_ARG(d->h_in >= 1 && d->h_in < lim && d->w_in >= 1 && d->w_in < lim && d->h_out >= 1 && d->h_out < lim &&
                   d->w_out >= 1 && d->w_out < lim,
               "disco: extent out of range");
  if (d->transposed) {
    SC_CHECK_ARG(d->opad_h >= 0 && d->opad_h < d->sh && d->opad_w >= 0 && d->opad_w < d->sw,
                 "disco: output padding from 0 to stride - 1");
    SC_CHECK_ARG(d->h_out == (d->h_in - 1) * d->sh - 2 * d->pad_h + d->ph + d->opad_h &&
                     d->w_out == (d->w_in - 1) * d->sw - 2 * d->pad_w + d->pw + d->opad_w,
                 "disco: output extents do not follow from input, support, stride and padding");
  } else {
    SC_CHECK_ARG(d->opad_h == 0 && d->opad_w == 0, "disco: output padding belongs to the transposed form");
    SC_CHECK_ARG(d->h_in + 2 * d->pad_h >= d->ph && d->w_in + 2 * d->pad_w >= d->pw,
                 "disco: the support is larger than the padded input");
    SC_CHECK_ARG(d->h_out == (d->h_in + 2 * d->pad_h - d->ph) / d->sh + 1 &&
                     d->w_out == (d->w_in + 2 * d->pad_w - d->pw) / d->sw + 1,
                 "disco: output extents do not follow from input, support, stride and padding");
  }
  std::memset(p, 0, sizeof(*p));
  p->transposed = d->transposed;
  p->groups = d->groups;
  p->nk = d->basis;
  p->hf = (int)(d->transposed ? d->h_out : d->h_in);
  p->wf = (int)(d->transposed ? d->w_out : d->w_in);
  p->hc = (int)(d->transposed ? d->h_in : d->h_out);
  p->wc = (int)(d->transposed ? d->w_in : d->w_out);
  p->ph = d->ph;
  p->pw = d->pw;
  p->sh = d->sh;
  p->sw = d->sw;
  p->padh = d->pad_h;
  p->padw = d->pad_w;
  p->tr = d->sh == 1 ? 16 : (d->sh == 2 ? 8 : 4);
  p->batch = d->batch;
  p->cc_in = d->transposed ? d->c_out : d->c_in;
  p->cc_out = d->transposed ? d->c_in : d->c_out;
  p->c_out = d->c_out;
  p->out_pts = d->h_out * d->w_out;
  p->q = d->q_weight;
  p->taps = (int64_t)d->ph * d->pw;
  const int64_t cmax = d->c_in > d->c_out ? d->c_in : d->c_out;
  const int64_t fpts = (int64_t)p->hf * p->wf;
  SC_CHECK_ARG(fpts < FD_MAX_ELEMS / 4 && cmax < ((int64_t)1 << 20) && d->batch < lim &&
                   d->batch * cmax * (fpts + 4 * (int64_t)DC_MAX_P * (p->hf + p->wf + DC_MAX_P)) < FD_MAX_ELEMS,
               "disco: tensor too large");
  const int64_t pairs = p->cc_out * (p->cc_in / p->groups);
  p->wn = pairs * p->taps;
  p->nw = pairs * p->nk;
  SC_CHECK_ARG(p->wn < ((int64_t)1 << 31) && p->nw < ((int64_t)1 << 31), "disco: weight too large");
  const bool dense = d->sh == 1 && d->sw == 1 && d->ph == 3 && d->pw == 3 && d->pad_h == 1 && d->pad_w == 1 &&
                     d->groups == 1 && fd_mfma_channels(d->c_in) && fd_mfma_channels(d->c_out);
  p->path = dense ? SC_DISCO_PATH_MFMA : SC_DISCO_PATH_GENERAL;
  // launches: every grid below 2^31 workgroups
  const int64_t ctiles = dense ? (int64_t)((p->hc + FDM_TR - 1) / FDM_TR) * ((p->wc + FDM_TC - 1) / FDM_TC)
                               : (int64_t)((p->hc + p->tr - 1) / p->tr) * ((p->wc + DC_TC - 1) / DC_TC);
  const int64_t ftiles = dense ? ctiles : (int64_t)((p->hf + DT_TR - 1) / DT_TR) * ((p->wf + DC_TC - 1) / DC_TC);
  SC_CHECK_ARG(d->batch * cmax * (ctiles > ftiles ? ctiles : ftiles) < FD_MAX_GRID,
               "disco: too many workgroups for one launch");
  const int64_t units = d->batch * ctiles;
  const int64_t jobs = pairs * p->ph;
  const int64_t want = dense ? 64 : (jobs >= 1024 ? 1 : (1024 / jobs < 32 ? 1024 / jobs : 32));
  p->chunks = units < want ? units : want;
  p->parts = dense ? 4 * p->chunks : p->chunks;
  SC_CHECK_ARG(jobs * p->chunks < FD_MAX_GRID && p->nw / 256 + d->c_out + 1 < FD_MAX_GRID,
               "disco: too many workgroups for one launch");
  return 0;
}

// floats: kernel | kernel flipped and transposed | their round-major copies (matrix-core route) | weight-gradient partials
static int64_t dc_wcopies(const DcPlan& p) { return p.path == SC_DISCO_PATH_MFMA ? 4 : 2; }
static size_t dc_fwd_floats(const DcPlan& p) { return (size_t)(dc_wcopies(p) * p.wn); }
static size_t dc_ws_floats(const DcPlan& p) { return (size_t)(dc_wcopies(p) * p.wn + p.parts * p.wn); }

extern "C" int sc_disco_path(const sc_disco_desc* d) {
  DcPlan p;
  if (dc_plan(d, &p)) return 0;
  return p.path;
}

extern "C" size_t sc_disco_workspace_bytes(const sc_disco_desc* d) {
  DcPlan p;
  if (dc_plan(d, &p)) return 0;
  return dc_ws_floats(p) * sizeof(float);
}

extern "C" size_t sc_disco_forward_workspace_bytes(const sc_disco_desc* d) {
  DcPlan p;
  if (dc_plan(d, &p)) return 0;
  return dc_fwd_floats(p) * sizeof(float);
}

static void dc_geom(const DcPlan& p, const bool fine_tiles, DcGeom* g) {
  std::memset(g, 0, sizeof(*g));
  g->hf = p.hf;
  g->wf = p.wf;
  g->hc = p.hc;
  g->wc = p.wc;
  g->ph = p.ph;
  g->pw = p.pw;
  g->sh = p.sh;
  g->sw = p.sw;
  g->padh = p.padh;
  g->padw = p.padw;
  g->tr = p.tr;
  g->tiles_r = fine_tiles ? (p.hf + DT_TR - 1) / DT_TR : (p.hc + p.tr - 1) / p.tr;
  g->tiles_c = ((fine_tiles ? p.wf : p.wc) + DC_TC - 1) / DC_TC;
}

static int dc_fold(const DcPlan& p, const float* w, const float* psi, float* ws, sc_stream_t st) {
  const int64_t n = p.cc_out * (p.cc_in / p.groups);
  const bool mx = p.path == SC_DISCO_PATH_MFMA;
  SC_LAUNCH(k_disco_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, psi, ws, ws + p.wn,
            mx ? ws + 2 * p.wn : (float*)nullptr, mx ? ws + 3 * p.wn : (float*)nullptr, (int)p.cc_out,
            (int)(p.cc_in / p.groups), (int)(p.cc_out / p.groups), p.nk, (int)p.taps, p.q);
  return sc_check_launch("k_disco_fold");
}

// coarse = C(fine) (adjoint false) or fine = C^T(coarse); wf = the folded weights of dc_fold
static int dc_apply(const DcPlan& p, const bool adjoint, const float* in, const float* wf, const float* bias, float* out,
                    sc_stream_t st) {
  if (p.path == SC_DISCO_PATH_MFMA) {
    FdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.c_in = (int)(adjoint ? p.cc_out : p.cc_in);
    a.c_out = (int)(adjoint ? p.cc_in : p.cc_out);
    a.groups = 1;
    FdGeom& g = a.g;
    g.d0 = g.o0 = g.k0 = 1;
    g.d1 = g.o1 = p.hf;
    g.d2 = g.o2 = p.wf;
    g.k1 = g.k2 = 3;
    g.r1 = g.r2 = 1;
    g.mode = FD_ZEROS;
    g.tiles_r = (p.hf + FDM_TR - 1) / FDM_TR;
    g.tiles_c = (p.wf + FDM_TC - 1) / FDM_TC;
    const float* w = wf + (adjoint ? 3 : 2) * p.wn;
    const dim3 grid((unsigned)(p.batch * g.tiles_r * g.tiles_c));
    if (a.c_out == 32) SC_LAUNCH(k_disco_mfma<1>, grid, dim3(256), 0, st, in, w, bias, out, a);
    else if (a.c_out == 64) SC_LAUNCH(k_disco_mfma<2>, grid, dim3(256), 0, st, in, w, bias, out, a);
    else SC_LAUNCH(k_disco_mfma<4>, grid, dim3(256), 0, st, in, w, bias, out, a);
    return sc_check_launch("k_disco_mfma");
  }
  DcArgs a;
  std::memset(&a, 0, sizeof(a));
  dc_geom(p, adjoint, &a.g);
  a.cc_in = (int)p.cc_in;
  a.cc_out = (int)p.cc_out;
  a.groups = p.groups;
  const int64_t per_g = (adjoint ? p.cc_in : p.cc_out) / p.groups;
  a.n_blk = (int)((per_g + DC_OCB - 1) / DC_OCB);
  const dim3 grid((unsigned)(p.batch * p.groups * a.n_blk * a.g.tiles_r * a.g.tiles_c));
  if (adjoint) {
    SC_LAUNCH(k_disco_convT, grid, dim3(256), 0, st, in, wf + p.wn, bias, out, a);
    return sc_check_launch("k_disco_convT");
  }
  SC_LAUNCH(k_disco_conv, grid, dim3(256), 0, st, in, wf, bias, out, a);
  return sc_check_launch("k_disco_conv");
}

extern "C" int sc_disco_forward(const sc_disco_desc* d, const float* x, const float* w, const float* psi,
                                const float* bias, float* y, void* ws, size_t ws_bytes, void* stream) {
  DcPlan p;
  if (int e = dc_plan(d, &p)) return e;
  SC_CHECK_ARG(x && w && psi && y && ws, "null argument");
  SC_CHECK_ARG(ws_bytes >= dc_fwd_floats(p) * sizeof(float), "disco: workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  float* wf = (float*)ws;
  if (int e = dc_fold(p, w, psi, wf, st)) return e;
  return dc_apply(p, p.transposed != 0, x, wf, bias, y, st);
}

extern "C" int sc_disco_backward(const sc_disco_desc* d, const float* x, const float* w, const float* psi,
                                 const float* gout, float* gx, float* gw, float* gbias, void* ws, size_t ws_bytes,
                                 void* stream) {
  DcPlan p;
  if (int e = dc_plan(d, &p)) return e;
  SC_CHECK_ARG(gx || gw || gbias, "disco: no gradient is wanted");
  SC_CHECK_ARG(gout && (!gx || (w && psi)) && (!gw || (x && psi)) && (ws || !(gx || gw)), "null argument");
  SC_CHECK_ARG(!(gx || gw) || ws_bytes >= dc_ws_floats(p) * sizeof(float), "disco: workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  float* wf = (float*)ws;
  float* parts = wf ? wf + dc_wcopies(p) * p.wn : nullptr;
  if (gx) {
    if (int e = dc_fold(p, w, psi, wf, st)) return e;
    if (int e = dc_apply(p, p.transposed == 0, gout, wf, nullptr, gx, st)) return e;
  }
  if (gw) {
    const float* fine = p.transposed ? gout : x;
    const float* coarse = p.transposed ? x : gout;
    if (p.path == SC_DISCO_PATH_MFMA) {
      FdWgArgs a;
      std::memset(&a, 0, sizeof(a));
      FdGeom& g = a.g;
      g.d0 = g.o0 = g.k0 = 1;
      g.d1 = g.o1 = p.hf;
      g.d2 = g.o2 = p.wf;
      g.k1 = g.k2 = 3;
      g.r1 = g.r2 = 1;
      g.mode = FD_ZEROS;
      g.tiles_r = (p.hf + FDM_TR - 1) / FDM_TR;
      g.tiles_c = (p.wf + FDM_TC - 1) / FDM_TC;
      a.batch = (int)p.batch;
      a.c_in = (int)p.cc_in;
      a.c_out = (int)p.cc_out;
      a.groups = 1;
      a.chunks = (int)p.chunks;
      a.units = p.batch * g.tiles_r * g.tiles_c;
      a.per_chunk = (a.units + a.chunks - 1) / a.chunks;
      const dim3 grid((unsigned)((p.cc_out / 32) * (p.cc_in / 32) * p.chunks));
      SC_LAUNCH(k_fdconv_wgrad_mfma, grid, dim3(256), 0, st, fine, coarse, parts, a);
      if (int e = sc_check_launch("k_fdconv_wgrad_mfma")) return e;
    } else {
      DcWgArgs a;
      std::memset(&a, 0, sizeof(a));
      dc_geom(p, false, &a.g);
      a.batch = (int)p.batch;
      a.cc_in = (int)p.cc_in;
      a.cc_out = (int)p.cc_out;
      a.groups = p.groups;
      a.chunks = (int)p.chunks;
      a.units = p.batch * a.g.tiles_r * a.g.tiles_c;
      a.per_chunk = (a.units + a.chunks - 1) / a.chunks;
      const dim3 grid((unsigned)(p.cc_out * (p.cc_in / p.groups) * p.ph * p.chunks));
      SC_LAUNCH(k_disco_wgrad, grid, dim3(256), 0, st, fine, coarse, parts, a);
      if (int e = sc_check_launch("k_disco_wgrad")) return e;
    }
  }
  if (gw && p.parts > 1) {
    SC_LAUNCH(k_disco_psum, dim3((unsigned)((p.wn + 255) / 256)), dim3(256), 0, st, parts, (long long)p.wn, (int)p.parts);
    if (int e = sc_check_launch("k_disco_psum")) return e;
  }
  if (gw || gbias) {
    const int w_blocks = gw ? (int)((p.nw + 255) / 256) : 0;
    SC_LAUNCH(k_disco_wreduce, dim3((unsigned)(w_blocks + (gbias ? p.c_out : 0))), dim3(256), 0, st,
              (const float*)parts, psi, gout, gw, gbias, (long long)p.nw, p.nk, (int)p.taps, 1, p.q,
              w_blocks, (int)p.batch, (int)p.c_out, (long long)p.out_pts);
    if (int e = sc_check_launch("k_disco_wreduce")) return e;
  }
  return 0;
}
