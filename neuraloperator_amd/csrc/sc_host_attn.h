// sc_host_attn.h -- host side of the attention kernel integral (kernels: sc_kernels_attn.h).  Every entry point refuses
// a bad descriptor before any launch; nothing here reads device memory or waits for the device, so a step records into a
// graph.  The chunking of the D x D sums is a function of the descriptor alone: the same call gives the same bits
// anywhere.
#pragma once
#include "sc_host_common.h"
#include "sc_kernels_attn.h"

#define ATT_MAX_I32 (((int64_t)1 << 31) - 1)

struct AttPlan {
  int64_t batch, n_src, n_qry, bh, dd;     // bh = batch heads, dd = D D
  int64_t chunks_src, chunks_qry;
  int heads, D, DP, rotary, has_weights, path;
};

static int att_plan(const sc_attn_desc* d, AttPlan* p) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->batch >= 1 && d->heads >= 1 && d->n_src >= 1 && d->n_qry >= 1,
               "attn: batch, heads and point counts must be positive");
  SC_CHECK_ARG(d->head_dim >= 2 && d->head_dim <= 128 && d->head_dim % 2 == 0,
               "attn: head_dim must be even and within 2 to 128");
  SC_CHECK_ARG(d->rotary >= 0 && d->rotary <= 2, "attn: rotary is 0 (none), 1 or 2 position dimensions");
  SC_CHECK_ARG(d->rotary != 2 || d->head_dim % 4 == 0, "attn: the 2-d rotary embedding needs head_dim % 4 == 0");
  SC_CHECK_ARG(d->has_weights == 0 || d->has_weights == 1, "attn: has_weights is 0 or 1");
  SC_CHECK_ARG(d->n_src <= ATT_MAX_I32 && d->n_qry <= ATT_MAX_I32 && d->batch <= ATT_MAX_I32 && d->heads <= ATT_MAX_I32,
               "attn: n_src and n_qry must fit 32-bit indices");
  const int64_t nmax = d->n_src > d->n_qry ? d->n_src : d->n_qry, hd = (int64_t)d->heads * d->head_dim;
  SC_CHECK_ARG(hd <= ATT_MAX_I32 && d->batch * d->heads < 65536 && nmax * hd <= ATT_MAX_I32 &&
                   d->batch * nmax <= ATT_MAX_I32 / hd,
               "attn: batch heads must stay below 65536 and batch n heads head_dim within 32-bit indices");
  std::memset(p, 0, sizeof(*p));
  p->batch = d->batch;
  p->n_src = d->n_src;
  p->n_qry = d->n_qry;
  p->heads = (int)d->heads;
  p->D = d->head_dim;
  p->DP = d->head_dim <= 32 ? 32 : (d->head_dim <= 64 ? 64 : 128);
  p->rotary = d->rotary;
  p->has_weights = d->has_weights;
  p->bh = d->batch * d->heads;
  p->dd = (int64_t)d->head_dim * d->head_dim;
  p->chunks_src = (d->n_src + ATT_CHUNK - 1) / ATT_CHUNK;
  p->chunks_qry = (d->n_qry + ATT_CHUNK - 1) / ATT_CHUNK;
  p->path = d->head_dim == 32 || d->head_dim == 64 || d->head_dim == 128 ? SC_ATTN_PATH_MFMA : SC_ATTN_PATH_VECTOR;
  return 0;
}

// floats of the workspace: parts | dots^T | g_dots | g_dots^T (the forward call uses the partials alone)
static size_t att_fwd_floats(const AttPlan& p) { return (size_t)(p.bh * p.chunks_src * p.dd); }
static size_t att_ws_floats(const AttPlan& p) {
  const int64_t c = p.chunks_src > p.chunks_qry ? p.chunks_src : p.chunks_qry;
  return (size_t)(p.bh * c * p.dd + 3 * p.bh * p.dd);
}

extern "C" int sc_attn_path(const sc_attn_desc* d) {
  AttPlan p;
  if (att_plan(d, &p)) return 0;
  return p.path;
}

extern "C" size_t sc_attn_workspace_bytes(const sc_attn_desc* d) {
  AttPlan p;
  if (att_plan(d, &p)) return 0;
  return att_ws_floats(p) * sizeof(float);
}

static AttGeom att_geom(const AttPlan& p, const int64_t n, const float rot_scale) {
  AttGeom g;
  g.n = (int)n;
  g.heads = p.heads;
  g.D = p.D;
  g.rotary = p.rotary;
  g.rot_scale = rot_scale;
  g.wconst = 1.f / (float)p.n_src;
  return g;
}

// points of a tile of the per-point kernels: 32 on the vector route, 128 (64 at D = 128) on the matrix-core route
static int att_tile_points(const AttPlan& p) { return p.path == SC_ATTN_PATH_MFMA ? ATT_MTP(p.DP) : 32; }

template <typename KM, typename KV, typename A>
static void att_launch2(KM km, KV kv, const bool mf, const dim3 grid, sc_stream_t st, const A& a) {
  if (mf) SC_LAUNCH(km, grid, dim3(256), 0, st, a);
  else SC_LAUNCH(kv, grid, dim3(256), 0, st, a);
}

static int att_outer(const AttPlan& p, const AttOuterArgs& a, sc_stream_t st) {
  const dim3 grid((unsigned)a.chunks, (unsigned)p.bh);
  const bool mf = p.path == SC_ATTN_PATH_MFMA;
  if (p.DP == 32) att_launch2(k_attn_outer<32, true>, k_attn_outer<32, false>, mf, grid, st, a);
  else if (p.DP == 64) att_launch2(k_attn_outer<64, true>, k_attn_outer<64, false>, mf, grid, st, a);
  else att_launch2(k_attn_outer<128, true>, k_attn_outer<128, false>, mf, grid, st, a);
  return sc_check_launch("k_attn_outer");
}

static int att_reduce(const AttPlan& p, const float* parts, float* M, float* MT, const int64_t chunks, sc_stream_t st) {
  const int64_t total = p.bh * p.dd;
  SC_LAUNCH(k_attn_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, parts, M, MT, p.D, (int)chunks,
            (long long)total);
  return sc_check_launch("k_attn_reduce");
}

static int att_apply_launch(const AttPlan& p, const AttApplyArgs& a, sc_stream_t st) {
  const bool mf = p.path == SC_ATTN_PATH_MFMA;
  const int tp = att_tile_points(p);
  const dim3 grid((unsigned)((a.g.n + tp - 1) / tp), (unsigned)p.bh);
  if (p.DP == 32) att_launch2(k_attn_apply<32, true>, k_attn_apply<32, false>, mf, grid, st, a);
  else if (p.DP == 64) att_launch2(k_attn_apply<64, true>, k_attn_apply<64, false>, mf, grid, st, a);
  else att_launch2(k_attn_apply<128, true>, k_attn_apply<128, false>, mf, grid, st, a);
  return sc_check_launch("k_attn_apply");
}

extern "C" int sc_attn_forward(const sc_attn_desc* d, const float* q, const float* k, const float* v,
                               const float* pos_src, const float* pos_qry, const float* inv_freq, float rot_scale,
                               const float* weights, float* u, float* dots, void* ws, size_t ws_bytes, void* stream) {
  AttPlan p;
  if (int e = att_plan(d, &p)) return e;
  SC_CHECK_ARG(q && k && v && u && dots && ws, "null argument");
  SC_CHECK_ARG(!p.rotary || (pos_src && pos_qry && inv_freq), "attn: a rotary descriptor needs positions and inv_freq");
  SC_CHECK_ARG(!p.has_weights || weights, "attn: the descriptor announces weights");
  SC_CHECK_ARG(ws_bytes >= att_fwd_floats(p) * sizeof(float), "attn: workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  float* parts = (float*)ws;
  AttOuterArgs o;
  std::memset(&o, 0, sizeof(o));
  o.a = k;
  o.b = v;
  o.pos = p.rotary ? pos_src : nullptr;
  o.inv_freq = inv_freq;
  o.parts = parts;
  o.g = att_geom(p, p.n_src, rot_scale);
  o.chunks = (int)p.chunks_src;
  o.mode = 0;
  if (int e = att_outer(p, o, st)) return e;
  if (int e = att_reduce(p, parts, dots, nullptr, p.chunks_src, st)) return e;
  AttApplyArgs a;
  std::memset(&a, 0, sizeof(a));
  a.x = q;
  a.M = dots;
  a.pos = p.rotary ? pos_qry : nullptr;
  a.inv_freq = inv_freq;
  a.weights = p.has_weights ? weights : nullptr;
  a.out = u;
  a.g = att_geom(p, p.n_qry, rot_scale);
  a.mode = 0;
  return att_apply_launch(p, a, st);
}

extern "C" int sc_attn_backward(const sc_attn_desc* d, const float* q, const float* k, const float* v,
                                const float* pos_src, const float* pos_qry, const float* inv_freq, float rot_scale,
                                const float* weights, const float* dots, const float* gu, float* gq, float* gk,
                                float* gv, void* ws, size_t ws_bytes, void* stream) {
  AttPlan p;
  if (int e = att_plan(d, &p)) return e;
  SC_CHECK_ARG(gq || gk || gv, "attn: no gradient is wanted");
  SC_CHECK_ARG(gu && ws && (dots || !gq) && ((q && k && v) || !(gk || gv)), "null argument");
  SC_CHECK_ARG(!p.rotary || (pos_qry && inv_freq && (pos_src || !(gk || gv))),
               "attn: a rotary descriptor needs positions and inv_freq");
  SC_CHECK_ARG(!p.has_weights || weights, "attn: the descriptor announces weights");
  SC_CHECK_ARG(ws_bytes >= att_ws_floats(p) * sizeof(float), "attn: workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  const int64_t cmax = p.chunks_src > p.chunks_qry ? p.chunks_src : p.chunks_qry;
  float* parts = (float*)ws;
  float* dots_t = parts + p.bh * cmax * p.dd;
  float* gd = dots_t + p.bh * p.dd;
  float* gd_t = gd + p.bh * p.dd;
  const float* w = p.has_weights ? weights : nullptr;
  if (gq) {
    const int64_t total = p.bh * p.dd;
    SC_LAUNCH(k_attn_transpose, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dots, dots_t, p.D,
              (long long)total);
    if (int e = sc_check_launch("k_attn_transpose")) return e;
    AttApplyArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = gu;
    a.M = dots_t;
    a.pos = p.rotary ? pos_qry : nullptr;
    a.inv_freq = inv_freq;
    a.weights = w;
    a.out = gq;
    a.g = att_geom(p, p.n_qry, rot_scale);
    a.mode = 1;
    if (int e = att_apply_launch(p, a, st)) return e;
  }
  if (gk || gv) {
    AttOuterArgs o;
    std::memset(&o, 0, sizeof(o));
    o.a = q;
    o.b = gu;
    o.pos = p.rotary ? pos_qry : nullptr;
    o.inv_freq = inv_freq;
    o.weights = w;
    o.parts = parts;
    o.g = att_geom(p, p.n_qry, rot_scale);
    o.chunks = (int)p.chunks_qry;
    o.mode = 1;
    if (int e = att_outer(p, o, st)) return e;
    if (int e = att_reduce(p, parts, gd, gd_t, p.chunks_qry, st)) return e;
    AttKvBwdArgs b;
    std::memset(&b, 0, sizeof(b));
    b.k = k;
    b.v = v;
    b.pos = p.rotary ? pos_src : nullptr;
    b.inv_freq = inv_freq;
    b.G = gd;
    b.GT = gd_t;
    b.gk = gk;
    b.gv = gv;
    b.g = att_geom(p, p.n_src, rot_scale);
    const bool mf = p.path == SC_ATTN_PATH_MFMA;
    const int tp = att_tile_points(p);
    const dim3 grid((unsigned)((p.n_src + tp - 1) / tp), (unsigned)p.bh);
    if (p.DP == 32) att_launch2(k_attn_kv_bwd_mfma<32>, k_attn_kv_bwd<32>, mf, grid, st, b);
    else if (p.DP == 64) att_launch2(k_attn_kv_bwd_mfma<64>, k_attn_kv_bwd<64>, mf, grid, st, b);
    else att_launch2(k_attn_kv_bwd_mfma<128>, k_attn_kv_bwd<128>, mf, grid, st, b);
    if (int e = sc_check_launch("k_attn_kv_bwd")) return e;
  }
  return 0;
}
