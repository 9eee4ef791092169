// sc_host_disco_sparse.h -- host side of the point-cloud discrete-continuous convolution (kernels:
// sc_kernels_disco_sparse.h).  Every entry point refuses a bad descriptor before any launch; nothing here reads device
// memory or waits for the device, so a step records into a graph.  The slice count of the weight gradient is a function
// of the descriptor alone: the same call gives the same bits anywhere.
#pragma once
#include "sc_host_common.h"
#include "sc_kernels_disco_sparse.h"

#define DSP_MAX_I32 (((int64_t)1 << 31) - 1)
#define DSP_MAX_ELEMS ((int64_t)1 << 40)

struct DspPlan {
  int64_t batch, c_in, c_out, n_in, n_out, nnz, rows;       // rows = n_out batch: rows of the contraction
  int64_t wn;                                                // floats of the weight
  int64_t slices, per_slice;                                 // weight gradient
  int groups, K, cg, og, path;
};

static bool dsp_mfma_channels(const int64_t c) { return c == 32 || c == 64 || c == 128; }

static int dsp_plan(const sc_dsparse_desc* d, DspPlan* p) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->batch >= 1 && d->c_in >= 1 && d->c_out >= 1, "dsparse: batch and channel counts must be positive");
  SC_CHECK_ARG(d->groups >= 1 && d->c_in % d->groups == 0 && d->c_out % d->groups == 0,
               "dsparse: groups must divide both channel counts");
  SC_CHECK_ARG(d->basis >= 1 && d->basis <= 4096, "dsparse: 1 to 4096 basis functions");
  SC_CHECK_ARG(d->n_in >= 1 && d->n_out >= 1 && d->nnz >= 0, "dsparse: point and entry counts out of range");
  SC_CHECK_ARG(d->n_in <= DSP_MAX_I32 && d->n_out <= DSP_MAX_I32 && d->n_out * d->basis <= DSP_MAX_I32 &&
                   d->nnz <= DSP_MAX_I32,
               "dsparse: n_in, n_out basis and nnz must fit 32-bit indices");
  const int64_t cmax = d->c_in > d->c_out ? d->c_in : d->c_out, nmax = d->n_in > d->n_out ? d->n_in : d->n_out;
  SC_CHECK_ARG(cmax < ((int64_t)1 << 20) && d->batch < ((int64_t)1 << 20) && d->batch * cmax < ((int64_t)1 << 24) &&
                   d->basis * cmax <= DSP_MAX_I32 && d->batch * cmax * d->basis * nmax < DSP_MAX_ELEMS,
               "dsparse: tensor too large");
  std::memset(p, 0, sizeof(*p));
  p->batch = d->batch;
  p->c_in = d->c_in;
  p->c_out = d->c_out;
  p->n_in = d->n_in;
  p->n_out = d->n_out;
  p->nnz = d->nnz;
  p->groups = d->groups;
  p->K = d->basis;
  p->cg = (int)(d->c_in / d->groups);
  p->og = (int)(d->c_out / d->groups);
  p->rows = d->n_out * d->batch;
  p->wn = d->c_out * p->cg * p->K;
  p->path = d->groups == 1 && dsp_mfma_channels(d->c_in) && dsp_mfma_channels(d->c_out) ? SC_DSPARSE_PATH_MFMA
                                                                                         : SC_DSPARSE_PATH_GENERAL;
  SC_CHECK_ARG(p->wn <= DSP_MAX_I32, "dsparse: weight too large");
  // about 256 rows to a slice, 64 slices at the most
  int64_t s = (p->rows + 255) / 256;
  s = s < 1 ? 1 : (s > 64 ? 64 : s);
  p->per_slice = (p->rows + s - 1) / s;
  p->slices = (p->rows + p->per_slice - 1) / p->per_slice;
  // launches: every grid below 2^31 workgroups, second dimensions below 65536
  SC_CHECK_ARG((p->rows + DSP_ROWS - 1) / DSP_ROWS <= DSP_MAX_I32 && (p->K * d->c_in + 63) / 64 < 65536 &&
                   p->slices * (d->c_out / 32 + 1) * p->K <= DSP_MAX_I32 &&
                   (d->batch * cmax + DSP_TP - 1) / DSP_TP < 65536,
               "dsparse: too many workgroups for one launch");
  const int64_t wg = p->slices * p->groups * ((p->og + DSP_WG_OC - 1) / DSP_WG_OC) *
                     (((int64_t)p->K * p->cg + DSP_WG_J - 1) / DSP_WG_J);
  SC_CHECK_ARG(wg <= DSP_MAX_I32, "dsparse: too many workgroups for one launch");
  return 0;
}

static int dsp_check_csr(const DspPlan& p, const sc_dsparse_csr* m, const int64_t rows, const char* what) {
  SC_CHECK_ARG(m, "null argument");
  SC_CHECK_ARG(m->rows == rows, std::string("dsparse: the ") + what + " has the wrong number of rows (splits length)");
  SC_CHECK_ARG(m->nnz == p.nnz, std::string("dsparse: the ") + what + " does not hold desc.nnz entries");
  SC_CHECK_ARG(m->splits && (p.nnz == 0 || (m->cols && m->vals)), "null argument");
  return 0;
}

// floats of the forward workspace: W2 | Xq | out2
static size_t dsp_fwd_floats(const DspPlan& p) {
  return (size_t)(p.wn + p.n_in * p.batch * p.c_in + p.rows * p.c_out);
}
// floats of the backward workspace: W2T | g2 | gZ | gXq | parts | parts_b
static size_t dsp_bwd_floats(const DspPlan& p) {
  return (size_t)(p.wn + p.rows * p.c_out + p.rows * p.K * p.c_in + p.n_in * p.batch * p.c_in +
                  p.slices * (p.wn + p.c_out));
}

extern "C" int sc_dsparse_path(const sc_dsparse_desc* d) {
  DspPlan p;
  if (dsp_plan(d, &p)) return 0;
  return p.path;
}

extern "C" size_t sc_dsparse_workspace_bytes(const sc_dsparse_desc* d) {
  DspPlan p;
  if (dsp_plan(d, &p)) return 0;
  const size_t f = dsp_fwd_floats(p), b = dsp_bwd_floats(p);
  return (f > b ? f : b) * sizeof(float);
}

extern "C" size_t sc_dsparse_forward_workspace_bytes(const sc_dsparse_desc* d) {
  DspPlan p;
  if (dsp_plan(d, &p)) return 0;
  return dsp_fwd_floats(p) * sizeof(float);
}

static int dsp_pack(const float* src, const float* scale, float* dst, const int64_t n, const int64_t cols,
                    sc_stream_t st) {
  const dim3 grid((unsigned)((n + DSP_TP - 1) / DSP_TP), (unsigned)((cols + DSP_TP - 1) / DSP_TP));
  SC_LAUNCH(k_dsp_pack, grid, dim3(256), 0, st, src, scale, dst, (int)n, (int)cols);
  return sc_check_launch("k_dsp_pack");
}

static int dsp_unpack(const float* src, const float* scale, const float* bias, float* dst, const int64_t n,
                      const int64_t cols, const int64_t c, sc_stream_t st) {
  const dim3 grid((unsigned)((n + DSP_TP - 1) / DSP_TP), (unsigned)((cols + DSP_TP - 1) / DSP_TP));
  SC_LAUNCH(k_dsp_unpack, grid, dim3(256), 0, st, src, scale, bias, dst, (int)n, (int)cols, (int)c);
  return sc_check_launch("k_dsp_unpack");
}

// forward: dst = Z over the (o, k) rows from src = Xq; adjoint: dst = gXq over the input points from src = gZ
static int dsp_spmm(const DspPlan& p, const sc_dsparse_csr* m, const bool adjoint, const float* src, float* dst,
                    sc_stream_t st) {
  DspSpmmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.splits = m->splits;
  a.cols = m->cols;
  a.vals = m->vals;
  a.src = src;
  a.dst = dst;
  const DspSide flat = {p.batch * p.c_in, 1, (int)p.c_in};
  const DspSide zed = {p.batch * p.K * p.c_in, p.K, (int)(p.K * p.c_in)};
  a.s = adjoint ? zed : flat;
  a.d = adjoint ? flat : zed;
  a.rows = (int)m->rows;
  a.src_rows = (int)(adjoint ? p.n_out * p.K : p.n_in);
  a.nnz = (int)p.nnz;
  a.c = (int)p.c_in;
  a.width = (int)(p.batch * p.c_in);
  SC_LAUNCH(k_dsp_spmm, dim3((unsigned)((m->rows + 3) / 4)), dim3(256), 0, st, a);
  return sc_check_launch("k_dsp_spmm");
}

static int dsp_fold(const DspPlan& p, const float* w, float* w2, float* w2t, sc_stream_t st) {
  SC_LAUNCH(k_dsp_fold, dim3((unsigned)((p.wn + 255) / 256)), dim3(256), 0, st, w, w2, w2t, (int)p.c_out, p.cg, p.og,
            p.K);
  return sc_check_launch("k_dsp_fold");
}

template <int NOB>
static int dsp_gemm_launch(const DspGemmArgs& g, const unsigned groups, sc_stream_t st) {
  const dim3 grid((unsigned)((g.M + DSPM_ROWS - 1) / DSPM_ROWS), groups);
  SC_LAUNCH(k_dsp_gemm_mfma<NOB>, grid, dim3(256), 0, st, g);
  return sc_check_launch("k_dsp_gemm_mfma");
}

static int dsp_contract(const DspPlan& p, const bool adjoint, const float* in, const float* m, float* out,
                        sc_stream_t st) {
  if (p.path == SC_DSPARSE_PATH_MFMA) {
    const int kc = (int)(p.K * p.c_in), co = (int)p.c_out;
    const DspGemmArgs g = adjoint ? DspGemmArgs{in, m, out, p.rows, co, co, kc, kc}
                                  : DspGemmArgs{in, m, out, p.rows, kc, kc, co, co};
    const int64_t width = adjoint ? p.c_in : p.c_out;
    const unsigned groups = adjoint ? (unsigned)p.K : 1u;
    if (width == 32) return dsp_gemm_launch<1>(g, groups, st);
    if (width == 64) return dsp_gemm_launch<2>(g, groups, st);
    return dsp_gemm_launch<4>(g, groups, st);
  }
  DspContractArgs a;
  std::memset(&a, 0, sizeof(a));
  a.in = in;
  a.m = m;
  a.out = out;
  a.rows = p.rows;
  if (!adjoint) {
    a.KK = p.K;
    a.CI = (int)p.c_in;
    a.L = p.cg;
    a.NJ = (int)p.c_out;
    a.jmod = (int)p.c_out;
    a.jdiv = p.og;
  } else {
    a.KK = 1;
    a.CI = (int)p.c_out;
    a.L = p.og;
    a.NJ = (int)(p.K * p.c_in);
    a.jmod = (int)p.c_in;
    a.jdiv = p.cg;
  }
  const dim3 grid((unsigned)((p.rows + DSP_ROWS - 1) / DSP_ROWS), (unsigned)((a.NJ + 63) / 64));
  SC_LAUNCH(k_dsp_contract, grid, dim3(256), 0, st, a);
  return sc_check_launch("k_dsp_contract");
}

extern "C" int sc_dsparse_forward(const sc_dsparse_desc* d, const sc_dsparse_csr* psi, const float* x, const float* q,
                                  const float* weight, const float* bias, float* out, float* z, void* ws,
                                  size_t ws_bytes, void* stream) {
  DspPlan p;
  if (int e = dsp_plan(d, &p)) return e;
  if (int e = dsp_check_csr(p, psi, p.n_out * p.K, "forward CSR")) return e;
  SC_CHECK_ARG(x && q && weight && out && z && ws, "null argument");
  SC_CHECK_ARG(ws_bytes >= dsp_fwd_floats(p) * sizeof(float), "dsparse: workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  float* w2 = (float*)ws;
  float* xq = w2 + p.wn;
  float* out2 = xq + p.n_in * p.batch * p.c_in;
  if (int e = dsp_fold(p, weight, w2, nullptr, st)) return e;
  if (int e = dsp_pack(x, q, xq, p.n_in, p.batch * p.c_in, st)) return e;
  if (int e = dsp_spmm(p, psi, false, xq, z, st)) return e;
  if (int e = dsp_contract(p, false, z, w2, out2, st)) return e;
  return dsp_unpack(out2, nullptr, bias, out, p.n_out, p.batch * p.c_out, p.c_out, st);
}

extern "C" int sc_dsparse_backward(const sc_dsparse_desc* d, const sc_dsparse_csr* psi_t, const float* q,
                                   const float* weight, const float* z, const float* gout, float* gx, float* gw,
                                   float* gbias, void* ws, size_t ws_bytes, void* stream) {
  DspPlan p;
  if (int e = dsp_plan(d, &p)) return e;
  SC_CHECK_ARG(gx || gw || gbias, "dsparse: no gradient is wanted");
  if (gx)
    if (int e = dsp_check_csr(p, psi_t, p.n_in, "transposed CSR")) return e;
  SC_CHECK_ARG(gout && ws && ((weight && q) || !gx) && (z || !gw), "null argument");
  SC_CHECK_ARG(ws_bytes >= dsp_bwd_floats(p) * sizeof(float), "dsparse: workspace too small");
  sc_stream_t st = (sc_stream_t)stream;
  float* w2t = (float*)ws;
  float* g2 = w2t + p.wn;
  float* gz = g2 + p.rows * p.c_out;
  float* gxq = gz + p.rows * p.K * p.c_in;
  float* parts = gxq + p.n_in * p.batch * p.c_in;
  float* parts_b = parts + p.slices * p.wn;
  if (int e = dsp_pack(gout, nullptr, g2, p.n_out, p.batch * p.c_out, st)) return e;
  if (gx) {
    if (int e = dsp_fold(p, weight, nullptr, w2t, st)) return e;
    if (int e = dsp_contract(p, true, g2, w2t, gz, st)) return e;
    if (int e = dsp_spmm(p, psi_t, true, gz, gxq, st)) return e;
    if (int e = dsp_unpack(gxq, q, nullptr, gx, p.n_in, p.batch * p.c_in, p.c_in, st)) return e;
  }
  if ((gw || gbias) && p.path == SC_DSPARSE_PATH_MFMA) {
    DspWgMArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g2 = g2;
    a.Z = gw ? z : nullptr;
    a.parts = parts;
    a.parts_b = parts_b;
    a.rows = p.rows;
    a.per_slice = p.per_slice;
    a.c_in = (int)p.c_in;
    a.c_out = (int)p.c_out;
    a.K = p.K;
    a.kj = gw ? p.K : 1;                                     // the bias sums come from the waves of k = 0
    a.slices = (int)p.slices;
    const int64_t jobs = p.slices * (p.c_out / 32) * a.kj;
    const dim3 grid((unsigned)((jobs + 3) / 4));
    if (p.c_in == 32) SC_LAUNCH(k_dsp_wgrad_mfma<1>, grid, dim3(256), 0, st, a);
    else if (p.c_in == 64) SC_LAUNCH(k_dsp_wgrad_mfma<2>, grid, dim3(256), 0, st, a);
    else SC_LAUNCH(k_dsp_wgrad_mfma<4>, grid, dim3(256), 0, st, a);
    if (int e = sc_check_launch("k_dsp_wgrad_mfma")) return e;
  } else if (gw || gbias) {
    DspWgArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g2 = g2;
    a.Z = gw ? z : nullptr;
    a.parts = parts;
    a.parts_b = parts_b;
    a.rows = p.rows;
    a.per_slice = p.per_slice;
    a.c_in = (int)p.c_in;
    a.c_out = (int)p.c_out;
    a.cg = p.cg;
    a.og = p.og;
    a.K = p.K;
    a.slices = (int)p.slices;
    a.oc_tiles = (p.og + DSP_WG_OC - 1) / DSP_WG_OC;
    a.j_tiles = gw ? (p.K * p.cg + DSP_WG_J - 1) / DSP_WG_J : 1;   // the bias sums come from the first column tile
    const int64_t wg = p.slices * p.groups * a.oc_tiles * a.j_tiles;
    SC_LAUNCH(k_dsp_wgrad, dim3((unsigned)wg), dim3(256), 0, st, a);
    if (int e = sc_check_launch("k_dsp_wgrad")) return e;
  }
  if (gw || gbias) {
    const int64_t n = p.wn + p.c_out;
    SC_LAUNCH(k_dsp_wreduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)parts,
              (const float*)parts_b, gw, gbias, (int)p.c_out, p.cg, p.K, (int)p.slices);
    if (int e = sc_check_launch("k_dsp_wreduce")) return e;
  }
  return 0;
}
