// sc_host_nufd.h -- host side of the point-cloud finite-difference entry points (kernels: sc_kernels_nufd.h).  Every entry
// point refuses a bad descriptor before any launch; a valid empty problem (no points) returns success without a launch.
// None of them needs a workspace, reads device memory on the host or waits for the device.
#pragma once
#include "sc_host_common.h"
#include "sc_kernels_nufd.h"

#define NUFD_MAX (((int64_t)1 << 31) - 1)

extern "C" int sc_knn(const sc_knn_desc* d, const float* data, const float* queries, int64_t* index, float* d2,
                      void* stream) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->d >= 1 && d->d <= 3, "knn: d must be 1, 2 or 3");
  SC_CHECK_ARG(d->n >= 0 && d->m >= 0, "knn: negative point count");
  SC_CHECK_ARG(d->n < NUFD_MAX && d->m < NUFD_MAX, "knn: point count out of range");
  SC_CHECK_ARG(d->k >= 3 && d->k <= NUFD_KMAX, "knn: k must be 3 to 32");
  SC_CHECK_ARG(d->m * d->k < NUFD_MAX, "knn: m k out of range");
  if (d->m == 0) return 0;
  SC_CHECK_ARG(d->k <= d->n, "knn: k exceeds the number of data points");
  SC_CHECK_ARG(data && queries && index && d2, "null argument");
  KnnArgs a;
  std::memset(&a, 0, sizeof(a));
  a.data = data;
  a.queries = queries;
  a.n = d->n;
  a.m = d->m;
  a.k = d->k;
  a.index = (long long*)index;
  a.d2 = d2;
  const dim3 grid((unsigned)((a.m + NUFD_QPB - 1) / NUFD_QPB));
  if (d->d == 1) SC_LAUNCH((k_knn<1>), grid, dim3(256), 0, (sc_stream_t)stream, a);
  else if (d->d == 2) SC_LAUNCH((k_knn<2>), grid, dim3(256), 0, (sc_stream_t)stream, a);
  else SC_LAUNCH((k_knn<3>), grid, dim3(256), 0, (sc_stream_t)stream, a);
  return sc_check_launch("k_knn");
}

static int nufd_check(const sc_nufd_desc* d, const bool weights) {
  SC_CHECK_ARG(d, "null argument");
  SC_CHECK_ARG(d->n >= 0 && d->n < NUFD_MAX, "nufd: point count out of range");
  SC_CHECK_ARG(d->k >= 1 && d->k <= NUFD_KMAX, "nufd: k must be 1 to 32");
  SC_CHECK_ARG(d->n_deriv >= 1 && d->n_deriv <= NUFD_MAX_DERIV, "nufd: 1 to 8 derivatives");
  SC_CHECK_ARG(d->batch >= 1 && d->batch < 65536, "nufd: 1 to 65535 batch entries");
  SC_CHECK_ARG(d->n * d->k * d->n_deriv < NUFD_MAX && d->n * d->batch * d->n_deriv < NUFD_MAX, "nufd: size out of range");
  if (weights) {
    SC_CHECK_ARG(d->d >= 1 && d->d <= 3, "nufd: d must be 1, 2 or 3");
    SC_CHECK_ARG(d->k >= d->d + 1, "nufd: k must be at least d + 1");
    for (int j = 0; j < d->n_deriv; ++j)
      SC_CHECK_ARG(d->deriv[j] >= 0 && d->deriv[j] < d->d, "nufd: derivative index outside [0, d)");
    SC_CHECK_ARG(!d->has_radius || (d->radius >= 0.0 && d->radius == d->radius), "nufd: the radius must be a number >= 0");
    SC_CHECK_ARG(!d->has_radius || d->d <= 2, "nufd: a radius needs d <= 2");
    SC_CHECK_ARG(d->lambda >= 0.0 && d->lambda == d->lambda, "nufd: lambda must be a number >= 0");
  }
  return 0;
}

extern "C" int sc_nufd_weights(const sc_nufd_desc* d, const float* points, const int64_t* index, const float* d2,
                               float* weights, int32_t* flag, void* stream) {
  if (int e = nufd_check(d, true)) return e;
  if (d->n == 0) return 0;
  SC_CHECK_ARG(points && index && weights && flag && (d2 || !d->has_radius), "null argument");
  NufdWArgs a;
  std::memset(&a, 0, sizeof(a));
  a.points = points;
  a.index = (const long long*)index;
  a.d2 = d2;
  a.weights = weights;
  a.flag = flag;
  a.n = d->n;
  a.k = d->k;
  a.n_deriv = d->n_deriv;
  for (int j = 0; j < d->n_deriv; ++j) a.deriv |= (unsigned)d->deriv[j] << (2 * j);
  a.has_radius = d->has_radius ? 1 : 0;
  a.r2 = (float)(d->radius * d->radius);
  a.lambda = d->lambda;
  const dim3 grid((unsigned)((a.n + 255) / 256));
  if (d->d == 1) SC_LAUNCH((k_nufd_weights<1>), grid, dim3(256), 0, (sc_stream_t)stream, a);
  else if (d->d == 2) SC_LAUNCH((k_nufd_weights<2>), grid, dim3(256), 0, (sc_stream_t)stream, a);
  else SC_LAUNCH((k_nufd_weights<3>), grid, dim3(256), 0, (sc_stream_t)stream, a);
  return sc_check_launch("k_nufd_weights");
}

static void nufd_apply_args(const sc_nufd_desc* d, NufdApplyArgs* a) {
  std::memset(a, 0, sizeof(*a));
  a->n = d->n;
  a->k = d->k;
  a->n_deriv = d->n_deriv;
  a->batch = d->batch;
}

extern "C" int sc_nufd_apply(const sc_nufd_desc* d, const float* weights, const int64_t* index, const float* values,
                             float* out, void* stream) {
  if (int e = nufd_check(d, false)) return e;
  if (d->n == 0) return 0;
  SC_CHECK_ARG(weights && index && values && out, "null argument");
  NufdApplyArgs a;
  nufd_apply_args(d, &a);
  a.weights = weights;
  a.index = (const long long*)index;
  a.in = values;
  a.out = out;
  SC_LAUNCH(k_nufd_apply, dim3((unsigned)((a.n + 255) / 256), (unsigned)a.batch), dim3(256), 0, (sc_stream_t)stream, a);
  return sc_check_launch("k_nufd_apply");
}

extern "C" int sc_nufd_apply_adjoint(const sc_nufd_desc* d, const float* weights, const int64_t* col_splits,
                                     const int32_t* perm, const float* gout, float* gvalues, void* stream) {
  if (int e = nufd_check(d, false)) return e;
  if (d->n == 0) return 0;
  SC_CHECK_ARG(weights && col_splits && perm && gout && gvalues, "null argument");
  NufdApplyArgs a;
  nufd_apply_args(d, &a);
  a.weights = weights;
  a.col_splits = (const long long*)col_splits;
  a.perm = perm;
  a.in = gout;
  a.out = gvalues;
  SC_LAUNCH(k_nufd_adjoint, dim3((unsigned)((a.n + 255) / 256), (unsigned)a.batch), dim3(256), 0, (sc_stream_t)stream, a);
  return sc_check_launch("k_nufd_adjoint");
}
