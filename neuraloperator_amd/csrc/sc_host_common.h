// sc_host_common.h -- what every host part of libsc_engine.so shares: the error state behind sc_last_error with the
// SC_CHECK_* macros and sc_check_launch, and sc_conj_dispatch.  sc_engine.cpp includes it after it has defined
// SC_DIAG_ENV, which the parts use for their measurement switches.
#pragma once
#include "../../include/sc_engine.h"

#include <string>

#include "sc_device.h"

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int sc_fail(const std::string& msg) {
  g_last_error = msg;
  return 1;
}

#define SC_CHECK_ARG(cond, msg) \
  do {                          \
    if (!(cond)) return sc_fail(std::string("sc_engine: ") + msg); \
  } while (0)

#define SC_CHECK_HIP(expr)                                                               \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return sc_fail(std::string("sc_engine: HIP error in " #expr ": ") + hipGetErrorString(e_)); \
  } while (0)

static int sc_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sc_fail(std::string("sc_engine: launch of ") + what + " failed: " + hipGetErrorString(e));
  return 0;
}

// the two conjugation flags of a contraction as compile-time tags, the way f2p_dispatch (sc_engine.cpp) hands out its
// sizes: returns f(sc_bool<CA>(), sc_bool<CB>()).  Every route picks its kernel instantiation through this one ladder.
template <bool B>
struct sc_bool {
  static constexpr bool value = B;
};
template <typename F>
static auto sc_conj_dispatch(int ca, int cb, F&& f) {
  if (!ca && !cb) return f(sc_bool<false>(), sc_bool<false>());
  if (ca && !cb) return f(sc_bool<true>(), sc_bool<false>());
  if (!ca && cb) return f(sc_bool<false>(), sc_bool<true>());
  return f(sc_bool<true>(), sc_bool<true>());
}
