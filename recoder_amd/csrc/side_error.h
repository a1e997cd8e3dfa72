// The last-error buffer and the argument / launch checks of a side library (index, als, vae, ease, svd,
// rp3, slim).  Host only.  Everything here is static: each library is one translation unit in a .so of its
// own, so each has its own buffer, which its rk_<x>_last_error() returns.  The names stay clear of
// rk_set_error / RK_REQUIRE / RK_CHECK_LAUNCH of common.h, which vae.hip and svd.hip include as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

static thread_local char g_rk_side_err[512] = "";

static void rk_side_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_rk_side_err, sizeof(g_rk_side_err), fmt, ap);
  va_end(ap);
}

// a bad argument: "<function>: <msg>", return -2
#define RK_SIDE_REQUIRE(cond, msg)                                         \
  do {                                                                     \
    if (!(cond)) {                                                         \
      rk_side_set_error("%s: %s", __func__, msg);                          \
      return -2;                                                           \
    }                                                                      \
  } while (0)

// after a launch: "<kernel>: <HIP's error string>", return -1
#define RK_SIDE_CHECK_LAUNCH(name)                                         \
  do {                                                                     \
    hipError_t e__ = hipGetLastError();                                    \
    if (e__ != hipSuccess) {                                               \
      rk_side_set_error("%s: %s", name, hipGetErrorString(e__));           \
      return -1;                                                           \
    }                                                                      \
  } while (0)
