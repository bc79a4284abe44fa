// What csrc/modspec_filter.hip and csrc/modspec_fft.h need beyond tests/gmm_host/common.h (tests/test_msfilter_host_cpu.py): the
// bit reversal, sincospi, the dtype constants and check of csrc/common.h, the launch-counter kind, the two switches of the FFT
// route, and stand-ins for max_workgroups / items_per_launch whose limit comes from the command line (SHIM_MAX_WORKGROUPS), so
// that one build walks a batch of three utterances in two launches.  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#include <cstdint>
#define MLPG_HIP_F32 0
#define MLPG_HIP_F64 1
inline unsigned __brev(unsigned v) { return __builtin_bitreverse32(v); }
inline void sincospi(double x, double *s, double *c) {
  const double pi = 3.14159265358979323846;
  *s = sin(pi * x);
  *c = cos(pi * x);
}
namespace mlpg {
constexpr int kCountModspecFilter = 31;
inline int check_dtype(const char *, int dtype) { return dtype == 0 || dtype == 1 ? 0 : -1; }
inline bool modspec_fft_takes(int n) { return n >= 2 && n <= 4096 && !(n & (n - 1)); }
inline bool modspec_direct() { return false; }
#ifdef SHIM_MAX_WORKGROUPS
constexpr long max_workgroups(int) { return SHIM_MAX_WORKGROUPS; }
#else
constexpr long max_workgroups(int threads) { return ((1L << 32) - 1) / threads; }
#endif
inline long items_per_launch(long per_item, int threads) { return per_item > 0 ? max_workgroups(threads) / per_item : 0; }
}
