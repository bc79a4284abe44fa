// What csrc/dtw_costs.hip and csrc/dtw.hip need beyond tests/gmm_host/common.h (tests/test_dtw_costs_host_cpu.py): the wave-wide
// ballot and find-first-set of the trim kernel, the dtype, tie-rule and error constants, and stand-ins for max_workgroups /
// items_per_launch.  The stand-in for mlpg::scratch() is the shim's: the window kernel's cfirst / clast and the cost kernel's D
// rows and back-pointers start as 0xFF bytes.  Included behind common.h and in front of the kernel texts.
#pragma once
#include "common.h"
#include <cstdint>
#define MLPG_HIP_F32 0
#define MLPG_HIP_F64 1
#define MLPG_HIP_ENOMEM (-3)
#define MLPG_HIP_TIE_FIRST_MIN 0
#define MLPG_HIP_TIE_DIAG_LAST 1
// one bit per lane of the wave whose predicate holds (lanes past the workgroup's end give 0)
inline unsigned long long __ballot(int pred) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_xs[w][l] = pred ? 1ull : 0ull;
  g_wave_bar[w]->arrive_and_wait();
  unsigned long long r = 0;
  const int lanes = (int)(blockDim.x - 64u * w < 64u ? blockDim.x - 64u * w : 64u);
  for (int k = 0; k < lanes; ++k) r |= g_xs[w][k] << k;
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
namespace mlpg {
constexpr long max_workgroups(int threads) { return ((1L << 32) - 1) / threads; }
inline long items_per_launch(long per_item, int threads) { return per_item > 0 ? max_workgroups(threads) / per_item : 0; }
}
