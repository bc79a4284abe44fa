// What csrc/joint_rows.hip needs beyond tests/gmm_host/common.h (tests/test_joint_host_cpu.py): stand-ins for max_workgroups /
// items_per_launch whose limit comes from the command line (SHIM_MAX_WORKGROUPS), so that one build walks its tiles in slices of
// four; the population count; and hipMemsetAsync as memset.  Its constants come from include/nnmnkwii_joint.h, which the test
// copies next to the text.  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#include <cstdint>
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
namespace mlpg {
#ifdef SHIM_MAX_WORKGROUPS
constexpr long max_workgroups(int) { return SHIM_MAX_WORKGROUPS; }
#else
constexpr long max_workgroups(int threads) { return ((1L << 32) - 1) / threads; }
#endif
inline long items_per_launch(long per_item, int threads) { return per_item > 0 ? max_workgroups(threads) / per_item : 0; }
}
