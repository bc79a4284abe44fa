// What csrc/f0_interp.hip needs beyond tests/gmm_host/common.h (tests/test_f0_host_cpu.py): stand-ins for max_workgroups /
// items_per_launch whose limit comes from the command line (SHIM_MAX_WORKGROUPS), so that one build walks a batch of fifteen
// (utterance, column) pairs in four launches.  Its constants come from include/nnmnkwii_f0.h, which the test copies next to the
// text; the scans use the shim's typed shuffles and barrier.  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#include <cstdint>
namespace mlpg {
#ifdef SHIM_MAX_WORKGROUPS
constexpr long max_workgroups(int) { return SHIM_MAX_WORKGROUPS; }
#else
constexpr long max_workgroups(int threads) { return ((1L << 32) - 1) / threads; }
#endif
inline long items_per_launch(long per_item, int threads) { return per_item > 0 ? max_workgroups(threads) / per_item : 0; }
}
