// What csrc/wave_codec.hip needs beyond tests/gmm_host/common.h (tests/test_wave_host_cpu.py): stand-ins for max_workgroups /
// items_per_launch whose limit comes from the command line (SHIM_MAX_WORKGROUPS), so that one build walks a batch in several
// launches.  Its constants come from include/nnmnkwii_wave.h, which the test copies next to the text; the scan uses the shim's
// typed shuffles and barrier, log1p and pow are the host's.  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#include <cmath>
#include <cstdint>
namespace mlpg {
#ifdef SHIM_MAX_WORKGROUPS
constexpr long max_workgroups(int) { return SHIM_MAX_WORKGROUPS; }
#else
constexpr long max_workgroups(int threads) { return ((1L << 32) - 1) / threads; }
#endif
inline long items_per_launch(long per_item, int threads) { return per_item > 0 ? max_workgroups(threads) / per_item : 0; }
}
