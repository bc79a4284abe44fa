// What csrc/colstats.hip needs beyond tests/gmm_host/common.h (tests/test_norm_host_cpu.py): the dtype constants and check of
// csrc/common.h and the two launch-counter kinds.  MLPG_HIP_COLSTATS_CHUNK_ROWS and _BLOCK_ROWS come from the command line (the
// test reads them from include/mlpg_hip.h).  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#include <cstdint>
#define MLPG_HIP_F32 0
#define MLPG_HIP_F64 1
namespace mlpg {
constexpr int kCountColStats = 39, kCountColAffine = 41;
inline int check_dtype(const char *, int dtype) { return dtype == 0 || dtype == 1 ? 0 : -1; }
}
