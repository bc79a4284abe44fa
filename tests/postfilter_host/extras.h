// What csrc/postfilter.hip needs beyond tests/gmm_host/common.h (tests/test_postfilter_host_cpu.py): the workgroup-wide OR behind
// a barrier, the dtype constants and check of csrc/common.h and the launch-counter kind.  MLPG_HIP_POSTFILTER_FRAME_TILE comes
// from the command line (the test reads it from include/mlpg_hip.h).  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#include <atomic>
#include <cstdint>
#define MLPG_HIP_F32 0
#define MLPG_HIP_F64 1
inline std::atomic<int> g_block_or{0};
// every thread of the workgroup calls it
inline int __syncthreads_or(int pred) {
  if (pred) g_block_or.store(1);
  g_block_bar->arrive_and_wait();
  const int r = g_block_or.load();
  g_block_bar->arrive_and_wait();
  if (threadIdx.x == 0) g_block_or.store(0);
  g_block_bar->arrive_and_wait();
  return r;
}
namespace mlpg {
constexpr int kCountPostfilter = 29;
inline int check_dtype(const char *, int dtype) { return dtype == 0 || dtype == 1 ? 0 : -1; }
}
