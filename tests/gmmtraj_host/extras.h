// What csrc/gmm_traj.hip needs beyond tests/gmm_host/common.h (tests/test_gmmtraj_host_cpu.py): the wave-wide ballot, the first
// lane's value, find-first-set, the row tile and the launch-counter kind.  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#define MLPG_HIP_GMM_TRAJ_ROW_TILE 64
inline unsigned long long g_ballot[8][64];
inline int g_first[8][64];
// every lane of the wave calls it (no divergence in the kernel at its call sites): bit l of the result is lane l's predicate
inline unsigned long long __ballot(int pred) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_ballot[w][l] = pred ? 1ull : 0ull;
  g_wave_bar[w]->arrive_and_wait();
  unsigned long long m = 0;
  for (int i = 0; i < 64; ++i) m |= g_ballot[w][i] << i;
  g_wave_bar[w]->arrive_and_wait();
  return m;
}
inline int __builtin_amdgcn_readfirstlane(int v) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_first[w][l] = v;
  g_wave_bar[w]->arrive_and_wait();
  const int r = g_first[w][0];
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
namespace mlpg {
constexpr int kCountGmmTraj = 33;
}
