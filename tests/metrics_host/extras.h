// What csrc/frame_metrics.hip needs beyond tests/gmm_host/common.h (tests/test_metrics_host_cpu.py): the two wave-level builtins
// of its mt_wave_sync.  On the host a wave is 64 threads, so the wave barrier is a real one; the fences have nothing left to do.
// Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#include <cstdint>
#define __builtin_amdgcn_fence(order, scope) ((void)0)
#define __builtin_amdgcn_wave_barrier() (g_wave_bar[threadIdx.x >> 6]->arrive_and_wait())
