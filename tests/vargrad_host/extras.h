// What csrc/mlpg_vargrad.hip, csrc/mlpg_streams_bwd.hip and csrc/vargrad_element.h need beyond tests/gmm_host/common.h
// (tests/test_vargrad_host_cpu.py): the window and column tables of csrc/common.h, which the kernels take by value, its constants
// and the two launch-counter kinds.  Included behind common.h and in front of the kernel texts.
#pragma once
#include "common.h"
#include <cstdint>
#define MLPG_HIP_F32 0
#define MLPG_HIP_F64 1
#define MLPG_HIP_VAR_FRAME 0
#define MLPG_HIP_VAR_GLOBAL 1
namespace mlpg {
constexpr int kCountVarGrad = 13, kCountStreamsBwd = 15;
constexpr int kMaxWindows = 8, kMaxCoef = 48, kMaxExtent = 4, kMaxStreams = 64;
struct WinSet { int nw, q, mw; int l[kMaxWindows], u[kMaxWindows], off[kMaxWindows]; double c[kMaxCoef]; };
struct ColTable { int n, total; int begin[kMaxStreams], in_col[kMaxStreams], out_col[kMaxStreams], sd[kMaxStreams], stat_col[kMaxStreams]; };
constexpr int kStreamsBwdPass = 3;
}
