// What csrc/mlpg_gv.hip, csrc/assemble.h and csrc/device_prims.h need beyond tests/gmm_host/common.h
// (tests/test_gvmlpg_host_cpu.py): the cross-lane moves (one lane up, one lane down; the xor shuffle is common.h's), the
// structures and checks of csrc/common.h that the entry point uses, and stand-ins for the device-only builtins that
// device_prims.h names in functions this file never calls.  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#define __forceinline__ inline
#define MLPG_HIP_F32 0
#define MLPG_HIP_F64 1
#define MLPG_HIP_VAR_FRAME 0
#define MLPG_HIP_VAR_GLOBAL 1
#define MLPG_HIP_VAR_UNIT 2
// every lane of the wave calls these (no divergence in the kernel at its call sites); a lane without a source keeps its own value
inline double gv_lane_move(double v, int from_delta) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_xa[w][l] = v;
  g_wave_bar[w]->arrive_and_wait();
  const int src = l + from_delta;
  const double r = (src >= 0 && src < 64) ? g_xa[w][src] : v;
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
inline double __shfl_up(double v, int d) { return gv_lane_move(v, -d); }
inline double __shfl_down(double v, int d) { return gv_lane_move(v, d); }
// device-only names of device_prims.h (reciprocal seeds, buffer descriptors, bit casts): declared so that the header parses;
// the GV kernel uses recip_in_dtype alone, which is an exact divide here as on the device
typedef unsigned gv_u32x2 __attribute__((ext_vector_type(2)));
struct gv_rsrc {};
#define __amdgpu_buffer_rsrc_t gv_rsrc
inline double __builtin_amdgcn_rcp(double d) { return 1.0 / d; }
inline float __fdiv_rn(float a, float b) { return a / b; }
inline unsigned __builtin_amdgcn_readfirstlane(unsigned v) { return v; }
inline gv_rsrc __builtin_amdgcn_make_buffer_rsrc(void *, int, int, int) { return {}; }
inline gv_u32x2 __builtin_amdgcn_raw_buffer_load_b64(gv_rsrc, unsigned, unsigned, int) { return {0u, 0u}; }
inline unsigned __builtin_amdgcn_raw_buffer_load_b32(gv_rsrc, unsigned, unsigned, int) { return 0u; }
inline void __builtin_amdgcn_raw_buffer_store_b64(gv_u32x2, gv_rsrc, unsigned, unsigned, int) {}
inline void __builtin_amdgcn_raw_buffer_store_b32(unsigned, gv_rsrc, unsigned, unsigned, int) {}
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
inline float __uint_as_float(unsigned v) { float f; memcpy(&f, &v, 4); return f; }
inline unsigned __float_as_uint(float f) { unsigned v; memcpy(&v, &f, 4); return v; }
namespace mlpg {
constexpr int kCountGvAscent = 35, kCountGv = 37;
constexpr int kMaxWindows = 8, kMaxCoef = 48, kMaxExtent = 4;
struct WinSet { int nw, q, mw; int l[kMaxWindows], u[kMaxWindows], off[kMaxWindows]; double c[kMaxCoef]; };
struct Problem {
  const void *mean, *var, *grad_out; const int32_t *lengths; void *out; int32_t *status;
  int var_mode, B, Tmax, D, sd, pitch = 0; long ld_in, ld_gout, ld_out; int ld_status;
};
struct StreamMap { int n, total, begin[4], in_col[4], sd[4], out_col[4], stat_col[4], tr_u, tr_nd, tr_B, tr_in, tr_out, tr_stat; };
inline Problem dense_problem(const void *mean, const void *var, const void *grad_out, const int32_t *lengths, void *out, int32_t *status,
                             bool backward, int var_mode, int B, int Tmax, int D, int sd) {
  Problem p;
  p.mean = mean; p.var = var; p.grad_out = grad_out; p.lengths = lengths; p.out = out; p.status = status;
  p.var_mode = var_mode; p.B = B; p.Tmax = Tmax; p.D = D; p.sd = sd;
  p.ld_in = D; p.ld_gout = backward ? sd : 0; p.ld_out = backward ? D : sd; p.ld_status = sd;
  return p;
}
inline int check_dtype(const char *, int dtype) { return dtype == 0 || dtype == 1 ? 0 : -1; }
inline int check_var(const char *, int var_mode, const void *var) { return var_mode >= 0 && var_mode <= 2 && (var_mode == 2 || var) ? 0 : -1; }
inline int pack_windows(int nw, const int32_t *wl, const int32_t *wu, const double *wc, WinSet *ws) {
  memset(ws, 0, sizeof(*ws));
  ws->nw = nw;
  int off = 0;
  for (int w = 0; w < nw; ++w) {
    const int n = wl[w] + wu[w] + 1;
    ws->l[w] = wl[w]; ws->u[w] = wu[w]; ws->off[w] = off;
    for (int i = 0; i < n; ++i) ws->c[off + i] = wc[off + i];
    off += n;
    if (wl[w] + wu[w] > ws->q) ws->q = wl[w] + wu[w];
    const int m = wl[w] > wu[w] ? wl[w] : wu[w];
    if (m > ws->mw) ws->mw = m;
  }
  return 0;
}
}
