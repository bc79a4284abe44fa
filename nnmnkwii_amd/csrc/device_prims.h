// Device primitives shared by the MLPG kernel families (strip, constant-coefficient, chunked, wave-per-system, FIR):
// the reciprocal rules, buffer-descriptor access, the lane -> stream map of the merged launches and the 2x2 block
// algebra.  Each is defined here once; a family header adds only what is its own.  Device-only, no state.
#pragma once
#include <type_traits>

#include "common.h"

namespace mlpg {

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// ---- reciprocals ------------------------------------------------------------------------------------------------
// 1/d to ~1 ulp: hardware seed + two Newton steps (an IEEE-exact f64 divide is ~2x the
// instructions; the difference, 1e-16 relative, is far below every tolerance on this path).
__device__ __forceinline__ double fast_rcp(double d) {
  double x = __builtin_amdgcn_rcp(d);
  x = __builtin_fma(__builtin_fma(-d, x, 1.0), x, x);
  x = __builtin_fma(__builtin_fma(-d, x, 1.0), x, x);
  return x;
}
// The two rules for 1/var, side by side.
// recip_in_dtype: the reference's own -- evaluated in the input dtype (_mlpg.py:188), an exact divide in either.  The
// natural-order kernels and the constant-coefficient kernels (one reciprocal per dim and launch) use it.
template <typename T>
__device__ __forceinline__ double recip_in_dtype(T v);
template <>
__device__ __forceinline__ double recip_in_dtype<float>(float v) {
  return (double)__fdiv_rn(1.0f, v);  // reciprocal evaluated in float32 (_mlpg.py:188)
}
template <>
__device__ __forceinline__ double recip_in_dtype<double>(double v) {
  return 1.0 / v;
}
// tau_of: the per-frame kernels' (strip, chunked, wave).  float32 inputs keep the reference's float32 reciprocal exactly;
// float64 to ~1 ulp by fast_rcp (a correctly rounded division is 25 instructions, three per frame).
template <typename T>
__device__ __forceinline__ double tau_of(T v);
template <>
__device__ __forceinline__ double tau_of<float>(float v) {
  return (double)__fdiv_rn(1.0f, v);  // float32 reciprocal, as _mlpg.py:188
}
template <>
__device__ __forceinline__ double tau_of<double>(double v) {
  return fast_rcp(v);
}

// ---- buffer access ----------------------------------------------------------------------------------------------
// Loads go through buffer descriptors: a wave-uniform descriptor (the utterance's rows from the dim group's first
// column on), the row/window offset in an SGPR (soffset) and this lane's 32-bit byte offset in ONE VGPR -- no
// per-load 64-bit address arithmetic and no address registers (global_load with 64-bit VGPR addresses costs two VALU
// instructions and a register pair per load, which is what drove the strip kernel into scratch).  Stores likewise.
// Address = base + soff + loff; the hardware checks loff -- not soff -- against the descriptor's 2^31 - 1 bytes (what
// rows_fit_buffer guarantees, and what the FIR kernels use as their mask: mlpg_fir.hip).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base) {
  // the base must be wave-uniform PROVABLY (a lane-tainted descriptor is wrapped in a waterfall loop per access)
  const unsigned long long u = (unsigned long long)base;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0, 0x7fffffff, 0x00020000);
}
// AUX: the instruction's cache-policy immediate (1 sc0, 2 nt, 16 sc1)
template <typename T, int AUX = 0>
__device__ __forceinline__ T buf_ld(__amdgpu_buffer_rsrc_t rs, unsigned soff, unsigned loff) {
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "float or double");
  if constexpr (std::is_same<T, double>::value) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, loff, soff, AUX);
    return __longlong_as_double((long long)(((unsigned long long)v.y << 32) | v.x));
  } else {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, loff, soff, AUX));
  }
}
template <int AUX = 0>
__device__ __forceinline__ void buf_st(__amdgpu_buffer_rsrc_t rs, unsigned soff, unsigned loff, double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const u32x2 w = {(unsigned)u, (unsigned)(u >> 32)};
  __builtin_amdgcn_raw_buffer_store_b64(w, rs, loff, soff, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ void buf_st(__amdgpu_buffer_rsrc_t rs, unsigned soff, unsigned loff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, loff, soff, AUX);
}

// ---- merged launches: lane -> stream ----------------------------------------------------------------------------
// MULTI kernels: the stream a merged static-dim index belongs to (at most 4 streams, StreamMap::begin[] ascending, unused
// entries = INT_MAX) and the dim's columns there
struct LaneStream { int sd, din, dstat, dout, dvar; };  // dvar: the dim's window-0 column in a global (D,) variance vector
// transposed form (StreamMap::tr_u): merged index d = u * tr_nd + dim of utterance b0 + u; the columns carry the utterance's offset
__device__ __forceinline__ LaneStream lane_stream_tr(const StreamMap &sm, int d) {
  const int u = d / sm.tr_nd, dl = d - u * sm.tr_nd;
  return {sm.sd[0], u * sm.tr_in + sm.in_col[0] + dl, u * sm.tr_stat + sm.stat_col[0] + dl, u * sm.tr_out + sm.out_col[0] + dl,
          sm.in_col[0] + dl};
}
__device__ __forceinline__ LaneStream lane_stream(const StreamMap &sm, int d) {
  const int s_ = (d >= sm.begin[1]) + (d >= sm.begin[2]) + (d >= sm.begin[3]);
  auto pick = [&](const int (&v)[4]) { return s_ == 0 ? v[0] : s_ == 1 ? v[1] : s_ == 2 ? v[2] : v[3]; };
  const int dl = d - pick(sm.begin);
  return {pick(sm.sd), dl + pick(sm.in_col), dl + pick(sm.stat_col), dl + pick(sm.out_col), dl + pick(sm.in_col)};
}

// ---- 2x2 blocks, one per lane -----------------------------------------------------------------------------------
struct S2 { double a, b, c; };     // symmetric [a b; b c]
struct M2 { double a, b, c, d; };  // full      [a b; c d]
struct V2 { double x, y; };

__device__ __forceinline__ M2 mul_ms(const M2 &L, const S2 &S) {  // L S
  return {L.a * S.a + L.b * S.b, L.a * S.b + L.b * S.c, L.c * S.a + L.d * S.b, L.c * S.b + L.d * S.c};
}
__device__ __forceinline__ M2 mul_sm(const S2 &S, const M2 &V) {  // S V
  return {S.a * V.a + S.b * V.c, S.a * V.b + S.b * V.d, S.b * V.a + S.c * V.c, S.b * V.b + S.c * V.d};
}
__device__ __forceinline__ M2 mul_smt(const S2 &S, const M2 &V) {  // S V^T
  return {S.a * V.a + S.b * V.b, S.a * V.c + S.b * V.d, S.b * V.a + S.c * V.b, S.b * V.c + S.c * V.d};
}
__device__ __forceinline__ double amax4(const M2 &m) {  // twice this bounds the block's 2-norm
  return __builtin_fmax(__builtin_fmax(__builtin_fabs(m.a), __builtin_fabs(m.b)),
                        __builtin_fmax(__builtin_fabs(m.c), __builtin_fabs(m.d)));
}
__device__ __forceinline__ M2 mul_mm(const M2 &A, const M2 &B) {
  return {A.a * B.a + A.b * B.c, A.a * B.b + A.b * B.d, A.c * B.a + A.d * B.c, A.c * B.b + A.d * B.d};
}
__device__ __forceinline__ S2 mul_mmt_sym(const M2 &A, const M2 &B) {  // A B^T, symmetric by construction
  return {A.a * B.a + A.b * B.b, A.a * B.c + A.b * B.d, A.c * B.c + A.d * B.d};
}
__device__ __forceinline__ S2 mul_mtm_sym(const M2 &A, const M2 &B) {  // A^T B, symmetric by construction
  return {A.a * B.a + A.c * B.c, A.a * B.b + A.c * B.d, A.b * B.b + A.d * B.d};
}
__device__ __forceinline__ V2 mul_mv(const M2 &A, const V2 &v) { return {A.a * v.x + A.b * v.y, A.c * v.x + A.d * v.y}; }
__device__ __forceinline__ V2 mul_mtv(const M2 &A, const V2 &v) { return {A.a * v.x + A.c * v.y, A.b * v.x + A.d * v.y}; }
__device__ __forceinline__ V2 mul_sv(const S2 &S, const V2 &v) { return {S.a * v.x + S.b * v.y, S.b * v.x + S.c * v.y}; }
__device__ __forceinline__ S2 sub(const S2 &A, const S2 &B) { return {A.a - B.a, A.b - B.b, A.c - B.c}; }
__device__ __forceinline__ S2 add(const S2 &A, const S2 &B) { return {A.a + B.a, A.b + B.b, A.c + B.c}; }
__device__ __forceinline__ V2 sub(const V2 &A, const V2 &B) { return {A.x - B.x, A.y - B.y}; }
__device__ __forceinline__ V2 add(const V2 &A, const V2 &B) { return {A.x + B.x, A.y + B.y}; }
__device__ __forceinline__ M2 neg(const M2 &A) { return {-A.a, -A.b, -A.c, -A.d}; }
__device__ __forceinline__ M2 transpose(const M2 &A) { return {A.a, A.c, A.b, A.d}; }

}  // namespace mlpg
