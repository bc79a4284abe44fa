// K17: joint feature rows over one or two padded batches (nnmk_joint_count / nnmk_joint_write, include/nnmnkwii_joint.h; the
// reference's delta_features + concatenate + remove_zeros_frames, preprocessing/generic.py:250-288 and :335-356).
// tools/joint_model.py is the executable specification of everything below; `tiled` there is these three stages.
//
// A stable stream compaction of the B * Tmax frames with the deltas computed on the way, in three stages on one stream.  No
// workgroup waits for another and there are no atomics: the result is the same bits on every call.
//   joint_count_kernel  a workgroup of four waves takes a tile of NNMK_JOINT_TILE frames of one utterance, each wave a quarter of
//                       them, its lanes over the columns of the row.  Per frame: the row's values (joint_row), rounded to the
//                       output's dtype, |.| summed per lane (j = lane, lane + 64, ...) and over the lanes by a butterfly, so every
//                       lane holds the same s; the frame's bit is s > eps.  The tile's 64-bit mask goes to the workspace.  A tile
//                       past both lengths, and every tile in LIVE mode, gets its mask from the lengths alone.
//   joint_scan_kernel   ONE workgroup: the exclusive scan of the masks' popcounts into int64 tile offsets, 1024 tiles per step
//                       with a carry, and the (B + 1) utterance offsets.
//   joint_write_kernel  the same tiling: a kept frame's row number is its tile's offset plus the popcount of the mask below its
//                       bit; its row is computed again (the t +- k neighbours mostly come from L2) and stored, unless at or past cap.
// More tiles than one grid takes go in slices (items_per_launch, as nnmk_f0_interp).  Every offset is 64-bit.  Control flow is
// uniform across a wave wherever a shuffle is reached and across the workgroup wherever a barrier is.
// Compiled with -ffp-contract=off: a tap is a multiplication and an addition, each rounded.
#include <atomic>

#include "common.h"
#include "../../include/nnmnkwii_joint.h"

namespace mlpg {

namespace {

constexpr int kJointTile = NNMK_JOINT_TILE;
constexpr int kJointWaves = 4;
constexpr int kJointPerWave = kJointTile / kJointWaves;
constexpr int kJointScanChunk = 4;   // tiles per thread and step of the scan
constexpr int kJointMaxCoef = NNMK_JOINT_MAX_WINDOWS * (2 * NNMK_JOINT_MAX_EXTENT + 1);
static_assert(kJointTile <= 64 && kJointTile % kJointWaves == 0, "one 64-bit mask per tile");

std::atomic<long long> g_joint_launches{0};

struct JointArgs {
  const void *x, *y;
  const int32_t *len_x, *len_y;
  long ld_x, ld_y, ld_out;
  int Dx, Dy, fx, fy;   // widths; 1: float64
  int B, Tmax, nw, W, plain, keep, out_f64;
  double eps;
  long tpu;     // tiles per utterance
  long tile0;   // the tile of workgroup 0: more tiles than a grid takes go in slices
  unsigned long long *mask;
  long long *toff;
  void *out;
  long long cap;
  int wl[NNMK_JOINT_MAX_WINDOWS], wu[NNMK_JOINT_MAX_WINDOWS], woff[NNMK_JOINT_MAX_WINDOWS];
  double wc[kJointMaxCoef];
};

__device__ inline int joint_len(const int32_t *len, int b, int Tmax, int D) {
  if (!D) return 0;
  if (!len) return Tmax;
  const int n = len[b];
  return n < 0 ? 0 : (n > Tmax ? Tmax : n);
}

__device__ inline double joint_load(const void *p, int f64, size_t i) {
  return f64 ? ((const double *)p)[i] : (double)((const float *)p)[i];
}

// The row of frame t of utterance b, handed to emit(j, value in float64 before the rounding) for this lane's columns j = lane,
// lane + 64, ... in ascending order.  The row is walked in segments -- one source, one window: D columns from `base` on -- so that
// everything but the column is the same in all lanes: the window's extents and coefficients and the taps' row offsets are
// scalars, and no division is needed to find a column's window.
template <typename F>
__device__ inline void joint_row(const JointArgs &a, int b, int t, int lane, int lx, int ly, F &&emit) {
  for (int src = 0; src < 2; ++src) {
    const int D = src ? a.Dy : a.Dx;
    if (!D) continue;
    const int len = src ? ly : lx, f64 = src ? a.fy : a.fx;
    const long ld = src ? a.ld_y : a.ld_x;
    const void *p = src ? a.y : a.x;
    const size_t first = (size_t)b * a.Tmax * ld;
    for (int w = 0; w < a.nw; ++w) {
      const int base = (src ? a.Dx * a.nw : 0) + w * D;
      const int l = a.plain ? 0 : a.wl[w], u = a.plain ? 0 : a.wu[w];
      const double *c = a.wc + (a.plain ? 0 : a.woff[w]) + l;
      for (int j = base + ((lane - base) & 63); j < base + D; j += 64) {
        const size_t col = first + (size_t)(j - base);
        double acc = 0.0;
        if (t < len) {
          if (a.plain) {
            acc = joint_load(p, f64, col + (size_t)t * ld);
          } else {
            for (int k = -l; k <= u; ++k) {
              const int tt = t + k;
              if (tt >= 0 && tt < len) acc = acc + c[k] * joint_load(p, f64, col + (size_t)tt * ld);
            }
          }
        }
        emit(j, acc);
      }
    }
  }
}

__global__ __launch_bounds__(256) void joint_count_kernel(JointArgs a) {
  __shared__ unsigned long long wm[kJointWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long tile = a.tile0 + (long)blockIdx.x;
  const int b = (int)(tile / a.tpu), t0 = (int)(tile - (long)b * a.tpu) * kJointTile;
  const int lx = joint_len(a.len_x, b, a.Tmax, a.Dx), ly = joint_len(a.len_y, b, a.Tmax, a.Dy);
  const int L = lx > ly ? lx : ly;
  if (a.keep == NNMK_JOINT_LIVE || t0 >= L) {   // (the same in every thread of the workgroup)
    if (tid == 0) {
      const int n = L - t0;
      a.mask[tile] = n <= 0 ? 0ull : (n >= 64 ? ~0ull : (1ull << n) - 1);
    }
    return;
  }
  unsigned long long bits = 0;
  for (int i = 0; i < kJointPerWave; ++i) {
    const int f = wave * kJointPerWave + i, t = t0 + f;
    if (t >= L) break;   // (the same in every lane of the wave)
    double s = 0.0;
    joint_row(a, b, t, lane, lx, ly, [&](int, double v) {
      if (!a.out_f64) v = (double)(float)v;
      s = s + fabs(v);
    });
    for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m);
    if (s > a.eps) bits |= 1ull << f;
  }
  if (lane == 0) wm[wave] = bits;
  __syncthreads();
  if (tid == 0) {
    unsigned long long m = 0;
    for (int w = 0; w < kJointWaves; ++w) m |= wm[w];
    a.mask[tile] = m;
  }
}

__global__ __launch_bounds__(256) void joint_scan_kernel(const unsigned long long *mask, long long *toff, long long *offsets, long ntiles,
                                                         long tpu, int B) {
  __shared__ long long wsum[kJointWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  long long carry = 0;
  for (long c0 = 0; c0 < ntiles; c0 += 256 * kJointScanChunk) {
    const long i0 = c0 + (long)kJointScanChunk * tid;
    int n[kJointScanChunk];
    long long mine = 0;
    for (int q = 0; q < kJointScanChunk; ++q) {
      n[q] = i0 + q < ntiles ? __popcll(mask[i0 + q]) : 0;
      mine += n[q];
    }
    long long inc = mine;
    for (int off = 1; off < 64; off <<= 1) {
      const long long u = __shfl_up(inc, off);
      if (lane >= off) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long o = carry + inc - mine, total = 0;
    for (int w = 0; w < kJointWaves; ++w) {
      if (w < wave) o += wsum[w];
      total += wsum[w];
    }
    for (int q = 0; q < kJointScanChunk; ++q)
      if (i0 + q < ntiles) {
        toff[i0 + q] = o;
        if ((i0 + q) % tpu == 0) offsets[(i0 + q) / tpu] = o;
        o += n[q];
      }
    carry += total;
    __syncthreads();   // (wsum is free for the next step)
  }
  if (tid == 0) offsets[B] = carry;
}

__global__ __launch_bounds__(256) void joint_write_kernel(JointArgs a) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long tile = a.tile0 + (long)blockIdx.x;
  const unsigned long long m = a.mask[tile];
  if (!m) return;
  const long long first = a.toff[tile];
  const int b = (int)(tile / a.tpu), t0 = (int)(tile - (long)b * a.tpu) * kJointTile;
  const int lx = joint_len(a.len_x, b, a.Tmax, a.Dx), ly = joint_len(a.len_y, b, a.Tmax, a.Dy);
  for (int i = 0; i < kJointPerWave; ++i) {
    const int f = wave * kJointPerWave + i;
    if (!((m >> f) & 1)) continue;
    const long long r = first + __popcll(m & ((1ull << f) - 1));
    if (r >= a.cap) continue;
    const size_t row = (size_t)r * a.ld_out;
    joint_row(a, b, t0 + f, lane, lx, ly, [&](int j, double v) {
      if (a.out_f64)
        ((double *)a.out)[row + j] = v;
      else
        ((float *)a.out)[row + j] = (float)v;
    });
  }
}

int joint_refuse(const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  set_error(fmt, a, b, c);
  return MLPG_HIP_EINVAL;
}

bool joint_dtype_ok(int dtype) { return dtype == NNMK_JOINT_F32 || dtype == NNMK_JOINT_F64; }

// The checks both entries share and the kernels' arguments.  0: go; 1: nothing to do (B * Tmax * W == 0); -1: refused.
int joint_args(int device, int dtype_x, const void *x, int64_t ld_x, const int32_t *len_x, int Dx, int dtype_y, const void *y, int64_t ld_y,
               const int32_t *len_y, int Dy, int B, int Tmax, int num_windows, const int32_t *win_l, const int32_t *win_u,
               const double *win_coef, int dtype_out, const void *workspace, int64_t workspace_bytes, JointArgs *a) {
  if (!joint_dtype_ok(dtype_x) || (Dy > 0 && !joint_dtype_ok(dtype_y)) || !joint_dtype_ok(dtype_out))
    return joint_refuse("joint: dtype must be 0 (float32) or 1 (float64), got dtype_x = %lld, dtype_y = %lld, dtype_out = %lld", dtype_x, dtype_y,
                        dtype_out);
  if (B < 0 || Tmax < 0 || Dx < 0 || Dy < 0)
    return joint_refuse("joint: negative size (B = %lld, Tmax = %lld, Dx or Dy = %lld)", B, Tmax, Dx < Dy ? Dx : Dy);
  if (ld_x < Dx || ld_y < Dy)
    return joint_refuse("joint: the row strides must reach the last column (ld_x = %lld, ld_y = %lld below Dx, Dy)", ld_x, ld_y);
  if (num_windows < 0 || num_windows > NNMK_JOINT_MAX_WINDOWS)
    return joint_refuse("joint: num_windows must be in [0, %lld], got %lld", NNMK_JOINT_MAX_WINDOWS, num_windows);
  if (num_windows > 0 && (!win_l || !win_u || !win_coef)) return joint_refuse("joint: NULL window table");
  int ncoef = 0;
  for (int w = 0; w < num_windows; ++w) {
    if (win_l[w] < 0 || win_l[w] > NNMK_JOINT_MAX_EXTENT || win_u[w] < 0 || win_u[w] > NNMK_JOINT_MAX_EXTENT)
      return joint_refuse("joint: window %lld has l = %lld, u = %lld outside [0, 8]", w, win_l[w], win_u[w]);
    a->wl[w] = win_l[w];
    a->wu[w] = win_u[w];
    a->woff[w] = ncoef;
    for (int k = 0; k <= win_l[w] + win_u[w]; ++k) a->wc[ncoef + k] = win_coef[ncoef + k];
    ncoef += win_l[w] + win_u[w] + 1;
  }
  const int nw = num_windows > 0 ? num_windows : 1;
  const long long W = ((long long)Dx + Dy) * nw;
  if (W > 2147483647LL) return joint_refuse("joint: the row width (Dx + Dy) * windows = %lld is over 2^31 - 1", W);
  const int64_t need = nnmk_joint_workspace_bytes(B, Tmax);
  if (workspace_bytes < need) return joint_refuse("joint: the workspace has %lld bytes, %lld are needed", workspace_bytes, need);
  if (int rc = check_device("joint", device)) return rc;
  if (B == 0 || Tmax == 0 || W == 0) return 1;
  if ((Dx > 0 && !x) || (Dy > 0 && !y)) return joint_refuse("joint: NULL x or y");
  if (!workspace) return joint_refuse("joint: NULL workspace");
  if ((uintptr_t)workspace % 8) return joint_refuse("joint: the workspace must be aligned to 8 bytes");
  a->x = x;
  a->y = y;
  a->len_x = len_x;
  a->len_y = len_y;
  a->ld_x = (long)ld_x;
  a->ld_y = (long)ld_y;
  a->Dx = Dx;
  a->Dy = Dy;
  a->fx = dtype_x == NNMK_JOINT_F64;
  a->fy = dtype_y == NNMK_JOINT_F64;
  a->B = B;
  a->Tmax = Tmax;
  a->nw = nw;
  a->W = (int)W;
  a->plain = num_windows == 0;
  a->out_f64 = dtype_out == NNMK_JOINT_F64;
  a->tpu = ((long)Tmax + kJointTile - 1) / kJointTile;
  a->tile0 = 0;
  a->mask = (unsigned long long *)workspace;
  a->toff = (long long *)workspace + (long)B * a->tpu;
  return 0;
}

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int nnmk_joint_abi_version(void) { return NNMK_JOINT_ABI_VERSION; }

__attribute__((visibility("default"))) long long nnmk_joint_launch_count(void) { return g_joint_launches.load(std::memory_order_relaxed); }

__attribute__((visibility("default"))) int64_t nnmk_joint_workspace_bytes(int B, int Tmax) {
  if (B < 0 || Tmax < 0) return -1;
  return 16 * (int64_t)B * (((int64_t)Tmax + kJointTile - 1) / kJointTile);
}

__attribute__((visibility("default"))) int nnmk_joint_count(int device, void *stream, int dtype_x, const void *x, int64_t ld_x,
                                                            const int32_t *len_x, int Dx, int dtype_y, const void *y, int64_t ld_y,
                                                            const int32_t *len_y, int Dy, int B, int Tmax, int num_windows,
                                                            const int32_t *win_l, const int32_t *win_u, const double *win_coef, int keep,
                                                            double eps, int dtype_out, void *workspace, int64_t workspace_bytes,
                                                            int64_t *offsets) {
  JointArgs a = {};
  if (keep != NNMK_JOINT_NONZERO && keep != NNMK_JOINT_LIVE) return joint_refuse("joint: unknown keep mode %lld", keep);
  if (!(eps >= 0.0)) return joint_refuse("joint: eps must be >= 0 (and no NaN)");
  if (B > 0 && !offsets) return joint_refuse("joint: NULL offsets");
  const int rc = joint_args(device, dtype_x, x, ld_x, len_x, Dx, dtype_y, y, ld_y, len_y, Dy, B, Tmax, num_windows, win_l, win_u, win_coef,
                            dtype_out, workspace, workspace_bytes, &a);
  if (rc < 0 || (rc == 1 && B == 0)) return rc < 0 ? rc : 0;
  DeviceGuard g("joint", device);
  if (g.rc) return g.rc;
  hipStream_t st = (hipStream_t)stream;
  if (rc == 1) {
    MLPG_HIP_CHECK(hipMemsetAsync(offsets, 0, sizeof(int64_t) * ((size_t)B + 1), st));
    return 0;
  }
  a.keep = keep;
  a.eps = eps;
  const long ntiles = (long)B * a.tpu, step = items_per_launch(1, 256);
  for (long i0 = 0; i0 < ntiles; i0 += step) {
    a.tile0 = i0;
    hipLaunchKernelGGL(joint_count_kernel, dim3((unsigned)(ntiles - i0 < step ? ntiles - i0 : step)), dim3(256), 0, st, a);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(joint_scan_kernel, dim3(1), dim3(256), 0, st, (const unsigned long long *)a.mask, a.toff, (long long *)offsets, ntiles,
                     a.tpu, B);
  MLPG_HIP_CHECK(hipGetLastError());
  g_joint_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

__attribute__((visibility("default"))) int nnmk_joint_write(int device, void *stream, int dtype_x, const void *x, int64_t ld_x,
                                                            const int32_t *len_x, int Dx, int dtype_y, const void *y, int64_t ld_y,
                                                            const int32_t *len_y, int Dy, int B, int Tmax, int num_windows,
                                                            const int32_t *win_l, const int32_t *win_u, const double *win_coef,
                                                            const void *workspace, int64_t workspace_bytes, int dtype_out, void *out,
                                                            int64_t ld_out, int64_t cap) {
  JointArgs a = {};
  if (cap < 0) return joint_refuse("joint: cap = %lld is negative", cap);
  const int nw = num_windows > 0 ? num_windows : 1;
  if (Dx >= 0 && Dy >= 0 && ld_out < ((int64_t)Dx + Dy) * nw)
    return joint_refuse("joint: the row strides must reach the last column (ld_out = %lld below W = %lld)", ld_out, ((int64_t)Dx + Dy) * nw);
  const int rc = joint_args(device, dtype_x, x, ld_x, len_x, Dx, dtype_y, y, ld_y, len_y, Dy, B, Tmax, num_windows, win_l, win_u, win_coef,
                            dtype_out, workspace, workspace_bytes, &a);
  if (rc < 0) return rc;
  if (rc == 1 || cap == 0) return 0;
  if (!out) return joint_refuse("joint: NULL out");
  DeviceGuard g("joint", device);
  if (g.rc) return g.rc;
  a.out = out;
  a.ld_out = (long)ld_out;
  a.cap = cap;
  const long ntiles = (long)B * a.tpu, step = items_per_launch(1, 256);
  for (long i0 = 0; i0 < ntiles; i0 += step) {
    a.tile0 = i0;
    hipLaunchKernelGGL(joint_write_kernel, dim3((unsigned)(ntiles - i0 < step ? ntiles - i0 : step)), dim3(256), 0, (hipStream_t)stream, a);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  g_joint_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

}  // extern "C"
