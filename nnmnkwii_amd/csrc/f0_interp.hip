// K15: continuous F0 over a padded batch (nnmk_f0_interp, include/nnmnkwii_f0.h; the reference's preprocessing/f0.py:5-68,
// interp1d, and the V/UV flag of the Merlin recipe).  tools/f0_model.py is the executable specification of everything below;
// `tiled` there is this walk, frame for frame.
//
// f0_interp_kernel: a workgroup of four waves takes ONE column of ONE utterance and walks its L live frames in tiles of
// NNMK_F0_TILE.  The walk works on the ORIGINAL voiced flags (x > 0) alone; the reference's edge hold falls out of two rules:
// a frame with no voiced frame below it has p = 0 and a = b (frame 0 holds the first voiced value), one with none above it has
// q = L-1 and b = a (frame L-1 holds the last), and frames 0 and L-1, where not voiced, take a.  A frame with neither belongs to a
// column without a voiced frame and keeps its value.
//   load      thread i reads frame t0 + i once (float64 from here on), keeps it in a register and in LDS, and classifies it.
//   scan      the nearest voiced frame at or below / at or above each frame inside the tile: a max-scan and a min-scan on the
//             in-tile index through wave shuffles, the four waves joined through eight LDS words; the values come from the tile
//             in LDS.
//   carry     the last voiced frame of the tiles behind (index and value), in registers, the same in every thread.
//   ahead     when the tile's last live frame is not voiced and nothing valid is kept, the workgroup reads the tiles in front,
//             one at a time, until one holds a voiced frame (a min-reduction), and keeps its index and value until the walk has
//             passed it -- or keeps `hold`: there is none up to L-1.  It only reads.  So a frame is read at most twice, the
//             second time from L2, and LDS use does not depend on L.
//   store     every thread stores its own frame -- the one it loaded, so y may be x -- rounded once to y's dtype, and the flag.
// Rows from L to Tmax get zeros.  No frame at or past L is read.  Every offset is 64-bit.  Control flow is uniform across the
// workgroup wherever a shuffle or a barrier is reached.
// Compiled with -ffp-contract=off: the linear form is a division, a subtraction, a multiplication and an addition, each rounded.
#include <atomic>

#include "common.h"
#include "../../include/nnmnkwii_f0.h"

namespace mlpg {

namespace {

constexpr int kF0Tile = NNMK_F0_TILE;
constexpr int kF0Waves = kF0Tile / 64;

std::atomic<long long> g_f0_launches{0};

struct F0Args {
  const void *x;
  void *y, *vuv;
  long ld_x, ld_y, ld_v;
  const int32_t *lengths;
  long item0;   // the (utterance, column) pair of workgroup 0: a batch over the grid's limit goes in slices
  int Tmax, C, kind;
};

// the value of fillable frame t between the knots p < t < q with values a and b (include/nnmnkwii_f0.h)
__device__ inline double f0_fill(int kind, double a, double b, int t, int p, int q) {
  const long long dt = (long long)t - p, dq = (long long)q - p;
  switch (kind) {
    case NNMK_F0_SLINEAR:
    case NNMK_F0_LINEAR:
      return a + (b - a) * ((double)dt / (double)dq);
    case NNMK_F0_PREVIOUS:
    case NNMK_F0_ZERO:
      return a;
    case NNMK_F0_NEXT:
      return b;
    case NNMK_F0_NEAREST:
      return 2 * dt <= dq ? a : b;
    default:
      return 2 * dt < dq ? a : b;
  }
}

template <typename TX, typename TY, typename TV>
__global__ __launch_bounds__(256) void f0_interp_kernel(F0Args a) {
  __shared__ double sv[kF0Tile];
  __shared__ int wmax[kF0Waves], wmin[kF0Waves], wfirst[kF0Waves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long item = a.item0 + (long)blockIdx.x;
  const int b = (int)(item / a.C), c = (int)(item - (long)b * a.C);
  int L = a.Tmax;
  if (a.lengths) {
    const int n = a.lengths[b];
    L = n < 0 ? 0 : (n > a.Tmax ? a.Tmax : n);
  }
  const TX *__restrict__ x = (const TX *)a.x + (size_t)b * a.Tmax * a.ld_x + c;
  TY *y = a.y ? (TY *)a.y + (size_t)b * a.Tmax * a.ld_y + c : nullptr;   // (may be x: no __restrict__)
  TV *vu = a.vuv ? (TV *)a.vuv + (size_t)b * a.Tmax * a.ld_v + c : nullptr;

  int carry_idx = -1, ahead_idx = -1;
  double carry_val = 0.0, ahead_val = 0.0;
  bool hold = false;
  for (long t0 = 0; t0 < L; t0 += kF0Tile) {
    const int n = L - t0 < kF0Tile ? (int)(L - t0) : kF0Tile;
    const int t = (int)(t0 + tid);   // (used where tid < n)
    double v = 0.0;
    if (tid < n) v = (double)x[(size_t)t * a.ld_x];
    const bool voiced = v > 0.0;
    double r = v;
    if (y) {   // (the same in every workgroup of the launch)
      // ---- scan
      sv[tid] = v;
      int below = voiced ? tid : -1, above = voiced ? tid : kF0Tile;
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(below, off), d = __shfl_down(above, off);
        if (lane >= off && u > below) below = u;
        if (lane + off < 64 && d < above) above = d;
      }
      if (lane == 63) wmax[wave] = below;
      if (lane == 0) wmin[wave] = above;
      __syncthreads();
      int last = -1;
      for (int w = 0; w < kF0Waves; ++w) {
        const int hi = wmax[w], lo = wmin[w];
        if (w < wave && hi > below) below = hi;
        if (w > wave && lo < above) above = lo;
        if (hi > last) last = hi;
      }
      // ---- ahead
      if (last < n - 1 && !(hold || (long)ahead_idx >= t0 + n)) {
        bool found = false;
        for (long tm = t0 + kF0Tile; tm < L && !found; tm += kF0Tile) {
          const int nm = L - tm < kF0Tile ? (int)(L - tm) : kF0Tile;
          int hit = kF0Tile;
          if (tid < nm && (double)x[(size_t)(tm + tid) * a.ld_x] > 0.0) hit = tid;
          for (int m = 32; m >= 1; m >>= 1) {
            const int o = __shfl_xor(hit, m);
            if (o < hit) hit = o;
          }
          __syncthreads();   // (the reads of the round before are done)
          if (lane == 0) wfirst[wave] = hit;
          __syncthreads();
          for (int w = 0; w < kF0Waves; ++w)
            if (wfirst[w] < hit) hit = wfirst[w];
          if (hit < kF0Tile) {
            found = true;
            ahead_idx = (int)(tm + hit);
            ahead_val = (double)x[(size_t)ahead_idx * a.ld_x];
          }
        }
        hold = !found;
      }
      // ---- the frame's two knots
      if (tid < n) {
        bool has_p = true, has_q = true;
        int p = 0, q = L - 1;
        double pa = 0.0, qb = 0.0;
        if (below >= 0) {
          p = (int)t0 + below;
          pa = sv[below];
        } else if (carry_idx >= 0) {
          p = carry_idx;
          pa = carry_val;
        } else {
          has_p = false;
        }
        if (above < kF0Tile) {
          q = (int)t0 + above;
          qb = sv[above];
        } else if (!hold) {
          q = ahead_idx;
          qb = ahead_val;
        } else {
          has_q = false;
        }
        if (!has_p) pa = qb;
        if (!has_q) qb = pa;
        if (L < 2 || voiced || (!has_p && !has_q))
          r = v;
        else if (t == 0 || t == L - 1)
          r = pa;
        else if (v <= 0.0)
          r = f0_fill(a.kind, pa, qb, t, p, q);
      }
      if (last >= 0) {
        carry_idx = (int)t0 + last;
        carry_val = sv[last];
      }
      __syncthreads();   // (the tile in LDS is free for the next one)
    }
    // ---- store
    if (tid < n) {
      if (y) y[(size_t)t * a.ld_y] = (TY)r;
      if (vu) vu[(size_t)t * a.ld_v] = (TV)(voiced ? 1 : 0);
    }
  }
  for (long t = (long)L + tid; t < a.Tmax; t += kF0Tile) {
    if (y) y[(size_t)t * a.ld_y] = (TY)0;
    if (vu) vu[(size_t)t * a.ld_v] = (TV)0;
  }
}

int f0_refuse(const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  set_error(fmt, a, b, c);
  return MLPG_HIP_EINVAL;
}

template <typename TX, typename TY>
void f0_launch_v(hipStream_t st, int dtype_vuv, unsigned blocks, const F0Args &a) {
  if (dtype_vuv == NNMK_F0_F64)
    hipLaunchKernelGGL((f0_interp_kernel<TX, TY, double>), dim3(blocks), dim3(kF0Tile), 0, st, a);
  else
    hipLaunchKernelGGL((f0_interp_kernel<TX, TY, float>), dim3(blocks), dim3(kF0Tile), 0, st, a);
}

template <typename TX>
void f0_launch_y(hipStream_t st, int dtype_y, int dtype_vuv, unsigned blocks, const F0Args &a) {
  if (dtype_y == NNMK_F0_F64)
    f0_launch_v<TX, double>(st, dtype_vuv, blocks, a);
  else
    f0_launch_v<TX, float>(st, dtype_vuv, blocks, a);
}

int launch_f0_interp(hipStream_t st, int dtype_x, int dtype_y, int dtype_vuv, long items, F0Args a) {
  // one launch per slice of (utterance, column) pairs, each under the grid's thread limit
  const long step = items_per_launch(1, kF0Tile);
  for (long i0 = 0; i0 < items; i0 += step) {
    const unsigned cnt = (unsigned)(items - i0 < step ? items - i0 : step);
    a.item0 = i0;
    if (dtype_x == NNMK_F0_F64)
      f0_launch_y<double>(st, dtype_y, dtype_vuv, cnt, a);
    else
      f0_launch_y<float>(st, dtype_y, dtype_vuv, cnt, a);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  g_f0_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

bool f0_dtype_ok(int dtype) { return dtype == NNMK_F0_F32 || dtype == NNMK_F0_F64; }

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int nnmk_f0_abi_version(void) { return NNMK_F0_ABI_VERSION; }

__attribute__((visibility("default"))) long long nnmk_f0_launch_count(void) { return g_f0_launches.load(std::memory_order_relaxed); }

__attribute__((visibility("default"))) int nnmk_f0_interp(int device, void *stream, int dtype_x, const void *x, int64_t ld_x,
                                                          const int32_t *lengths, int B, int Tmax, int C, int kind, int dtype_y, void *y,
                                                          int64_t ld_y, int dtype_vuv, void *vuv, int64_t ld_vuv) {
  const char *who = "f0";
  if (!f0_dtype_ok(dtype_x) || !f0_dtype_ok(dtype_y) || !f0_dtype_ok(dtype_vuv))
    return f0_refuse("f0: dtype must be 0 (float32) or 1 (float64), got dtype_x = %lld, dtype_y = %lld, dtype_vuv = %lld", dtype_x, dtype_y,
                     dtype_vuv);
  if (kind < NNMK_F0_SLINEAR || kind > NNMK_F0_NEAREST_UP) return f0_refuse("f0: unknown kind %lld", kind);
  if (B < 0 || Tmax < 0 || C < 0) return f0_refuse("f0: negative size (B = %lld, Tmax = %lld, C = %lld)", B, Tmax, C);
  if (ld_x < C || (y && ld_y < C) || (vuv && ld_vuv < C))
    return f0_refuse("f0: the row strides must reach the last column (ld_x = %lld, ld_y = %lld, ld_vuv = %lld below C)", ld_x, ld_y, ld_vuv);
  if (!y && !vuv) return f0_refuse("f0: y and vuv are both NULL: nothing to compute");
  if (int rc = check_device(who, device)) return rc;
  const bool empty = B == 0 || Tmax == 0 || C == 0;
  if (!empty && !x) return f0_refuse("f0: NULL x");
  if (empty) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  F0Args a;
  a.x = x;
  a.y = y;
  a.vuv = vuv;
  a.ld_x = (long)ld_x;
  a.ld_y = (long)ld_y;
  a.ld_v = (long)ld_vuv;
  a.lengths = lengths;
  a.item0 = 0;
  a.Tmax = Tmax;
  a.C = C;
  a.kind = kind;
  return launch_f0_interp((hipStream_t)stream, dtype_x, dtype_y, dtype_vuv, (long)B * C, a);
}

}  // extern "C"
