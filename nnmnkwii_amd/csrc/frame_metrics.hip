// K13: objective metrics over padded batches (nnmk_metrics_batch, include/nnmnkwii_metrics.h; the reference's
// metrics/__init__.py:27-183: melcd, mean_squared_error, lf0_mean_squared_error, vuv_error).  tools/metrics_model.py is the
// executable specification of everything below, summation order included.
//
// One call evaluates up to 8 terms over two padded matrices x and y.  A term yields the pair (sum, count) in float64.
// metrics_kernel: a workgroup of four waves takes NNMK_METRICS_BLOCK_ROWS frames of ONE utterance, counted from its frame 0; wave
// w takes the live frames w, w + 4, ... of them.  For a frame the wave loads the columns [xmin, xmin + xspan) of x and
// [ymin, ymin + yspan) of y -- the span from the first to the last column any term names -- with its lanes over consecutive
// columns, once, as stored, into a slab of LDS of its own; it stages up to 8 of its frames at a time (as many as 64 KB of LDS per
// workgroup hold; the kernel is instantiated for 1, 2, 4 and 8 terms, whose accumulators live in registers), all their loads in flight together, and then takes them in order.  Every term reads its operands from the slab with lanes over ITS OWN
// columns d = lane, lane + 64, ...: the order of a term's additions depends on the term and the frame's index in the utterance
// alone, not on the other terms, B or Tmax.
//   FRAME_L2        a lane adds z^2 over its d in order; the 64 lane sums meet in an xor butterfly (32, 16, ..., 1: the same bits
//                   in every lane); lane 0 adds sqrt of it to its running sum.
//   SQUARED         a lane adds z^2 over the wave's frames, and within a frame over its d, into its running sum.
//   MISMATCH        the same with 1.0 per differing element (exact).
//   VOICED_SQUARED  lane 0 alone (width 1): mask test, z^2 into its sum, 1.0 into its count.
// At the end of the block the running sums of a wave's lanes meet in the butterfly, the four waves' values are added in wave order
// and the workgroup writes (sum, count) to workspace[(p * nterms + i) * 2], p = b * ceil(Tmax / BLOCK_ROWS) + block.  A workgroup
// with no live frame reads nothing and writes zeros.
// metrics_finish_kernel, one workgroup per value (term, sum | count): thread q takes the utterances [q * per, (q + 1) * per),
// per = ceil(B / 256); it adds an utterance's blocks in block order (per_utt gets that), adds its utterances in order, and the 256
// thread sums meet in a tree over adjacent threads in LDS.  The division of the work depends on (B, Tmax) and the terms alone and
// there are no atomics: the same bits on every call and on every device.
// Compiled with -ffp-contract=off: separate multiply and add, as numpy.
#include <math.h>

#include <atomic>

#include "common.h"
#include "../../include/nnmnkwii_metrics.h"

namespace mlpg {

namespace {

constexpr int kMtBlockRows = NNMK_METRICS_BLOCK_ROWS;
constexpr int kMtWaves = 4;
constexpr int kMtMaxTerms = NNMK_METRICS_MAX_TERMS;
constexpr int kMtFinSeg = 256;
constexpr int kMtStage = 8;   // frames a wave stages at once, at most

std::atomic<long long> g_metrics_launches{0};

// the terms and the spans of columns they name, by value in the kernel's arguments
struct MtTerms {
  int n;
  int xmin, xspan, ymin, yspan;
  nnmk_metrics_term t[kMtMaxTerms];
};

// A wave's LDS accesses complete in program order, so its lanes see each other's stores behind this point; the fences keep the
// compiler from moving the accesses across it.
__device__ inline void mt_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sum over the wave's 64 lanes, the same bits in every lane
__device__ inline double mt_wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}

// one staged frame: every term's additions, in the order of the terms
template <int NT, typename TX, typename TY>
__device__ inline void mt_frame(const MtTerms &ts, const TX *xs, const TY *ys, int lane, double (&sum)[NT], double (&cnt)[NT]) {
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (i >= ts.n) continue;
    const nnmk_metrics_term &t = ts.t[i];
    const TX *xt = xs + (t.x_col - ts.xmin);
    const TY *yt = ys + (t.y_col - ts.ymin);
    const double thr = t.threshold;
    const bool has_thr = thr == thr;
    if (t.kind == NNMK_METRICS_FRAME_L2) {
      double s = 0.0;
      for (int d = lane; d < t.width; d += 64) {
        const double z = (double)xt[d] - (double)yt[d];
        s += z * z;
      }
      s = mt_wave_sum(s);
      if (lane == 0) sum[i] += sqrt(s);
    } else if (t.kind == NNMK_METRICS_SQUARED) {
      for (int d = lane; d < t.width; d += 64) {
        const double z = (double)xt[d] - (double)yt[d];
        sum[i] += z * z;
      }
    } else if (t.kind == NNMK_METRICS_MISMATCH) {
      for (int d = lane; d < t.width; d += 64) {
        const double u = (double)xt[d], v = (double)yt[d];
        const bool ne = has_thr ? ((u > thr) != (v > thr)) : (u != v);
        sum[i] += ne ? 1.0 : 0.0;
      }
    } else if (lane == 0) {   // VOICED_SQUARED, width 1
      const double xm = (double)xs[t.x_mask_col - ts.xmin], ym = (double)ys[t.y_mask_col - ts.ymin];
      const bool voiced = has_thr ? (xm > thr && ym > thr) : (xm + ym >= 2.0);
      if (voiced) {
        double u = (double)xt[0], v = (double)yt[0];
        if (t.flags & NNMK_METRICS_FLAG_EXP) {
          u = exp(u);
          v = exp(v);
        }
        const double z = u - v;
        sum[i] += z * z;
        cnt[i] += 1.0;
      }
    }
  }
}

// the columns [0, span) of the wave's next nstage frames r0, r0 + 4, ... into their slabs: the loads of a column step are all
// issued before the first of them is stored
template <typename T>
__device__ inline void mt_stage(const T *__restrict__ g, long ld, int span, int r0, int nrows, int nstage, double *slabs, int slab,
                                int lane) {
  for (int c = lane; c < span; c += 64) {
    T v[kMtStage];
#pragma unroll
    for (int k = 0; k < kMtStage; ++k) {
      const int r = r0 + k * kMtWaves;
      v[k] = (k < nstage && r < nrows) ? g[(size_t)r * ld + c] : (T)0;
    }
#pragma unroll
    for (int k = 0; k < kMtStage; ++k)
      if (k < nstage && r0 + k * kMtWaves < nrows) ((T *)(slabs + (size_t)k * slab))[c] = v[k];
  }
}

// slab: doubles of LDS per staged frame (x from its start, y from xslab); nstage: frames a wave stages at once; NT: 1, 2, 4 or 8, at
// least the number of terms (the accumulators of NT terms live in registers)
template <typename TX, typename TY, int NT>
__global__ __launch_bounds__(256) void metrics_kernel(const TX *__restrict__ x, long ld_x, const TY *__restrict__ y, long ld_y,
                                                      const int32_t *__restrict__ lengths, int Tmax, int nblk, MtTerms ts,
                                                      int slab, int xslab, int nstage, double *__restrict__ ws) {
  extern __shared__ double lds[];
  __shared__ double red[kMtWaves - 1][2 * kMtMaxTerms];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned p = blockIdx.x;   // partial index b * nblk + j
  const int b = (int)(p / (unsigned)nblk), j = (int)(p - (unsigned)b * (unsigned)nblk);
  int live = Tmax;
  if (lengths) {
    live = lengths[b];
    live = live < 0 ? 0 : (live > Tmax ? Tmax : live);
  }
  const int t0 = j * kMtBlockRows;
  const int nrows = (live < t0 + kMtBlockRows ? live : t0 + kMtBlockRows) - t0;   // live frames of this workgroup
  double *out = ws + (size_t)p * ts.n * 2;
  if (nrows <= 0) {
    if (tid < 2 * ts.n) out[tid] = 0.0;
    return;
  }
  double sum[NT], cnt[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) sum[i] = cnt[i] = 0.0;
  double *slabs = lds + (size_t)wave * nstage * slab;
  const TX *x0 = x + ((size_t)b * Tmax + t0) * ld_x + ts.xmin;   // frame t0 of utterance b, column xmin
  const TY *y0 = y + ((size_t)b * Tmax + t0) * ld_y + ts.ymin;
  for (int r0 = wave; r0 < nrows; r0 += kMtWaves * nstage) {
    mt_stage(x0, ld_x, ts.xspan, r0, nrows, nstage, slabs, slab, lane);
    mt_stage(y0, ld_y, ts.yspan, r0, nrows, nstage, slabs + xslab, slab, lane);
    mt_wave_sync();
    for (int k = 0; k < nstage && r0 + k * kMtWaves < nrows; ++k)   // the wave's frames in order
      mt_frame<NT>(ts, (const TX *)(slabs + (size_t)k * slab), (const TY *)(slabs + (size_t)k * slab + xslab), lane, sum, cnt);
    mt_wave_sync();   // the slabs are free for the wave's next frames
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (i >= ts.n) continue;
    sum[i] = mt_wave_sum(sum[i]);
    cnt[i] = mt_wave_sum(cnt[i]);
    if (wave > 0 && lane == 0) {
      red[wave - 1][2 * i] = sum[i];
      red[wave - 1][2 * i + 1] = cnt[i];
    }
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      if (i >= ts.n) continue;
      double s = sum[i], c = cnt[i];
      for (int w = 0; w < kMtWaves - 1; ++w) {
        s += red[w][2 * i];
        c += red[w][2 * i + 1];
      }
      const int kind = ts.t[i].kind;
      if (kind == NNMK_METRICS_FRAME_L2) c = (double)nrows;
      if (kind == NNMK_METRICS_SQUARED || kind == NNMK_METRICS_MISMATCH) c = (double)nrows * (double)ts.t[i].width;
      out[2 * i] = s;
      out[2 * i + 1] = c;
    }
  }
}

// per_utt may be NULL
__global__ __launch_bounds__(256) void metrics_finish_kernel(const double *__restrict__ ws, int B, int nblk, int nv,
                                                             double *__restrict__ per_utt, double *__restrict__ totals) {
  __shared__ double sh[kMtFinSeg];
  const int q = threadIdx.x, v = blockIdx.x;   // v: term * 2 + (0 sum | 1 count)
  const long per = ((long)B + kMtFinSeg - 1) / kMtFinSeg;
  const long b0 = q * per, b1 = b0 + per < B ? b0 + per : B;
  double s = 0.0;
  for (long b = b0; b < b1; ++b) {
    double u = 0.0;
    for (int j = 0; j < nblk; ++j) u += ws[((size_t)b * nblk + j) * nv + v];
    if (per_utt) per_utt[(size_t)b * nv + v] = u;
    s += u;
  }
  sh[q] = s;
  for (int h = 1; h < kMtFinSeg; h *= 2) {
    __syncthreads();
    if (q % (2 * h) == 0) {
      s += sh[q + h];
      sh[q] = s;
    }
  }
  if (q == 0) totals[v] = s;
}

int64_t mt_blocks(int Tmax) { return ((int64_t)Tmax + kMtBlockRows - 1) / kMtBlockRows; }

int64_t mt_workspace_bytes(int B, int Tmax, int nterms) {
  if (B < 0 || Tmax < 0 || nterms < 0) return -1;
  const int64_t P = (int64_t)B * mt_blocks(Tmax);   // < 2^31 * 2^23
  const int64_t per = (int64_t)nterms * 16;         // < 2^35
  if (P != 0 && per > INT64_MAX / P) return -1;
  return P * per;
}

template <typename TX, typename TY>
void mt_launch_nt(hipStream_t st, unsigned blocks, size_t lds_bytes, const TX *x, long ld_x, const TY *y, long ld_y, const int32_t *lengths,
                  int Tmax, int nblk, const MtTerms &ts, int slab, int xslab, int nstage, double *ws) {
#define MT_LAUNCH(NT)                                                                                                               \
  hipLaunchKernelGGL((metrics_kernel<TX, TY, NT>), dim3(blocks), dim3(256), lds_bytes, st, x, ld_x, y, ld_y, lengths, Tmax, nblk, ts, \
                     slab, xslab, nstage, ws)
  if (ts.n <= 1)
    MT_LAUNCH(1);
  else if (ts.n <= 2)
    MT_LAUNCH(2);
  else if (ts.n <= 4)
    MT_LAUNCH(4);
  else
    MT_LAUNCH(8);
#undef MT_LAUNCH
}

template <typename TX>
void mt_launch_y(hipStream_t st, int dtype_y, unsigned blocks, size_t lds_bytes, const TX *x, long ld_x, const void *y, long ld_y,
                 const int32_t *lengths, int Tmax, int nblk, const MtTerms &ts, int slab, int xslab, int nstage, double *ws) {
  if (dtype_y == NNMK_METRICS_F64)
    mt_launch_nt(st, blocks, lds_bytes, x, ld_x, (const double *)y, ld_y, lengths, Tmax, nblk, ts, slab, xslab, nstage, ws);
  else
    mt_launch_nt(st, blocks, lds_bytes, x, ld_x, (const float *)y, ld_y, lengths, Tmax, nblk, ts, slab, xslab, nstage, ws);
}

int launch_metrics(hipStream_t st, int dtype_x, const void *x, long ld_x, int dtype_y, const void *y, long ld_y, const int32_t *lengths,
                   int B, int Tmax, const MtTerms &ts, int xslab, int yslab, double *per_utt, double *totals, double *ws) {
  const int nblk = (int)mt_blocks(Tmax);
  const long P = (long)B * nblk;
  if (P > 0) {
    const int slab = xslab + yslab;   // doubles of LDS per staged frame
    int nstage = NNMK_METRICS_MAX_ROW_BYTES / (slab * 8);   // four waves' slabs and the static 384 bytes: at most 64 KB of LDS per workgroup
    nstage = nstage < 1 ? 1 : (nstage > kMtStage ? kMtStage : nstage);
    const size_t lds_bytes = (size_t)kMtWaves * nstage * slab * 8;
    if (dtype_x == NNMK_METRICS_F64)
      mt_launch_y(st, dtype_y, (unsigned)P, lds_bytes, (const double *)x, ld_x, y, ld_y, lengths, Tmax, nblk, ts, slab, xslab, nstage, ws);
    else
      mt_launch_y(st, dtype_y, (unsigned)P, lds_bytes, (const float *)x, ld_x, y, ld_y, lengths, Tmax, nblk, ts, slab, xslab, nstage, ws);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)(2 * ts.n)), dim3(kMtFinSeg), 0, st, (const double *)ws, B, nblk, 2 * ts.n,
                     per_utt, totals);
  MLPG_HIP_CHECK(hipGetLastError());
  g_metrics_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

int mt_refuse(const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  set_error(fmt, a, b, c, d);
  return MLPG_HIP_EINVAL;
}

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int nnmk_metrics_abi_version(void) { return NNMK_METRICS_ABI_VERSION; }

__attribute__((visibility("default"))) int64_t nnmk_metrics_workspace(int B, int Tmax, int nterms) {
  return mt_workspace_bytes(B, Tmax, nterms);
}

__attribute__((visibility("default"))) long long nnmk_metrics_launch_count(void) {
  return g_metrics_launches.load(std::memory_order_relaxed);
}

__attribute__((visibility("default"))) int nnmk_metrics_batch(int device, void *stream, int dtype_x, const void *x, int64_t ld_x,
                                                              int dtype_y, const void *y, int64_t ld_y, const int32_t *lengths, int B,
                                                              int Tmax, const nnmk_metrics_term *terms, int nterms, double *per_utt,
                                                              double *totals, void *workspace, int64_t workspace_bytes) {
  const char *who = "metrics";
  if ((dtype_x != NNMK_METRICS_F32 && dtype_x != NNMK_METRICS_F64) || (dtype_y != NNMK_METRICS_F32 && dtype_y != NNMK_METRICS_F64))
    return mt_refuse("metrics: dtype must be 0 (float32) or 1 (float64), got dtype_x = %lld, dtype_y = %lld", dtype_x, dtype_y);
  if (B < 0 || Tmax < 0 || ld_x < 0 || ld_y < 0)
    return mt_refuse("metrics: negative size (B = %lld, Tmax = %lld, ld_x = %lld, ld_y = %lld)", B, Tmax, ld_x, ld_y);
  if (nterms < 1 || nterms > kMtMaxTerms) return mt_refuse("metrics: nterms must be in 1 .. %lld, got %lld", kMtMaxTerms, nterms);
  if (!terms) return mt_refuse("metrics: NULL terms");
  MtTerms ts;
  ts.n = nterms;
  int64_t xlo = INT64_MAX, xhi = 0, ylo = INT64_MAX, yhi = 0;   // the spans of columns the terms name
  for (int i = 0; i < nterms; ++i) {
    const nnmk_metrics_term &t = terms[i];
    if (t.kind < NNMK_METRICS_FRAME_L2 || t.kind > NNMK_METRICS_MISMATCH) return mt_refuse("metrics: term %lld: unknown kind %lld", i, t.kind);
    if (t.width < 1) return mt_refuse("metrics: term %lld: width must be at least 1, got %lld", i, t.width);
    if (t.x_col < 0 || t.y_col < 0) return mt_refuse("metrics: term %lld: negative column (x_col = %lld, y_col = %lld)", i, t.x_col, t.y_col);
    if ((int64_t)t.x_col + t.width > ld_x || (int64_t)t.y_col + t.width > ld_y)
      return mt_refuse("metrics: term %lld: the row strides must reach the term's last column (ld_x = %lld, ld_y = %lld)", i, ld_x, ld_y);
    const bool voiced = t.kind == NNMK_METRICS_VOICED_SQUARED;
    if (t.flags & ~(voiced ? NNMK_METRICS_FLAG_EXP : 0)) return mt_refuse("metrics: term %lld: unknown flags %lld", i, t.flags);
    xlo = t.x_col < xlo ? t.x_col : xlo;
    ylo = t.y_col < ylo ? t.y_col : ylo;
    xhi = (int64_t)t.x_col + t.width > xhi ? (int64_t)t.x_col + t.width : xhi;
    yhi = (int64_t)t.y_col + t.width > yhi ? (int64_t)t.y_col + t.width : yhi;
    if (voiced) {
      if (t.width != 1) return mt_refuse("metrics: term %lld: VOICED_SQUARED takes width 1, got %lld", i, t.width);
      if (t.x_mask_col < 0 || t.x_mask_col >= ld_x || t.y_mask_col < 0 || t.y_mask_col >= ld_y)
        return mt_refuse("metrics: term %lld: mask columns out of range (x_mask_col = %lld, y_mask_col = %lld)", i, t.x_mask_col, t.y_mask_col);
      xlo = t.x_mask_col < xlo ? t.x_mask_col : xlo;
      ylo = t.y_mask_col < ylo ? t.y_mask_col : ylo;
      xhi = t.x_mask_col + 1 > xhi ? t.x_mask_col + 1 : xhi;
      yhi = t.y_mask_col + 1 > yhi ? t.y_mask_col + 1 : yhi;
    }
    ts.t[i] = t;
  }
  for (int i = nterms; i < kMtMaxTerms; ++i) ts.t[i] = nnmk_metrics_term{0, 0, 0, 0, 0, 0, 0, 0.0};
  ts.xmin = (int)xlo;
  ts.xspan = (int)(xhi - xlo);
  ts.ymin = (int)ylo;
  ts.yspan = (int)(yhi - ylo);
  const int64_t xslab = ((xhi - xlo) * (dtype_x == NNMK_METRICS_F64 ? 8 : 4) + 7) / 8, yslab = ((yhi - ylo) * (dtype_y == NNMK_METRICS_F64 ? 8 : 4) + 7) / 8;
  if ((xslab + yslab) * 8 > NNMK_METRICS_MAX_ROW_BYTES)
    return mt_refuse("metrics: the terms span %lld bytes of a frame of x and y, at most %lld fit", (xslab + yslab) * 8, NNMK_METRICS_MAX_ROW_BYTES);
  const int64_t need = mt_workspace_bytes(B, Tmax, nterms);
  if (need < 0 || (int64_t)B * mt_blocks(Tmax) > 16777215LL /* 2^24 - 1 workgroups of 256 threads: a grid is 32 bits of threads, a larger one runs truncated and reports nothing */)
    return mt_refuse("metrics: the batch is too large for one grid (B = %lld, Tmax = %lld)", B, Tmax);
  if (int rc = check_device(who, device)) return rc;
  if (!totals) return mt_refuse("metrics: NULL totals");
  if (need > 0 && (!x || !y || !workspace)) return mt_refuse("metrics: NULL data pointer (x, y and workspace are required)");
  if (need > 0 && (uintptr_t)workspace % 8 != 0) return mt_refuse("metrics: the workspace must be 8-byte aligned");
  if (workspace_bytes < need)
    return mt_refuse("metrics: the workspace holds %lld bytes, nnmk_metrics_workspace asks for %lld", workspace_bytes, need);
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_metrics((hipStream_t)stream, dtype_x, x, (long)ld_x, dtype_y, y, (long)ld_y, lengths, B, Tmax, ts, (int)xslab, (int)yslab,
                        per_utt, totals, (double *)workspace);
}

}  // extern "C"
