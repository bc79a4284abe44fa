// K12: corpus normalisation (mlpg_hip_column_stats, mlpg_hip_column_affine; the reference's preprocessing/generic.py:496-829:
// meanvar / meanstd / minmax and scale / inv_scale / minmax_scale / inv_minmax_scale).  tools/norm_model.py is the executable
// specification of everything below, summation order included.
//
// Statistics.  One pass over a padded (B, Tmax, .) batch gives, per column, the count of live frames, their mean,
// M2 = sum (x - mean)^2, min and max.  Lanes run over 64 consecutive columns (a wave's load of a row is contiguous); a workgroup
// of four waves takes MLPG_HIP_COLSTATS_BLOCK_ROWS frames of ONE utterance and one group of 64 columns.  Its live frames are cut
// into chunks of MLPG_HIP_COLSTATS_CHUNK_ROWS; wave w takes chunks w, w + 4, ...  A lane holds a chunk of its column in
// registers and forms  mean_c = K + (sum (x - K)) / n,  M2_c = sum (x - mean_c)^2,  both summed in row order, where K is the
// column's value in the workgroup's first frame; it merges the chunk into its running state with Chan's pairwise update
// (cs_merge).  The shift by K makes a column that is constant over the live frames come out with mean == the constant and
// M2 == 0 exactly: every x - K is 0, every chunk mean is K, every delta of every merge is 0.  Two divisions per chunk.
// The waves' states meet in LDS and are merged in wave order; the workgroup writes its partial (count, mean, M2, min, max) to
// workspace[(p * 5 + s) * D + d], p = b * ceil(Tmax / BLOCK_ROWS) + block.  A workgroup whose frames are all padding reads
// nothing and writes the empty partial (0, 0, 0, +inf, -inf).
// colstats_finish_kernel merges the partials of a column: 64 segments of consecutive partials, each merged in order by one
// thread (segment 0 starts from the incoming state), then a tree over adjacent segments in LDS.  The division of the work
// depends on (B, Tmax, D) and these constants alone -- not on the device -- and there are no atomics: the same bits on every
// call and on every device.  If M2 comes out NaN (a non-finite live value) the mean is set to NaN with it.
// min / max propagate NaN as np.minimum / np.maximum do (fmin / fmax would drop it).
//
// Apply.  colaffine_kernel: y = (x - c[d]) / a[d] (mode 0) or y = a[d] * x + c[d] (mode 1) in float64, one rounding to the
// output type; rows past an utterance's length are never read and written as exact zeros in columns 0 .. D - 1; columns past D
// are never touched.  An element is read and written by the same thread: y may be x.
// Compiled with -ffp-contract=off: separate multiply and add, as numpy.
#include <math.h>

#include "common.h"

namespace mlpg {

namespace {

constexpr int kCsChunk = MLPG_HIP_COLSTATS_CHUNK_ROWS;
constexpr int kCsBlockRows = MLPG_HIP_COLSTATS_BLOCK_ROWS;
constexpr int kCsWaves = 4;
constexpr int kCsFinSeg = 64, kCsFinCols = 4;   // finish: 64 segments x 4 columns per workgroup
static_assert(kCsBlockRows % (kCsChunk * kCsWaves) == 0, "every wave of a full workgroup takes the same number of chunks");

struct ColStat {
  double n, mean, m2, mn, mx;
};

__device__ inline ColStat cs_empty() { return ColStat{0.0, 0.0, 0.0, INFINITY, -INFINITY}; }

// a <- a merged with b (a first): Chan, Golub, LeVeque's pairwise update; the extrema as np.minimum / np.maximum
__device__ inline void cs_merge(ColStat &a, const ColStat &b) {
  a.mn = (b.mn < a.mn || b.mn != b.mn) ? b.mn : a.mn;
  a.mx = (b.mx > a.mx || b.mx != b.mx) ? b.mx : a.mx;
  if (b.n == 0.0) return;
  if (a.n == 0.0) {
    a.n = b.n;
    a.mean = b.mean;
    a.m2 = b.m2;
    return;
  }
  const double n = a.n + b.n, delta = b.mean - a.mean, w = b.n / n;
  a.mean = a.mean + delta * w;
  a.m2 = (a.m2 + b.m2) + (delta * delta) * (a.n * w);
  a.n = n;
}

template <typename TX>
__global__ __launch_bounds__(256) void colstats_kernel(const TX *__restrict__ x, long ld_x, const int32_t *__restrict__ lengths,
                                                       int Tmax, int D, int nblk, int ncg, double *__restrict__ ws) {
  __shared__ double red[5][kCsWaves - 1][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned id = blockIdx.x;
  const int cg = (int)(id % (unsigned)ncg);
  const unsigned p = id / (unsigned)ncg;   // partial index b * nblk + j
  const int b = (int)(p / (unsigned)nblk), j = (int)(p - (unsigned)b * (unsigned)nblk);
  int live = Tmax;
  if (lengths) {
    live = lengths[b];
    live = live < 0 ? 0 : (live > Tmax ? Tmax : live);
  }
  const int t0 = j * kCsBlockRows;
  const int nrows = (live < t0 + kCsBlockRows ? live : t0 + kCsBlockRows) - t0;   // live frames of this workgroup
  const int d = cg * 64 + lane;
  const bool act = d < D;
  ColStat s = cs_empty();
  if (act && nrows > 0) {
    const TX *col = x + ((size_t)b * Tmax + t0) * ld_x + d;   // frame t0 of utterance b, column d
    const TX kraw = col[0];
    const double K = (double)kraw;
    // a chunk in registers as stored; a frame past the chunk's end holds K (it adds an exact zero to the sum)
    TX cur[kCsChunk];
    int r0 = wave * kCsChunk;
#pragma unroll
    for (int i = 0; i < kCsChunk; ++i) cur[i] = r0 + i < nrows ? col[(size_t)(r0 + i) * ld_x] : kraw;
    for (; r0 < nrows; r0 += kCsWaves * kCsChunk) {
      const int n = nrows - r0 < kCsChunk ? nrows - r0 : kCsChunk;
      ColStat c = cs_empty();
      double sum = 0.0;
#pragma unroll
      for (int i = 0; i < kCsChunk; ++i) {
        const double v = (double)cur[i];
        sum += v - K;
        if (i < n) {
          c.mn = (v < c.mn || v != v) ? v : c.mn;
          c.mx = (v > c.mx || v != v) ? v : c.mx;
        }
      }
      c.n = (double)n;
      c.mean = K + sum / c.n;
#pragma unroll
      for (int i = 0; i < kCsChunk; ++i) {
        const double e = (double)cur[i] - c.mean;
        c.m2 += i < n ? e * e : 0.0;
      }
      cs_merge(s, c);
      // the wave's next chunk: issued behind the merge, so that its loads are under way across the loop's back edge (measured:
      // float32 0.19 ms against 0.46 ms with the loads at the loop's head)
      const int rn = r0 + kCsWaves * kCsChunk;
#pragma unroll
      for (int i = 0; i < kCsChunk; ++i) cur[i] = rn + i < nrows ? col[(size_t)(rn + i) * ld_x] : kraw;
    }
  }
  if (wave > 0) {
    red[0][wave - 1][lane] = s.n;
    red[1][wave - 1][lane] = s.mean;
    red[2][wave - 1][lane] = s.m2;
    red[3][wave - 1][lane] = s.mn;
    red[4][wave - 1][lane] = s.mx;
  }
  __syncthreads();
  if (wave == 0 && act) {
    for (int w = 0; w < kCsWaves - 1; ++w) cs_merge(s, ColStat{red[0][w][lane], red[1][w][lane], red[2][w][lane], red[3][w][lane], red[4][w][lane]});
    double *o = ws + (size_t)p * 5 * D + d;
    o[0] = s.n;
    o[(size_t)D] = s.mean;
    o[(size_t)2 * D] = s.m2;
    o[(size_t)3 * D] = s.mn;
    o[(size_t)4 * D] = s.mx;
  }
}

// state_in may be state_out: a column's incoming state is read by the thread that later writes it, before it does
__global__ __launch_bounds__(256) void colstats_finish_kernel(const double *__restrict__ ws, long P, int D, const double *state_in,
                                                              double *state_out) {
  __shared__ double sh[5][kCsFinSeg][kCsFinCols];
  const int tid = threadIdx.x, dl = tid % kCsFinCols, q = tid / kCsFinCols;
  const int d = (int)blockIdx.x * kCsFinCols + dl;
  const bool act = d < D;
  ColStat s = cs_empty();
  if (act) {
    if (q == 0 && state_in)
      s = ColStat{state_in[d], state_in[(size_t)D + d], state_in[(size_t)2 * D + d], state_in[(size_t)3 * D + d],
                  state_in[(size_t)4 * D + d]};
    const long per = (P + kCsFinSeg - 1) / kCsFinSeg;
    const long p0 = q * per, p1 = p0 + per < P ? p0 + per : P;
    for (long p = p0; p < p1; ++p) {
      const double *o = ws + (size_t)p * 5 * D + d;
      cs_merge(s, ColStat{o[0], o[(size_t)D], o[(size_t)2 * D], o[(size_t)3 * D], o[(size_t)4 * D]});
    }
  }
  sh[0][q][dl] = s.n;
  sh[1][q][dl] = s.mean;
  sh[2][q][dl] = s.m2;
  sh[3][q][dl] = s.mn;
  sh[4][q][dl] = s.mx;
  for (int h = 1; h < kCsFinSeg; h *= 2) {
    __syncthreads();
    if (q % (2 * h) == 0) {
      cs_merge(s, ColStat{sh[0][q + h][dl], sh[1][q + h][dl], sh[2][q + h][dl], sh[3][q + h][dl], sh[4][q + h][dl]});
      sh[0][q][dl] = s.n;
      sh[1][q][dl] = s.mean;
      sh[2][q][dl] = s.m2;
      sh[3][q][dl] = s.mn;
      sh[4][q][dl] = s.mx;
    }
  }
  if (q == 0 && act) {
    if (s.m2 != s.m2 || s.mean != s.mean) s.mean = s.m2 = NAN;   // a non-finite live value: both are NaN
    state_out[d] = s.n;
    state_out[(size_t)D + d] = s.mean;
    state_out[(size_t)2 * D + d] = s.m2;
    state_out[(size_t)3 * D + d] = s.mn;
    state_out[(size_t)4 * D + d] = s.mx;
  }
}

constexpr int kCaRows = 64;   // rows per workgroup of the apply kernel: wave w takes rows w, w + 4, ...
// The grid of a launch is 32 bits of THREADS: with 256 threads per workgroup at most 2^24 - 1 workgroups.  A launch asked for more
// runs (blocks * 256) mod 2^32 threads and reports nothing -- 2^31 + 32768 rows came back with the first 32768 done.  Beyond this
// many row blocks the workgroups walk the blocks with the grid as their stride.
constexpr long kCaMaxBlocks = (1L << 24) - 1;
constexpr long kCsMaxBlocks = (1L << 24) - 1;  // the statistics kernel takes one workgroup per partial and column group: more are refused

// One row at a time per wave, the lanes over its columns.  Measured against two forms that keep eight rows of a column in
// flight per lane: this one is the fastest of the three.
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void colaffine_kernel(const TX *x, long ld_x, TY *y, long ld_y, const int32_t *__restrict__ lengths,
                                                        long rows, long stride, int Tmax, int D, int mode,
                                                        const double *__restrict__ a, const double *__restrict__ c) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long nblk = (rows + kCaRows - 1) / kCaRows;
  // stride: the workgroups of the launch.  An argument and not gridDim.x because this file is also compiled for the host
  // (tests/test_norm_host_cpu.py), against a shim that defines threadIdx and blockIdx only.  One pass unless the batch has more
  // than kCaMaxBlocks row blocks.
  for (long blk = blockIdx.x; blk < nblk; blk += stride) {
    const long n0 = blk * kCaRows;
    for (int r = wave; r < kCaRows; r += 4) {
      const long n = n0 + r;
      if (n >= rows) break;
      const long b = n / Tmax;
      const int t = (int)(n - b * Tmax);
      int live = Tmax;
      if (lengths) {
        live = lengths[b];
        live = live < 0 ? 0 : (live > Tmax ? Tmax : live);
      }
      TY *yr = y + (size_t)n * ld_y;
      if (t >= live) {
        for (int d = lane; d < D; d += 64) yr[d] = (TY)0;
        continue;
      }
      const TX *xr = x + (size_t)n * ld_x;
      for (int d = lane; d < D; d += 64) {
        const double v = (double)xr[d];
        yr[d] = (TY)(mode == 0 ? (v - c[d]) / a[d] : a[d] * v + c[d]);
      }
    }
  }
}

// partials of a (B, Tmax) batch: B * ceil(Tmax / BLOCK_ROWS); -1 if that, or the workspace's byte count, does not fit
int64_t cs_partials(int B, int Tmax) {
  const int64_t nblk = ((int64_t)Tmax + kCsBlockRows - 1) / kCsBlockRows;
  return (int64_t)B * nblk;   // < 2^31 * 2^22
}

int64_t cs_workspace_bytes(int B, int Tmax, int D) {
  if (B < 0 || Tmax < 0 || D < 0) return -1;
  const int64_t P = cs_partials(B, Tmax);
  const int64_t per = (int64_t)D * 5 * 8;   // < 2^37
  if (P != 0 && per > INT64_MAX / P) return -1;
  return P * per;
}

}  // namespace

int launch_colstats(hipStream_t st, int dtype, const void *x, long ld_x, const int32_t *lengths, int B, int Tmax, int D,
                    const double *state_in, double *state_out, double *ws) {
  const int nblk = (Tmax + kCsBlockRows - 1) / kCsBlockRows, ncg = (D + 63) / 64;
  const long P = (long)B * nblk;
  if (P > 0) {
    const unsigned blocks = (unsigned)(P * ncg);
    if (dtype == MLPG_HIP_F64)
      hipLaunchKernelGGL(colstats_kernel<double>, dim3(blocks), dim3(256), 0, st, (const double *)x, ld_x, lengths, Tmax, D, nblk, ncg, ws);
    else
      hipLaunchKernelGGL(colstats_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float *)x, ld_x, lengths, Tmax, D, nblk, ncg, ws);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(colstats_finish_kernel, dim3((unsigned)((D + kCsFinCols - 1) / kCsFinCols)), dim3(256), 0, st, (const double *)ws, P, D,
                     state_in, state_out);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountColStats);
  return 0;
}

template <typename TX>
static void launch_colaffine_out(hipStream_t st, int out_dtype, unsigned blocks, const TX *x, long ld_x, void *y, long ld_y,
                                 const int32_t *lengths, long rows, int Tmax, int D, int mode, const double *a, const double *c) {
  if (out_dtype == MLPG_HIP_F64)
    hipLaunchKernelGGL((colaffine_kernel<TX, double>), dim3(blocks), dim3(256), 0, st, x, ld_x, (double *)y, ld_y, lengths, rows, (long)blocks, Tmax, D, mode, a, c);
  else
    hipLaunchKernelGGL((colaffine_kernel<TX, float>), dim3(blocks), dim3(256), 0, st, x, ld_x, (float *)y, ld_y, lengths, rows, (long)blocks, Tmax, D, mode, a, c);
}

int launch_colaffine(hipStream_t st, int in_dtype, int out_dtype, int mode, const void *x, long ld_x, void *y, long ld_y,
                     const int32_t *lengths, int B, int Tmax, int D, const double *a, const double *c) {
  const long rows = (long)B * Tmax;
  const long nblk = (rows + kCaRows - 1) / kCaRows;
  const unsigned blocks = (unsigned)(nblk < kCaMaxBlocks ? nblk : kCaMaxBlocks);
  if (in_dtype == MLPG_HIP_F64)
    launch_colaffine_out(st, out_dtype, blocks, (const double *)x, ld_x, y, ld_y, lengths, rows, Tmax, D, mode, a, c);
  else
    launch_colaffine_out(st, out_dtype, blocks, (const float *)x, ld_x, y, ld_y, lengths, rows, Tmax, D, mode, a, c);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountColAffine);
  return 0;
}

}  // namespace mlpg

using namespace mlpg;

namespace {

int refuse_shape(const char *who, int B, int Tmax, int D) {
  if (B < 0 || Tmax < 0 || D < 0) {
    set_error("%s: negative size (B = %d, Tmax = %d, D = %d)", who, B, Tmax, D);
    return MLPG_HIP_EINVAL;
  }
  return 0;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t mlpg_hip_column_stats_workspace(int B, int Tmax, int D) {
  return cs_workspace_bytes(B, Tmax, D);
}

__attribute__((visibility("default"))) int mlpg_hip_column_stats(int device, void *stream, int dtype, const void *x, int64_t ld_x,
                                                                 const int32_t *lengths, int B, int Tmax, int D, const double *state_in,
                                                                 double *state_out, void *workspace, int64_t workspace_bytes) {
  const char *who = "column_stats";
  if (int rc = check_dtype(who, dtype)) return rc;
  if (int rc = refuse_shape(who, B, Tmax, D)) return rc;
  if (ld_x < D) {
    set_error("%s: the row stride must be at least D = %d (got ld_x = %lld)", who, D, (long long)ld_x);
    return MLPG_HIP_EINVAL;
  }
  const int64_t need = cs_workspace_bytes(B, Tmax, D);
  // (need >= 0: partials * 40 D fits 63 bits, so partials * ceil(D / 64) does)
  if (need < 0 || cs_partials(B, Tmax) * ((D + 63) / 64) > kCsMaxBlocks) {
    set_error("%s: the batch is too large for one call (B = %d, Tmax = %d, D = %d)", who, B, Tmax, D);
    return MLPG_HIP_EINVAL;
  }
  // the finish step takes a workgroup of 256 threads per kCsFinCols columns, whatever the batch (an empty one included)
  if (((int64_t)D + kCsFinCols - 1) / kCsFinCols > kCsMaxBlocks) {
    set_error("%s: D = %d columns are more than the %ld workgroups of 256 threads (%d columns each) one launch of the finish step takes",
              who, D, kCsMaxBlocks, kCsFinCols);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  if (D == 0) return 0;
  if (!state_out) {
    set_error("%s: NULL state_out", who);
    return MLPG_HIP_EINVAL;
  }
  if (need > 0 && (!x || !workspace)) {
    set_error("%s: NULL data pointer (x and workspace are required)", who);
    return MLPG_HIP_EINVAL;
  }
  if (need > 0 && (uintptr_t)workspace % 8 != 0) {
    set_error("%s: the workspace must be 8-byte aligned", who);
    return MLPG_HIP_EINVAL;
  }
  if (workspace_bytes < need) {
    set_error("%s: the workspace holds %lld bytes, mlpg_hip_column_stats_workspace asks for %lld", who, (long long)workspace_bytes,
              (long long)need);
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_colstats((hipStream_t)stream, dtype, x, (long)ld_x, lengths, B, Tmax, D, state_in, state_out, (double *)workspace);
}

__attribute__((visibility("default"))) int mlpg_hip_column_affine(int device, void *stream, int in_dtype, int out_dtype, int mode,
                                                                  const void *x, int64_t ld_x, void *y, int64_t ld_y,
                                                                  const int32_t *lengths, int B, int Tmax, int D, const double *a,
                                                                  const double *c) {
  const char *who = "column_affine";
  if (int rc = check_dtype(who, in_dtype)) return rc;
  if (int rc = check_dtype(who, out_dtype)) return rc;
  if (mode != 0 && mode != 1) {
    set_error("%s: mode must be 0 ((x - c) / a) or 1 (a x + c), got %d", who, mode);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = refuse_shape(who, B, Tmax, D)) return rc;
  if (ld_x < D || ld_y < D) {
    set_error("%s: row strides must be at least D = %d (got ld_x = %lld, ld_y = %lld)", who, D, (long long)ld_x, (long long)ld_y);
    return MLPG_HIP_EINVAL;
  }
  // (the apply kernel walks its row blocks, any number of them: what this refuses is a row count beyond 2^37)
  if (((int64_t)B * Tmax + kCaRows - 1) / kCaRows > 2147483647LL) {
    set_error("%s: the batch is too large for one call (B = %d, Tmax = %d)", who, B, Tmax);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || Tmax == 0 || D == 0) return 0;
  if (!x || !y || !a || !c) {
    set_error("%s: NULL data pointer (x, y, a and c are required)", who);
    return MLPG_HIP_EINVAL;
  }
  if (y == x && (in_dtype != out_dtype || ld_x != ld_y)) {
    set_error("%s: in place (y == x) needs one dtype and equal row strides", who);
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_colaffine((hipStream_t)stream, in_dtype, out_dtype, mode, x, (long)ld_x, y, (long)ld_y, lengths, B, Tmax, D, a, c);
}

}  // extern "C"
