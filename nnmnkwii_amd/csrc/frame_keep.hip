// K18: silence frames dropped over a padded batch (nnmk_sil_frame_counts, nnmk_sil_expand and nnmk_sil_gather,
// include/nnmnkwii_silence.h; the reference's np.delete(X, labels.silence_frame_indices(regex), axis=0) for the linguistic and the
// acoustic matrix of an utterance).  The keep mask is constant over a phone, so the removal needs no scan over frames: the
// kept-frame offset of a state is a prefix sum over the utterance's states.  tools/silence_model.py is the executable
// specification of everything below.
//
// keep_expand_kernel and keep_gather_kernel: a workgroup of four waves takes NNMK_SIL_BLOCK_ROWS OUTPUT rows of ONE utterance.
//   scan      as csrc/frame_expand.hip's, with two sums: every thread turns a run of consecutive states' durations into frames
//             and adds them up twice (int64), all of them and those of phones that are not flagged; the 256 pairs meet in two wave
//             scans (shuffles) and an eight-entry table in LDS; the thread then writes both running counts BEHIND each of its
//             states to LDS as int32, saturated at 2^31 - 1 (an output row and a source frame are below 2^31 - 1, so a saturated
//             entry still compares right).
//   describe  thread r < 64 finds the state of output row t0 + r by binary search on the KEPT counts (the first state whose kept
//             count exceeds the row: a flagged state and a state of 0 frames add nothing and are never found).  Its source frame
//             is the frame count in front of that state plus the offset inside it.  expand: the phone's S durations give fn, base
//             and pd of the ORIGINAL phone, and the row's phone index and F sub-phone values (float64) go to LDS.  gather: the
//             source frame goes to LDS; past K_b the rows continue with frame T_b + (r - K_b) (np.delete keeps what lies behind
//             the labels' frames); a frame at or past len_src[b] does not exist and its row is a pad row.
//   store     csrc/frame_expand.hip's: wave w takes rows 16 w .. 16 w + 15 of the block, its lanes consecutive columns
//             c = lane, lane + 64, ...; the gather reads whole source rows the same way.  Pad rows get zeros.
// Workgroup 0 of an utterance writes lengths_out.  No workgroup reads a duration, a phone row or a flag at or past
// num_phones[b], or a source row at or past len_src[b], and none stores outside its own rows' columns.  Every offset is 64-bit.
// Control flow is uniform wherever a shuffle or a barrier is reached; no atomics, no workgroup waits for another.
// keep_counts_kernel: one workgroup per utterance adds its states' frames (int64), all and kept.
//
// The duration-to-frames rule and the sub-phone columns are restated from csrc/frame_expand.hip, which stays self-contained
// (tests compile it from a fixed list of files); tests/test_silence_host_cpu.py ties both copies to the one model.
// Compiled with -ffp-contract=off: the affine map is a multiplication and an addition, each rounded, as numpy.
#include <math.h>

#include <atomic>

#include "common.h"
#include "../../include/nnmnkwii_silence.h"

extern __shared__ double sk_lds[];

namespace mlpg {

namespace {

constexpr int kSkBlockRows = NNMK_SIL_BLOCK_ROWS;
constexpr int kSkWaves = 4;
constexpr int kSkRowsPerWave = kSkBlockRows / kSkWaves;
constexpr int kSkMaxF = 9;
constexpr int kSkIntMax = 2147483647;
constexpr unsigned kSkMaxGrid = 16777215u;   // 2^24 - 1 workgroups of 256 threads: a grid is 32 bits of threads
// dynamic LDS, in bytes from its base: [expand alone: the rows' sub-phone values,] the waves' two sums, the rows' phones or source
// frames, the running frame counts, the running kept counts (every offset a multiple of 16)
constexpr int kSkFeatBytes = kSkBlockRows * kSkMaxF * 8;
constexpr int kSkOffRow = 2 * kSkWaves * 8;
constexpr int kSkOffCum = kSkOffRow + kSkBlockRows * 4;
constexpr size_t kSkDefaultLds = 65536;   // what a kernel gets unasked

std::atomic<long long> g_sil_launches{0};

struct SkArgs {
  const void *dur;
  int dtype_dur;
  const int32_t *num_phones;
  const uint8_t *sil;
  int Nmax, S, min_frames;
  // expand
  const void *phone;
  long ld_p;
  int Dl, F, kind;
  const double *cc, *scale, *mins;
  // gather
  const void *src;
  long ld_src;
  const int32_t *len_src;
  int Tmax, D;
  // both
  void *out;
  long ld_out;
  int Tcap, nblk;
  int32_t *lengths_out;
};

// a duration in frames (include/nnmnkwii_frontend.h; restated from csrc/frame_expand.hip)
__device__ inline int sk_frames(const void *d, int dtype, size_t idx, int min_frames) {
  if (dtype == NNMK_FRONTEND_I32 || dtype == NNMK_FRONTEND_I64) {
    long long v = dtype == NNMK_FRONTEND_I32 ? (long long)((const int32_t *)d)[idx] : (long long)((const int64_t *)d)[idx];
    if (v < min_frames) v = min_frames;
    return v > (long long)kSkIntMax ? kSkIntMax : (int)v;
  }
  const double x = dtype == NNMK_FRONTEND_F32 ? (double)((const float *)d)[idx] : ((const double *)d)[idx];
  const double r = rint(x);   // half to even
  if (!(r > (double)min_frames)) return min_frames;   // NaN too
  return r > (double)kSkIntMax ? kSkIntMax : (int)r;
}

__device__ inline int sk_num_phones(const int32_t *num_phones, int b, int Nmax) {
  if (!num_phones) return Nmax;
  const int n = num_phones[b];
  return n < 0 ? 0 : (n > Nmax ? Nmax : n);
}

// the F sub-phone values of frame i of state s (from 1) of fn frames, `base` frames into a phone of pd frames (restated from
// csrc/frame_expand.hip)
__device__ inline void sk_subphone(int kind, const double *__restrict__ cc, int S, int s, long long i, long long fn, long long base,
                                   long long pd, double *__restrict__ f) {
  const long long j = base + i;
  const double dfn = (double)fn, dpd = (double)pd;
  switch (kind) {
    case NNMK_FRONTEND_FULL:
      f[0] = (double)(i + 1) / dfn;
      f[1] = (double)(fn - i) / dfn;
      f[2] = dfn;
      f[3] = (double)s;
      f[4] = (double)(S + 1 - s);
      f[5] = dpd;
      f[6] = dfn / dpd;
      f[7] = (double)(pd - i - base) / dpd;
      f[8] = (double)(base + i + 1) / dpd;
      break;
    case NNMK_FRONTEND_MINIMAL_FRAME:
      f[0] = (double)(i + 1) / dfn;
      f[1] = (double)s;
      break;
    case NNMK_FRONTEND_STATE_ONLY:
      f[0] = (double)s;
      break;
    case NNMK_FRONTEND_FRAME_ONLY:
      f[0] = (double)(j + 1) / dpd;
      break;
    case NNMK_FRONTEND_UNIFORM_STATE: {
      const double x = (double)(j + 1) / dpd;
      const double y = rint(x * 5.0);
      f[0] = x;
      f[1] = y > 1.0 ? y : 1.0;
      break;
    }
    case NNMK_FRONTEND_COARSE_CODING: {
      int q = (int)((200.0 / dpd) * (double)j);   // j < pd: at most 200
      q = q < 0 ? 0 : (q > 299 ? 299 : q);        // (never taken: keeps the reads inside the table whatever the arithmetic gives)
      f[0] = (double)(float)cc[300 + q];
      f[1] = (double)(float)cc[NNMK_FRONTEND_CC_POINTS + 200 + q];
      f[2] = (double)(float)cc[2 * NNMK_FRONTEND_CC_POINTS + 100 + q];
      f[3] = dpd;
      break;
    }
    case NNMK_FRONTEND_MINIMAL_PHONEME:
      f[0] = (double)(j + 1) / dpd;
      f[1] = (double)(pd - j) / dpd;
      f[2] = dpd;
      break;
    default:
      break;
  }
}

__device__ inline int sk_saturate(long long v) { return v > (long long)kSkIntMax ? kSkIntMax : (int)v; }

// The scan of one utterance's ns states by the 256 threads of a workgroup: cuma[k] = frames of states 0 .. k, cumk[k] = those
// among them whose phone is not flagged, both saturated; the totals (int64) to every thread.  Reached by every thread; the caller
// puts a barrier between it and the first read of the counts.
__device__ inline void sk_scan(const SkArgs &a, int b, int ns, long long *wsum, int *cuma, int *cumk, long long &total_all,
                               long long &total_kept) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int S = a.S;
  const size_t d0 = (size_t)b * a.Nmax * S;
  const uint8_t *__restrict__ sil = a.sil + (size_t)b * a.Nmax;
  const int per = (ns + 255) / 256;
  const int k0 = tid * per < ns ? tid * per : ns, k1 = k0 + per < ns ? k0 + per : ns;
  long long mine_a = 0, mine_k = 0;
  for (int k = k0; k < k1; ++k) {
    const long long r = sk_frames(a.dur, a.dtype_dur, d0 + k, a.min_frames);
    mine_a += r;
    if (!sil[k / S]) mine_k += r;
  }
  long long inc_a = mine_a, inc_k = mine_k;
  for (int off = 1; off < 64; off <<= 1) {
    const long long ua = __shfl_up(inc_a, off), uk = __shfl_up(inc_k, off);
    if (lane >= off) {
      inc_a += ua;
      inc_k += uk;
    }
  }
  if (lane == 63) {
    wsum[2 * wave] = inc_a;
    wsum[2 * wave + 1] = inc_k;
  }
  __syncthreads();
  long long run_a = inc_a - mine_a, run_k = inc_k - mine_k;
  total_all = 0;
  total_kept = 0;
  for (int w = 0; w < kSkWaves; ++w) {
    if (w < wave) {
      run_a += wsum[2 * w];
      run_k += wsum[2 * w + 1];
    }
    total_all += wsum[2 * w];
    total_kept += wsum[2 * w + 1];
  }
  for (int k = k0; k < k1; ++k) {
    const long long r = sk_frames(a.dur, a.dtype_dur, d0 + k, a.min_frames);
    run_a += r;
    if (!sil[k / S]) run_k += r;
    cuma[k] = sk_saturate(run_a);
    cumk[k] = sk_saturate(run_k);
  }
}

// the first state whose running count exceeds v (the caller knows that the last one does)
__device__ inline int sk_first_above(const int *cum, int ns, int v) {
  int lo = 0, hi = ns - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] > v)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

template <typename TP, typename TO>
__global__ __launch_bounds__(256) void keep_expand_kernel(SkArgs a) {
  double *feat = sk_lds;
  long long *wsum = (long long *)((char *)sk_lds + kSkFeatBytes);
  int *rowphone = (int *)((char *)sk_lds + kSkFeatBytes + kSkOffRow);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned g = blockIdx.x;
  const int b = (int)(g / (unsigned)a.nblk), blk = (int)(g - (unsigned)b * (unsigned)a.nblk);
  const int S = a.S;
  const int ns = sk_num_phones(a.num_phones, b, a.Nmax) * S;   // <= NNMK_FRONTEND_MAX_STATES
  int *cuma = (int *)((char *)sk_lds + kSkFeatBytes + kSkOffCum), *cumk = cuma + (size_t)a.Nmax * S;
  const size_t d0 = (size_t)b * a.Nmax * S;

  long long total_all, total_kept;
  sk_scan(a, b, ns, wsum, cuma, cumk, total_all, total_kept);
  const int live = total_kept < (long long)a.Tcap ? (int)total_kept : a.Tcap;
  if (blk == 0 && tid == 0) a.lengths_out[b] = live;
  const int t0 = blk * kSkBlockRows;
  if (t0 >= a.Tcap) return;   // (Tcap == 0: the one workgroup of the utterance has written its length)
  const int nrows = a.Tcap - t0 < kSkBlockRows ? a.Tcap - t0 : kSkBlockRows;
  __syncthreads();

  // ---- describe: the phone and the sub-phone values of each of the block's rows
  if (tid < nrows) {
    const int r = t0 + tid;
    int ph = -1;
    if (r < live) {   // live <= K_b: the last kept count exceeds r
      const int lo = sk_first_above(cumk, ns, r);
      ph = lo / S;
      const int si = lo - ph * S;
      const long long i = r - (lo ? cumk[lo - 1] : 0);   // (an entry that is <= r is not saturated)
      long long pd = 0, base = 0, fn = 0;
      for (int q = 0; q < S; ++q) {
        const long long f = sk_frames(a.dur, a.dtype_dur, d0 + (size_t)ph * S + q, a.min_frames);
        pd += f;
        if (q < si) base += f;
        if (q == si) fn = f;
      }
      sk_subphone(a.kind, a.cc, S, si + 1, i, fn, base, pd, feat + tid * kSkMaxF);
    }
    rowphone[tid] = ph;
  }
  __syncthreads();

  // ---- store
  const int r0 = wave * kSkRowsPerWave, r1 = r0 + kSkRowsPerWave < nrows ? r0 + kSkRowsPerWave : nrows;
  const int Dl = a.Dl, W = a.Dl + a.F;
  const bool affine = a.scale != nullptr;
  const TP *__restrict__ P = (const TP *)a.phone + (size_t)b * a.Nmax * a.ld_p;
  TO *__restrict__ out = (TO *)a.out + ((size_t)b * a.Tcap + t0) * a.ld_out;
  for (int c = lane; c < W; c += 64) {
    double sc = 1.0, mn = 0.0;
    if (affine) {
      sc = a.scale[c];
      mn = a.mins[c];
    }
    int prev = -1;
    TO pv = (TO)0;
    for (int r = r0; r < r1; ++r) {
      const int ph = rowphone[r];
      TO *o = out + (size_t)r * a.ld_out + c;
      if (ph < 0) {
        *o = (TO)0;
        continue;
      }
      if (c < Dl) {
        if (ph != prev) {
          double v = (double)P[(size_t)ph * a.ld_p + c];
          if (affine) v = v * sc + mn;
          pv = (TO)v;
          prev = ph;
        }
        *o = pv;
      } else {
        double v = feat[r * kSkMaxF + (c - Dl)];
        if (affine) v = v * sc + mn;
        *o = (TO)v;
      }
    }
  }
}

template <typename TS, typename TO>
__global__ __launch_bounds__(256) void keep_gather_kernel(SkArgs a) {
  long long *wsum = (long long *)sk_lds;
  int *rowsrc = (int *)((char *)sk_lds + kSkOffRow);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned g = blockIdx.x;
  const int b = (int)(g / (unsigned)a.nblk), blk = (int)(g - (unsigned)b * (unsigned)a.nblk);
  const int S = a.S;
  const int ns = sk_num_phones(a.num_phones, b, a.Nmax) * S;
  int *cuma = (int *)((char *)sk_lds + kSkOffCum), *cumk = cuma + (size_t)a.Nmax * S;
  int len = a.len_src ? a.len_src[b] : a.Tmax;
  len = len < 0 ? 0 : (len > a.Tmax ? a.Tmax : len);

  long long total_all, total_kept;
  sk_scan(a, b, ns, wsum, cuma, cumk, total_all, total_kept);
  __syncthreads();
  if (blk == 0 && tid == 0) {
    // the frames in front of `len` that are kept
    long long n;
    if ((long long)len >= total_all) {
      n = total_kept + ((long long)len - total_all);
    } else {   // frame `len` exists: it lies in the first state whose frame count exceeds it
      const int lo = sk_first_above(cuma, ns, len);
      const int before = lo ? cuma[lo - 1] : 0;   // (<= len: not saturated, and neither is the kept count below)
      n = (lo ? cumk[lo - 1] : 0) + (a.sil[(size_t)b * a.Nmax + lo / S] ? 0 : len - before);
    }
    a.lengths_out[b] = n < (long long)a.Tcap ? (int)n : a.Tcap;
  }
  const int t0 = blk * kSkBlockRows;
  if (t0 >= a.Tcap) return;
  const int nrows = a.Tcap - t0 < kSkBlockRows ? a.Tcap - t0 : kSkBlockRows;

  // ---- describe: the source frame of each of the block's rows, -1 for a pad row
  if (tid < nrows) {
    const int r = t0 + tid;
    long long t;
    if ((long long)r < total_kept) {
      const int lo = sk_first_above(cumk, ns, r);
      t = (long long)(lo ? cuma[lo - 1] : 0) + (r - (lo ? cumk[lo - 1] : 0));   // (a saturated frame count is not below len)
    } else {
      t = total_all + ((long long)r - total_kept);
    }
    rowsrc[tid] = t < (long long)len ? (int)t : -1;
  }
  __syncthreads();

  // ---- store
  const int r0 = wave * kSkRowsPerWave, r1 = r0 + kSkRowsPerWave < nrows ? r0 + kSkRowsPerWave : nrows;
  const TS *__restrict__ src = (const TS *)a.src + (size_t)b * a.Tmax * a.ld_src;
  TO *__restrict__ out = (TO *)a.out + ((size_t)b * a.Tcap + t0) * a.ld_out;
  for (int r = r0; r < r1; ++r) {
    const int t = rowsrc[r];
    for (int c = lane; c < a.D; c += 64) out[(size_t)r * a.ld_out + c] = t < 0 ? (TO)0 : (TO)src[(size_t)t * a.ld_src + c];
  }
}

__global__ __launch_bounds__(256) void keep_counts_kernel(const void *dur, int dtype_dur, const int32_t *num_phones, const uint8_t *sil,
                                                          int Nmax, int S, int min_frames, int64_t *counts) {
  __shared__ long long wsum[2 * kSkWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const int ns = sk_num_phones(num_phones, b, Nmax) * S;
  const size_t d0 = (size_t)b * Nmax * S;
  long long s = 0, k = 0;
  for (int q = tid; q < ns; q += 256) {
    const long long r = sk_frames(dur, dtype_dur, d0 + q, min_frames);
    s += r;
    if (!sil[(size_t)b * Nmax + q / S]) k += r;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    s += __shfl_xor(s, m);
    k += __shfl_xor(k, m);
  }
  if (lane == 0) {
    wsum[2 * wave] = s;
    wsum[2 * wave + 1] = k;
  }
  __syncthreads();
  if (tid == 0) {
    counts[2 * (size_t)b] = (int64_t)(wsum[1] + wsum[3] + wsum[5] + wsum[7]);
    counts[2 * (size_t)b + 1] = (int64_t)(wsum[0] + wsum[2] + wsum[4] + wsum[6]);
  }
}

int sk_refuse(const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  set_error(fmt, a, b, c, d);
  return MLPG_HIP_EINVAL;
}

int sk_feature_size(int kind) {
  static const int sizes[8] = {0, 9, 2, 1, 1, 2, 4, 3};
  return kind >= 0 && kind < 8 ? sizes[kind] : -1;
}

// what all entries ask of the durations' side
int sk_check_durations(int dtype_dur, int B, int Nmax, int S, int min_frames) {
  if (dtype_dur < NNMK_FRONTEND_F32 || dtype_dur > NNMK_FRONTEND_I64)
    return sk_refuse("silence: dtype_dur must be 0 (float32), 1 (float64), 2 (int32) or 3 (int64), got %lld", dtype_dur);
  if (B < 0 || Nmax < 0 || min_frames < 0)
    return sk_refuse("silence: negative size (B = %lld, Nmax = %lld, min_frames = %lld)", B, Nmax, min_frames);
  if (S < 1 || S > NNMK_FRONTEND_MAX_S) return sk_refuse("silence: S must be in 1 .. %lld, got %lld", NNMK_FRONTEND_MAX_S, S);
  if ((int64_t)Nmax * S > NNMK_FRONTEND_MAX_STATES)
    return sk_refuse("silence: Nmax * S = %lld states, at most %lld fit (NNMK_FRONTEND_MAX_STATES)", (int64_t)Nmax * S, NNMK_FRONTEND_MAX_STATES);
  return 0;
}

bool sk_float_dtype(int dtype) { return dtype == NNMK_FRONTEND_F32 || dtype == NNMK_FRONTEND_F64; }

// a workgroup's LDS above what a kernel gets unasked has to be asked for (8192 states: 64 KB of running counts)
template <typename K>
int sk_launch(K kern, hipStream_t st, unsigned blocks, size_t lds_bytes, const SkArgs &a) {
  if (lds_bytes > kSkDefaultLds)
    MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kSkFeatBytes + kSkOffCum + 8 * NNMK_FRONTEND_MAX_STATES));
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds_bytes, st, a);
  MLPG_HIP_CHECK(hipGetLastError());
  g_sil_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

int launch_keep_expand(hipStream_t st, int dtype_phone, int dtype_out, int B, const SkArgs &a) {
  const size_t lds_bytes = (size_t)kSkFeatBytes + kSkOffCum + (size_t)a.Nmax * a.S * 8;   // at most 70464
  const unsigned blocks = (unsigned)((int64_t)B * a.nblk);
  if (dtype_phone == NNMK_FRONTEND_F64)
    return dtype_out == NNMK_FRONTEND_F64 ? sk_launch(keep_expand_kernel<double, double>, st, blocks, lds_bytes, a)
                                          : sk_launch(keep_expand_kernel<double, float>, st, blocks, lds_bytes, a);
  return dtype_out == NNMK_FRONTEND_F64 ? sk_launch(keep_expand_kernel<float, double>, st, blocks, lds_bytes, a)
                                        : sk_launch(keep_expand_kernel<float, float>, st, blocks, lds_bytes, a);
}

int launch_keep_gather(hipStream_t st, int dtype_src, int dtype_out, int B, const SkArgs &a) {
  const size_t lds_bytes = (size_t)kSkOffCum + (size_t)a.Nmax * a.S * 8;   // at most 65856
  const unsigned blocks = (unsigned)((int64_t)B * a.nblk);
  if (dtype_src == NNMK_FRONTEND_F64)
    return dtype_out == NNMK_FRONTEND_F64 ? sk_launch(keep_gather_kernel<double, double>, st, blocks, lds_bytes, a)
                                          : sk_launch(keep_gather_kernel<double, float>, st, blocks, lds_bytes, a);
  return dtype_out == NNMK_FRONTEND_F64 ? sk_launch(keep_gather_kernel<float, double>, st, blocks, lds_bytes, a)
                                        : sk_launch(keep_gather_kernel<float, float>, st, blocks, lds_bytes, a);
}

int launch_keep_counts(hipStream_t st, int dtype_dur, const void *dur, const int32_t *num_phones, const uint8_t *sil, int B, int Nmax,
                       int S, int min_frames, int64_t *counts) {
  hipLaunchKernelGGL(keep_counts_kernel, dim3((unsigned)B), dim3(256), 0, st, dur, dtype_dur, num_phones, sil, Nmax, S, min_frames, counts);
  MLPG_HIP_CHECK(hipGetLastError());
  g_sil_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int nnmk_sil_abi_version(void) { return NNMK_SIL_ABI_VERSION; }

__attribute__((visibility("default"))) long long nnmk_sil_launch_count(void) { return g_sil_launches.load(std::memory_order_relaxed); }

__attribute__((visibility("default"))) int nnmk_sil_frame_counts(int device, void *stream, int dtype_dur, const void *durations,
                                                                 const int32_t *num_phones, const uint8_t *silence, int B, int Nmax,
                                                                 int S, int min_frames, int64_t *counts) {
  const char *who = "silence";
  if (int rc = sk_check_durations(dtype_dur, B, Nmax, S, min_frames)) return rc;
  if ((unsigned)B > kSkMaxGrid) return sk_refuse("silence: the batch is too large for one grid (B = %lld)", B);
  if (int rc = check_device(who, device)) return rc;
  if (B > 0 && !counts) return sk_refuse("silence: NULL counts");
  if ((int64_t)B * Nmax > 0 && !durations) return sk_refuse("silence: NULL durations");
  if ((int64_t)B * Nmax > 0 && !silence) return sk_refuse("silence: NULL silence flags");
  if (B == 0) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_keep_counts((hipStream_t)stream, dtype_dur, durations, num_phones, silence, B, Nmax, S, min_frames, counts);
}

__attribute__((visibility("default"))) int nnmk_sil_expand(int device, void *stream, int dtype_phone, const void *phone, int64_t ld_phone,
                                                           int dtype_dur, const void *durations, const int32_t *num_phones,
                                                           const uint8_t *silence, int B, int Nmax, int S, int Dl, int min_frames,
                                                           int kind, const double *cc, const double *scale_, const double *min_,
                                                           int dtype_out, void *out, int64_t ld_out, int Tcap, int32_t *lengths_out) {
  const char *who = "silence";
  if (!sk_float_dtype(dtype_phone) || !sk_float_dtype(dtype_out))
    return sk_refuse("silence: dtype must be 0 (float32) or 1 (float64), got dtype_phone = %lld, dtype_out = %lld", dtype_phone, dtype_out);
  if (int rc = sk_check_durations(dtype_dur, B, Nmax, S, min_frames)) return rc;
  if (Dl < 0 || Tcap < 0) return sk_refuse("silence: negative size (Dl = %lld, Tcap = %lld)", Dl, Tcap);
  const int F = sk_feature_size(kind);
  if (F < 0) return sk_refuse("silence: unknown kind %lld", kind);
  const int64_t W = (int64_t)Dl + F;
  if (W > (int64_t)kSkIntMax) return sk_refuse("silence: Dl + F = %lld columns do not fit", W);
  if (ld_phone < Dl || ld_out < W)
    return sk_refuse("silence: the row strides must reach the last column (ld_phone = %lld < Dl = %lld or ld_out = %lld < Dl + F = %lld)", ld_phone, Dl,
                     ld_out, W);
  const int64_t nblk = Tcap > 0 ? ((int64_t)Tcap + kSkBlockRows - 1) / kSkBlockRows : 1;
  if ((int64_t)B * nblk > (int64_t)kSkMaxGrid)
    return sk_refuse("silence: the batch is too large for one grid (B = %lld, Tcap = %lld)", B, Tcap);
  if ((scale_ == nullptr) != (min_ == nullptr)) return sk_refuse("silence: scale_ and min_ go together (one of them is NULL)");
  if (kind == NNMK_FRONTEND_COARSE_CODING && !cc) return sk_refuse("silence: the coarse-coding kind needs its table (cc is NULL)");
  if (int rc = check_device(who, device)) return rc;
  if (B > 0 && !lengths_out) return sk_refuse("silence: NULL lengths_out");
  if ((int64_t)B * Nmax > 0 && !durations) return sk_refuse("silence: NULL durations");
  if ((int64_t)B * Nmax > 0 && !silence) return sk_refuse("silence: NULL silence flags");
  if ((int64_t)B * Nmax > 0 && Dl > 0 && !phone) return sk_refuse("silence: NULL phone matrix");
  if ((int64_t)B * Tcap > 0 && W > 0 && !out) return sk_refuse("silence: NULL out");
  if (B == 0) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  SkArgs a = {};
  a.dur = durations;
  a.dtype_dur = dtype_dur;
  a.num_phones = num_phones;
  a.sil = silence;
  a.Nmax = Nmax;
  a.S = S;
  a.min_frames = min_frames;
  a.phone = phone;
  a.ld_p = (long)ld_phone;
  a.Dl = Dl;
  a.F = F;
  a.kind = kind;
  a.cc = cc;
  a.scale = scale_;
  a.mins = min_;
  a.out = out;
  a.ld_out = (long)ld_out;
  a.Tcap = Tcap;
  a.nblk = (int)nblk;
  a.lengths_out = lengths_out;
  return launch_keep_expand((hipStream_t)stream, dtype_phone, dtype_out, B, a);
}

__attribute__((visibility("default"))) int nnmk_sil_gather(int device, void *stream, int dtype_dur, const void *durations,
                                                           const int32_t *num_phones, const uint8_t *silence, int B, int Nmax, int S,
                                                           int min_frames, int dtype_src, const void *src, int64_t ld_src,
                                                           const int32_t *len_src, int Tmax, int D, int dtype_out, void *out,
                                                           int64_t ld_out, int Tcap, int32_t *lengths_out) {
  const char *who = "silence";
  if (!sk_float_dtype(dtype_src) || !sk_float_dtype(dtype_out))
    return sk_refuse("silence: dtype must be 0 (float32) or 1 (float64), got dtype_src = %lld, dtype_out = %lld", dtype_src, dtype_out);
  if (int rc = sk_check_durations(dtype_dur, B, Nmax, S, min_frames)) return rc;
  if (Tmax < 0 || D < 0 || Tcap < 0) return sk_refuse("silence: negative size (Tmax = %lld, D = %lld, Tcap = %lld)", Tmax, D, Tcap);
  if (Tmax == kSkIntMax) return sk_refuse("silence: Tmax must be below 2^31 - 1 (a frame index has to stay below a saturated count)");
  if (ld_src < D || ld_out < D)
    return sk_refuse("silence: the row strides must reach the last column (ld_src = %lld or ld_out = %lld < D = %lld)", ld_src, ld_out, D);
  const int64_t nblk = Tcap > 0 ? ((int64_t)Tcap + kSkBlockRows - 1) / kSkBlockRows : 1;
  if ((int64_t)B * nblk > (int64_t)kSkMaxGrid)
    return sk_refuse("silence: the batch is too large for one grid (B = %lld, Tcap = %lld)", B, Tcap);
  if (int rc = check_device(who, device)) return rc;
  if (B > 0 && !lengths_out) return sk_refuse("silence: NULL lengths_out");
  if ((int64_t)B * Nmax > 0 && !durations) return sk_refuse("silence: NULL durations");
  if ((int64_t)B * Nmax > 0 && !silence) return sk_refuse("silence: NULL silence flags");
  if ((int64_t)B * Tmax > 0 && D > 0 && !src) return sk_refuse("silence: NULL src");
  if ((int64_t)B * Tcap > 0 && D > 0 && !out) return sk_refuse("silence: NULL out");
  if (out && out == src) return sk_refuse("silence: out == src (rows move across workgroups: the gather cannot run in place)");
  if (B == 0) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  SkArgs a = {};
  a.dur = durations;
  a.dtype_dur = dtype_dur;
  a.num_phones = num_phones;
  a.sil = silence;
  a.Nmax = Nmax;
  a.S = S;
  a.min_frames = min_frames;
  a.src = src;
  a.ld_src = (long)ld_src;
  a.len_src = len_src;
  a.Tmax = Tmax;
  a.D = D;
  a.out = out;
  a.ld_out = (long)ld_out;
  a.Tcap = Tcap;
  a.nblk = (int)nblk;
  a.lengths_out = lengths_out;
  return launch_keep_gather((hipStream_t)stream, dtype_src, dtype_out, B, a);
}

}  // extern "C"
