// K14: phone-level linguistic features expanded to frames over a padded batch (nnmk_frontend_expand and
// nnmk_frontend_frame_counts, include/nnmnkwii_frontend.h; the duration-dependent part of the reference's
// frontend/merlin.py:284-485, load_labels_with_state_alignment / _phone_alignment with add_frame_features=True).
// tools/frontend_model.py is the executable specification of everything below.
//
// expand_kernel: a workgroup of four waves takes NNMK_FRONTEND_BLOCK_ROWS frames of ONE utterance, counted from its frame 0.
//   scan      every thread turns a run of consecutive states' durations into frames and adds them up (int64); the 256 sums
//             meet in a wave scan (shuffles) and a four-entry table in LDS; the thread then writes the running count BEHIND each
//             of its states to LDS as int32, saturated at 2^31 - 1 (a frame index is below Tmax <= 2^31 - 1, so a saturated
//             entry still compares right).  Redone by every workgroup of the utterance: a few hundred states against 64 rows
//             of output.
//   describe  thread r < 64 finds the state of frame t0 + r by binary search (the first state whose running count exceeds the
//             frame index: states of 0 frames are never found), reads its phone's S durations again for fn, base and pd, and
//             writes the frame's phone index and its F sub-phone values (float64) to LDS.  Frames at or past the utterance's
//             length get phone -1.
//   store     wave w takes rows 16 w .. 16 w + 15 of the block, its lanes consecutive columns c = lane, lane + 64, ...: a lane
//             loads scale_[c] and min_[c] once, then walks down its rows; it loads the phone row's element only when the phone
//             changes (a wave-uniform test) and keeps the finished value, reads the sub-phone values from LDS, and stores one
//             element per row -- 256 contiguous bytes per wave instruction (float32).  Pad rows get zeros.
// Workgroup 0 of an utterance writes lengths_out.  No workgroup reads a duration or a phone row at or past num_phones[b], and
// none stores outside its own rows' first Dl + F columns.  Every offset is 64-bit.
// counts_kernel: one workgroup per utterance adds its states' frames (int64).
// Compiled with -ffp-contract=off: the affine map is a multiplication and an addition, each rounded, as numpy.
#include <math.h>

#include <atomic>

#include "common.h"
#include "../../include/nnmnkwii_frontend.h"

namespace mlpg {

namespace {

constexpr int kFxBlockRows = NNMK_FRONTEND_BLOCK_ROWS;
constexpr int kFxWaves = 4;
constexpr int kFxRowsPerWave = kFxBlockRows / kFxWaves;
constexpr int kFxMaxF = 9;
constexpr int kFxIntMax = 2147483647;
constexpr unsigned kFxMaxGrid = 16777215u;   // 2^24 - 1 workgroups of 256 threads: a grid is 32 bits of threads
// dynamic LDS, in bytes from its base: the rows' sub-phone values, the waves' sums, the rows' phones, the running counts
constexpr int kFxOffSums = kFxBlockRows * kFxMaxF * 8;
constexpr int kFxOffPhone = kFxOffSums + kFxWaves * 8;
constexpr int kFxOffCum = kFxOffPhone + kFxBlockRows * 4;

std::atomic<long long> g_frontend_launches{0};

struct FxArgs {
  const void *phone;
  long ld_p;
  const void *dur;
  int dtype_dur;
  const int32_t *num_phones;
  int Nmax, S, Dl, F, min_frames, kind;
  const double *cc, *scale, *mins;
  void *out;
  long ld_out;
  int Tmax, nblk;
  int32_t *lengths_out;
};

// a duration in frames (include/nnmnkwii_frontend.h)
__device__ inline int fx_frames(const void *d, int dtype, size_t idx, int min_frames) {
  if (dtype == NNMK_FRONTEND_I32 || dtype == NNMK_FRONTEND_I64) {
    long long v = dtype == NNMK_FRONTEND_I32 ? (long long)((const int32_t *)d)[idx] : (long long)((const int64_t *)d)[idx];
    if (v < min_frames) v = min_frames;
    return v > (long long)kFxIntMax ? kFxIntMax : (int)v;
  }
  const double x = dtype == NNMK_FRONTEND_F32 ? (double)((const float *)d)[idx] : ((const double *)d)[idx];
  const double r = rint(x);   // half to even
  if (!(r > (double)min_frames)) return min_frames;   // NaN too
  return r > (double)kFxIntMax ? kFxIntMax : (int)r;
}

__device__ inline int fx_num_phones(const int32_t *num_phones, int b, int Nmax) {
  if (!num_phones) return Nmax;
  const int n = num_phones[b];
  return n < 0 ? 0 : (n > Nmax ? Nmax : n);
}

// the F sub-phone values of frame i of state s (from 1) of fn frames, `base` frames into a phone of pd frames
__device__ inline void fx_subphone(int kind, const double *__restrict__ cc, int S, int s, long long i, long long fn, long long base,
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

template <typename TP, typename TO>
__global__ __launch_bounds__(256) void expand_kernel(FxArgs a) {
  extern __shared__ double fx_lds[];
  double *feat = fx_lds;
  long long *wsum = (long long *)((char *)fx_lds + kFxOffSums);
  int *rowphone = (int *)((char *)fx_lds + kFxOffPhone);
  int *cum = (int *)((char *)fx_lds + kFxOffCum);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned g = blockIdx.x;
  const int b = (int)(g / (unsigned)a.nblk), blk = (int)(g - (unsigned)b * (unsigned)a.nblk);
  const int S = a.S;
  const int ns = fx_num_phones(a.num_phones, b, a.Nmax) * S;   // <= NNMK_FRONTEND_MAX_STATES
  const size_t d0 = (size_t)b * a.Nmax * S;

  // ---- scan: cum[k] = frames of states 0 .. k, saturated
  const int per = (ns + 255) / 256;
  const int k0 = tid * per < ns ? tid * per : ns, k1 = k0 + per < ns ? k0 + per : ns;
  long long mine = 0;
  for (int k = k0; k < k1; ++k) mine += fx_frames(a.dur, a.dtype_dur, d0 + k, a.min_frames);
  long long inc = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const long long u = __shfl_up(inc, off);
    if (lane >= off) inc += u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  long long run = inc - mine, total = 0;
  for (int w = 0; w < kFxWaves; ++w) {
    if (w < wave) run += wsum[w];
    total += wsum[w];
  }
  for (int k = k0; k < k1; ++k) {
    run += fx_frames(a.dur, a.dtype_dur, d0 + k, a.min_frames);
    cum[k] = run > (long long)kFxIntMax ? kFxIntMax : (int)run;
  }
  const int live = total < (long long)a.Tmax ? (int)total : a.Tmax;
  if (blk == 0 && tid == 0) a.lengths_out[b] = live;
  const int t0 = blk * kFxBlockRows;
  if (t0 >= a.Tmax) return;   // (Tmax == 0: the one workgroup of the utterance has written its length)
  const int nrows = a.Tmax - t0 < kFxBlockRows ? a.Tmax - t0 : kFxBlockRows;
  __syncthreads();

  // ---- describe: the phone and the sub-phone values of each of the block's rows
  if (tid < nrows) {
    const int t = t0 + tid;
    int ph = -1;
    if (t < live) {   // live <= total: the last running count exceeds t
      int lo = 0, hi = ns - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > t)
          hi = mid;
        else
          lo = mid + 1;
      }
      ph = lo / S;
      const int si = lo - ph * S;
      const long long i = t - (lo ? cum[lo - 1] : 0);   // (an entry that is <= t is not saturated)
      long long pd = 0, base = 0, fn = 0;
      for (int q = 0; q < S; ++q) {
        const long long r = fx_frames(a.dur, a.dtype_dur, d0 + (size_t)ph * S + q, a.min_frames);
        pd += r;
        if (q < si) base += r;
        if (q == si) fn = r;
      }
      fx_subphone(a.kind, a.cc, S, si + 1, i, fn, base, pd, feat + tid * kFxMaxF);
    }
    rowphone[tid] = ph;
  }
  __syncthreads();

  // ---- store
  const int r0 = wave * kFxRowsPerWave, r1 = r0 + kFxRowsPerWave < nrows ? r0 + kFxRowsPerWave : nrows;
  const int Dl = a.Dl, W = a.Dl + a.F;
  const bool affine = a.scale != nullptr;
  const TP *__restrict__ P = (const TP *)a.phone + (size_t)b * a.Nmax * a.ld_p;
  TO *__restrict__ out = (TO *)a.out + ((size_t)b * a.Tmax + t0) * a.ld_out;
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
        double v = feat[r * kFxMaxF + (c - Dl)];
        if (affine) v = v * sc + mn;
        *o = (TO)v;
      }
    }
  }
}

__global__ __launch_bounds__(256) void counts_kernel(const void *dur, int dtype_dur, const int32_t *num_phones, int Nmax, int S,
                                                     int min_frames, int64_t *counts) {
  __shared__ long long wsum[kFxWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const int ns = fx_num_phones(num_phones, b, Nmax) * S;
  const size_t d0 = (size_t)b * Nmax * S;
  long long s = 0;
  for (int k = tid; k < ns; k += 256) s += fx_frames(dur, dtype_dur, d0 + k, min_frames);
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0) wsum[wave] = s;
  __syncthreads();
  if (tid == 0) counts[b] = (int64_t)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

int fx_refuse(const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  set_error(fmt, a, b, c, d);
  return MLPG_HIP_EINVAL;
}

int fx_feature_size(int kind) {
  static const int sizes[8] = {0, 9, 2, 1, 1, 2, 4, 3};
  return kind >= 0 && kind < 8 ? sizes[kind] : -1;
}

// what both entries ask of the durations' side
int fx_check_durations(int dtype_dur, int B, int Nmax, int S, int min_frames) {
  if (dtype_dur < NNMK_FRONTEND_F32 || dtype_dur > NNMK_FRONTEND_I64)
    return fx_refuse("frontend: dtype_dur must be 0 (float32), 1 (float64), 2 (int32) or 3 (int64), got %lld", dtype_dur);
  if (B < 0 || Nmax < 0 || min_frames < 0)
    return fx_refuse("frontend: negative size (B = %lld, Nmax = %lld, min_frames = %lld)", B, Nmax, min_frames);
  if (S < 1 || S > NNMK_FRONTEND_MAX_S) return fx_refuse("frontend: S must be in 1 .. %lld, got %lld", NNMK_FRONTEND_MAX_S, S);
  if ((int64_t)Nmax * S > NNMK_FRONTEND_MAX_STATES)
    return fx_refuse("frontend: Nmax * S = %lld states, at most %lld fit (NNMK_FRONTEND_MAX_STATES)", (int64_t)Nmax * S, NNMK_FRONTEND_MAX_STATES);
  return 0;
}

template <typename TP>
void fx_launch_out(hipStream_t st, int dtype_out, unsigned blocks, size_t lds_bytes, const FxArgs &a) {
  if (dtype_out == NNMK_FRONTEND_F64)
    hipLaunchKernelGGL((expand_kernel<TP, double>), dim3(blocks), dim3(256), lds_bytes, st, a);
  else
    hipLaunchKernelGGL((expand_kernel<TP, float>), dim3(blocks), dim3(256), lds_bytes, st, a);
}

int launch_expand(hipStream_t st, int dtype_phone, int dtype_out, int B, const FxArgs &a) {
  const size_t lds_bytes = (size_t)kFxOffCum + (size_t)a.Nmax * a.S * 4;   // at most 37664
  const unsigned blocks = (unsigned)((int64_t)B * a.nblk);
  if (dtype_phone == NNMK_FRONTEND_F64)
    fx_launch_out<double>(st, dtype_out, blocks, lds_bytes, a);
  else
    fx_launch_out<float>(st, dtype_out, blocks, lds_bytes, a);
  MLPG_HIP_CHECK(hipGetLastError());
  g_frontend_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

int launch_counts(hipStream_t st, int dtype_dur, const void *dur, const int32_t *num_phones, int B, int Nmax, int S, int min_frames,
                  int64_t *counts) {
  hipLaunchKernelGGL(counts_kernel, dim3((unsigned)B), dim3(256), 0, st, dur, dtype_dur, num_phones, Nmax, S, min_frames, counts);
  MLPG_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int nnmk_frontend_abi_version(void) { return NNMK_FRONTEND_ABI_VERSION; }

__attribute__((visibility("default"))) int nnmk_frontend_feature_size(int kind) { return fx_feature_size(kind); }

__attribute__((visibility("default"))) long long nnmk_frontend_launch_count(void) {
  return g_frontend_launches.load(std::memory_order_relaxed);
}

__attribute__((visibility("default"))) int nnmk_frontend_frame_counts(int device, void *stream, int dtype_dur, const void *durations,
                                                                      const int32_t *num_phones, int B, int Nmax, int S,
                                                                      int min_frames, int64_t *counts) {
  const char *who = "frontend";
  if (int rc = fx_check_durations(dtype_dur, B, Nmax, S, min_frames)) return rc;
  if ((unsigned)B > kFxMaxGrid) return fx_refuse("frontend: the batch is too large for one grid (B = %lld)", B);
  if (int rc = check_device(who, device)) return rc;
  if (B > 0 && !counts) return fx_refuse("frontend: NULL counts");
  if ((int64_t)B * Nmax > 0 && !durations) return fx_refuse("frontend: NULL durations");
  if (B == 0) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_counts((hipStream_t)stream, dtype_dur, durations, num_phones, B, Nmax, S, min_frames, counts);
}

__attribute__((visibility("default"))) int nnmk_frontend_expand(int device, void *stream, int dtype_phone, const void *phone,
                                                                int64_t ld_phone, int dtype_dur, const void *durations,
                                                                const int32_t *num_phones, int B, int Nmax, int S, int Dl,
                                                                int min_frames, int kind, const double *cc, const double *scale_,
                                                                const double *min_, int dtype_out, void *out, int64_t ld_out,
                                                                int Tmax, int32_t *lengths_out) {
  const char *who = "frontend";
  if ((dtype_phone != NNMK_FRONTEND_F32 && dtype_phone != NNMK_FRONTEND_F64) || (dtype_out != NNMK_FRONTEND_F32 && dtype_out != NNMK_FRONTEND_F64))
    return fx_refuse("frontend: dtype must be 0 (float32) or 1 (float64), got dtype_phone = %lld, dtype_out = %lld", dtype_phone, dtype_out);
  if (int rc = fx_check_durations(dtype_dur, B, Nmax, S, min_frames)) return rc;
  if (Dl < 0 || Tmax < 0) return fx_refuse("frontend: negative size (Dl = %lld, Tmax = %lld)", Dl, Tmax);
  const int F = fx_feature_size(kind);
  if (F < 0) return fx_refuse("frontend: unknown kind %lld", kind);
  const int64_t W = (int64_t)Dl + F;
  if (W > (int64_t)kFxIntMax) return fx_refuse("frontend: Dl + F = %lld columns do not fit", W);
  if (ld_phone < Dl || ld_out < W)
    return fx_refuse("frontend: the row strides must reach the last column (ld_phone = %lld < Dl = %lld or ld_out = %lld < Dl + F = %lld)", ld_phone, Dl,
                     ld_out, W);
  const int64_t nblk = Tmax > 0 ? ((int64_t)Tmax + kFxBlockRows - 1) / kFxBlockRows : 1;
  if ((int64_t)B * nblk > (int64_t)kFxMaxGrid)
    return fx_refuse("frontend: the batch is too large for one grid (B = %lld, Tmax = %lld)", B, Tmax);
  if ((scale_ == nullptr) != (min_ == nullptr)) return fx_refuse("frontend: scale_ and min_ go together (one of them is NULL)");
  if (kind == NNMK_FRONTEND_COARSE_CODING && !cc) return fx_refuse("frontend: the coarse-coding kind needs its table (cc is NULL)");
  if (int rc = check_device(who, device)) return rc;
  if (B > 0 && !lengths_out) return fx_refuse("frontend: NULL lengths_out");
  if ((int64_t)B * Nmax > 0 && !durations) return fx_refuse("frontend: NULL durations");
  if ((int64_t)B * Nmax > 0 && Dl > 0 && !phone) return fx_refuse("frontend: NULL phone matrix");
  if ((int64_t)B * Tmax > 0 && W > 0 && !out) return fx_refuse("frontend: NULL out");
  if (B == 0) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  FxArgs a;
  a.phone = phone;
  a.ld_p = (long)ld_phone;
  a.dur = durations;
  a.dtype_dur = dtype_dur;
  a.num_phones = num_phones;
  a.Nmax = Nmax;
  a.S = S;
  a.Dl = Dl;
  a.F = F;
  a.min_frames = min_frames;
  a.kind = kind;
  a.cc = cc;
  a.scale = scale_;
  a.mins = min_;
  a.out = out;
  a.ld_out = (long)ld_out;
  a.Tmax = Tmax;
  a.nblk = (int)nblk;
  a.lengths_out = lengths_out;
  return launch_expand((hipStream_t)stream, dtype_phone, dtype_out, B, a);
}

}  // extern "C"
