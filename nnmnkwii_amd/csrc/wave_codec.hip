// K16: the waveform side of preprocessing over a padded batch (nnmk_wave_encode / nnmk_wave_decode, include/nnmnkwii_wave.h; the
// reference's preprocessing/generic.py:56-226: mulaw, inv_mulaw, mulaw_quantize, inv_mulaw_quantize, preemphasis,
// inv_preemphasis).  tools/wave_model.py is the executable specification of everything below; `tiled` there is the decode walk,
// operation for operation.
//
// wave_encode_kernel: elementwise over (B, Lmax).  A thread takes 4 consecutive samples (one 16-byte access per 16 bytes where the
// pointer and the utterance stride allow, single elements otherwise), and for pre-emphasis one more load, its left neighbour.
// Pre-emphasis is computed in the input's dtype (two rounded operations, no contraction), the mu-law in float64 on that value,
// the class by truncation.  Both logarithms come from the device's log1p, so +-1 land on 0 and mu exactly.
//
// wave_decode_kernel: a workgroup of four waves takes ONE segment of ONE utterance and walks it in tiles of NNMK_WAVE_TILE.
//   front     thread i reads samples t0 + 4 i .. t0 + 4 i + 3 and turns them into float64 values: a table entry (the table sits in
//             LDS, or stays in memory when it is longer than NNMK_WAVE_TABLE_LDS), the float inv_mulaw, or the value itself.
//   local     with de-emphasis the thread runs z[m] = v[m] + c z[m-1] over its 4 values from a zero state; thread 0 starts from
//             the tile's carry.
//   scan      the threads' last values go through a Kogge-Stone scan, E[i] += c^(4 2^s) E[i - 2^s]: s = 0 .. 5 by __shfl_up
//             inside a wave; the four wave totals meet in four LDS words (two sets, taken in turn: one barrier per tile) and
//             every thread runs steps s = 6, 7 on them in registers.  A thread of wave w > 0 adds c^(4 (lane + 1)) times what
//             came in from the waves before -- that power is the product of the scan multipliers at the set bits of lane + 1,
//             formed once per thread -- and every thread but thread 0 adds c^(m + 1) times its left neighbour's final value to
//             sample m.  The last thread's final value is the next tile's carry; every thread forms it from the four words.
//   store     rounded once to y's dtype.
// The twelve powers (c^(4 2^s), s = 0 .. 7, and c^1 .. c^4) are computed on the host in float64 and passed in: the model uses
// the same numbers.  A segment j > 0 starts W samples early from a zero state and stores nothing there (nnmk_wave_plan: |c|^W <=
// 2^-80).  Without de-emphasis every tile is a segment of its own.  Samples at or past L are not read and get zeros (the class of
// silence for encode's class outputs).  Every offset is 64-bit.  Control flow is uniform across the workgroup wherever a shuffle
// or a barrier is reached.  Compiled with -ffp-contract=off: every multiplication and addition above is rounded.
#include <atomic>
#include <cmath>

#include "common.h"
#include "../../include/nnmnkwii_wave.h"

namespace mlpg {

namespace {

constexpr int kWaveTile = NNMK_WAVE_TILE;
constexpr int kWaveThreads = kWaveTile / 4;
constexpr int kWaveTabLds = NNMK_WAVE_TABLE_LDS;
// nnmk_wave_plan's own segment length (segment == 0): measured on an MI355X, profiles/wave.json and DESIGN.md K16
constexpr long kWaveAutoSegment = 16384;

std::atomic<long long> g_wave_launches{0};

// 4 consecutive samples as one access: 16-byte aligned for 4-byte elements and up, the 4 elements' own size below
template <typename T>
struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) WavePack {
  T v[4];
};

struct WaveEncArgs {
  const void *x;
  void *y;
  long ld_x, ld_y;
  const int32_t *lengths;
  long item0;   // the (utterance, tile) pair of workgroup 0: a batch over the grid's limit goes in slices
  long tiles;   // tiles per utterance
  int Lmax, mu, vec_x, vec_y;
  double coef;
};

struct WaveDecArgs {
  const void *x;
  void *y;
  const float *table;
  long ld_x, ld_y;
  const int32_t *lengths;
  long item0;   // the (utterance, segment) pair of workgroup 0
  long S, W, nseg;
  int Lmax, mu, vec_x, vec_y;
  double coef;
  double pw[12];   // c^(4 2^s), s = 0 .. 7; c^1 .. c^4
};

__device__ inline double wave_sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : (d == 0.0 ? 0.0 : d)); }

// sign(d) log1p(mu |d|) / log1p(mu), the reference's order; lm = log1p(mu) from the same routine
__device__ inline double wave_mulaw(double d, double mu, double lm) { return wave_sign(d) * log1p(mu * fabs(d)) / lm; }

// sign(d) (1 / mu) ((1 + mu)^|d| - 1), the reference's order
__device__ inline double wave_inv_mulaw(double d, double mu) { return wave_sign(d) * (1.0 / mu) * (pow(1.0 + mu, fabs(d)) - 1.0); }

// v truncated toward zero; NaN gives 0, and what no int64 holds gives +-2^62
__device__ inline long long wave_class(double v) {
  if (!(v == v)) return 0;
  const double lim = 4611686018427387904.0;
  return (long long)(v > lim ? lim : (v < -lim ? -lim : v));
}

template <typename TX, typename TY, int PRE, int STAGE>
__global__ __launch_bounds__(256) void wave_encode_kernel(WaveEncArgs a) {
  const long item = a.item0 + (long)blockIdx.x;
  const int b = (int)(item / a.tiles);
  const long n0 = (item - (long)b * a.tiles) * kWaveTile + 4 * (long)threadIdx.x;
  if (n0 >= a.Lmax) return;
  int L = a.Lmax;
  if (a.lengths) {
    const int n = a.lengths[b];
    L = n < 0 ? 0 : (n > a.Lmax ? a.Lmax : n);
  }
  const TX *x = (const TX *)a.x + (size_t)b * a.ld_x;   // (y may be x: no __restrict__)
  TY *y = (TY *)a.y + (size_t)b * a.ld_y;
  const int live = L - n0 >= 4 ? 4 : (L - n0 <= 0 ? 0 : (int)(L - n0));
  const int cnt = a.Lmax - n0 >= 4 ? 4 : (int)(a.Lmax - n0);
  TX v[4] = {(TX)0, (TX)0, (TX)0, (TX)0};
  if (live == 4 && a.vec_x) {
    const WavePack<TX> p = *(const WavePack<TX> *)(x + n0);
    for (int m = 0; m < 4; ++m) v[m] = p.v[m];
  } else {
    for (int m = 0; m < live; ++m) v[m] = x[n0 + m];
  }
  TX left = (TX)0;
  if (PRE && live > 0 && n0 > 0) left = x[n0 - 1];
  const TX nc = (TX)(-(TX)a.coef);
  const double mu = (double)a.mu;
  const double lm = STAGE != NNMK_WAVE_PLAIN ? log1p(mu) : 0.0;
  WavePack<TY> o;
  for (int m = 0; m < 4; ++m) {
    TX p = v[m];
    if (PRE) {   // (sample 0 meets the filter's initial state, +0.0: a -0.0 there comes out as +0.0, as from lfilter)
      const TX t = n0 + m > 0 ? nc * (m ? v[m - 1] : left) : (TX)0;
      p = v[m] + t;
    }
    if (m >= live) {
      o.v[m] = STAGE == NNMK_WAVE_QUANTIZE ? (TY)(a.mu / 2) : (TY)0;
    } else if (STAGE == NNMK_WAVE_PLAIN) {
      o.v[m] = (TY)p;
    } else {
      const double r = wave_mulaw((double)p, mu, lm);
      if (STAGE == NNMK_WAVE_MULAW)
        o.v[m] = (TY)r;
      else
        o.v[m] = (TY)wave_class((r + 1.0) / 2.0 * mu);
    }
  }
  if (cnt == 4 && a.vec_y) {
    *(WavePack<TY> *)(y + n0) = o;
  } else {
    for (int m = 0; m < cnt; ++m) y[n0 + m] = o.v[m];
  }
}

template <typename TX, typename TY, int FRONT, int EMPH>
__global__ __launch_bounds__(256) void wave_decode_kernel(WaveDecArgs a) {
  __shared__ float s_tab[kWaveTabLds];
  __shared__ double s_wt[2][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long item = a.item0 + (long)blockIdx.x;
  const int b = (int)(item / a.nseg);
  const long seg = item - (long)b * a.nseg;
  int L = a.Lmax;
  if (a.lengths) {
    const int n = a.lengths[b];
    L = n < 0 ? 0 : (n > a.Lmax ? a.Lmax : n);
  }
  const TX *x = (const TX *)a.x + (size_t)b * a.ld_x;   // (y may be x without de-emphasis: no __restrict__)
  TY *y = (TY *)a.y + (size_t)b * a.ld_y;
  const long lo = seg * a.S;
  const long hi = lo + a.S < a.Lmax ? lo + a.S : (long)a.Lmax;
  const long live_hi = hi < L ? hi : (long)L;
  const float *tab = a.table;
  if (FRONT == NNMK_WAVE_QUANTIZE && a.mu < kWaveTabLds) {   // (the same in every workgroup of the launch)
    for (int i = tid; i <= a.mu; i += kWaveThreads) s_tab[i] = a.table[i];
    __syncthreads();
    tab = s_tab;
  }
  const double c = a.coef, mu = (double)a.mu;
  double lanepow = 1.0;   // c^(4 (lane + 1))
  if (EMPH)
    for (int s = 0; s < 7; ++s)
      if (((lane + 1) >> s) & 1) lanepow = lanepow * a.pw[s];
  double carry = 0.0;
  int par = 0;
  const long start = EMPH && seg > 0 && lo < L ? lo - a.W : lo;
  for (long t0 = start; t0 < live_hi; t0 += kWaveTile) {
    const long n0 = t0 + 4 * (long)tid;
    const int live = live_hi - n0 >= 4 ? 4 : (live_hi - n0 <= 0 ? 0 : (int)(live_hi - n0));
    // ---- front
    TX raw[4] = {(TX)0, (TX)0, (TX)0, (TX)0};
    if (live == 4 && a.vec_x) {
      const WavePack<TX> p = *(const WavePack<TX> *)(x + n0);
      for (int m = 0; m < 4; ++m) raw[m] = p.v[m];
    } else {
      for (int m = 0; m < live; ++m) raw[m] = x[n0 + m];
    }
    double v[4];
    for (int m = 0; m < 4; ++m) {
      if (m >= live) {
        v[m] = 0.0;
      } else if (FRONT == NNMK_WAVE_QUANTIZE) {
        const long long k = (long long)raw[m];
        v[m] = (double)tab[k < 0 ? 0 : (k > a.mu ? a.mu : (int)k)];
      } else if (FRONT == NNMK_WAVE_MULAW) {
        v[m] = wave_inv_mulaw((double)raw[m], mu);
      } else {
        v[m] = (double)raw[m];
      }
    }
    if (EMPH) {
      // ---- local
      if (tid == 0) v[0] = v[0] + c * carry;
      for (int m = 1; m < 4; ++m) v[m] = v[m] + c * v[m - 1];
      // ---- scan
      double e = v[3];
      for (int s = 0; s < 6; ++s) {
        const double u = __shfl_up(e, 1 << s);
        if (lane >= (1 << s)) e = e + a.pw[s] * u;
      }
      if (lane == 63) s_wt[par][wave] = e;
      __syncthreads();
      const double t0w = s_wt[par][0], t1w = s_wt[par][1], t2w = s_wt[par][2], t3w = s_wt[par][3];
      par ^= 1;
      const double p0 = t0w;
      const double p1 = t1w + a.pw[6] * t0w;
      double p2 = t2w + a.pw[6] * t1w;
      p2 = p2 + a.pw[7] * p0;
      const double in_w = wave == 0 ? 0.0 : (wave == 1 ? p0 : (wave == 2 ? p1 : p2));
      const double f = wave == 0 ? e : e + lanepow * in_w;
      double in = __shfl_up(f, 1);
      if (lane == 0) in = in_w;
      if (tid != 0)
        for (int m = 0; m < 4; ++m) v[m] = v[m] + a.pw[8 + m] * in;
      carry = t3w + a.pw[6] * p2;   // (thread 255's f: its lanepow is c^256)
    }
    // ---- store
    if (t0 >= lo) {
      if (live == 4 && a.vec_y) {
        WavePack<TY> o;
        for (int m = 0; m < 4; ++m) o.v[m] = (TY)v[m];
        *(WavePack<TY> *)(y + n0) = o;
      } else {
        for (int m = 0; m < live; ++m) y[n0 + m] = (TY)v[m];
      }
    }
  }
  for (long t = (lo > L ? lo : (long)L) + tid; t < hi; t += kWaveThreads) y[t] = (TY)0;
}

int wave_refuse(const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  set_error(fmt, a, b, c);
  return MLPG_HIP_EINVAL;
}

bool wave_float(int dt) { return dt == NNMK_WAVE_F32 || dt == NNMK_WAVE_F64; }
bool wave_int(int dt) { return dt >= NNMK_WAVE_U8 && dt <= NNMK_WAVE_I64; }
size_t wave_size(int dt) {
  return dt == NNMK_WAVE_F32 || dt == NNMK_WAVE_I32 ? 4 : (dt == NNMK_WAVE_U8 ? 1 : (dt == NNMK_WAVE_I16 ? 2 : 8));
}
// whether 4 consecutive samples at a multiple of 4 from an utterance's start may go as one WavePack access
int wave_vec_ok(const void *p, long ld, int dt) {
  const size_t sz = wave_size(dt), al = 4 * sz > 16 ? 16 : 4 * sz;
  return (uintptr_t)p % al == 0 && ((size_t)ld * sz) % al == 0;
}

// ---- encode: dtype_x x dtype_y x pre-emphasis x stage
template <typename TX, typename TY, int STAGE>
void wave_enc_go(hipStream_t st, int pre, unsigned blocks, const WaveEncArgs &a) {
  if (pre)
    hipLaunchKernelGGL((wave_encode_kernel<TX, TY, 1, STAGE>), dim3(blocks), dim3(kWaveThreads), 0, st, a);
  else
    hipLaunchKernelGGL((wave_encode_kernel<TX, TY, 0, STAGE>), dim3(blocks), dim3(kWaveThreads), 0, st, a);
}

template <typename TX>
void wave_enc_y(hipStream_t st, int pre, int stage, int dtype_y, unsigned blocks, const WaveEncArgs &a) {
  if (stage == NNMK_WAVE_QUANTIZE) {
    switch (dtype_y) {
      case NNMK_WAVE_U8: return wave_enc_go<TX, uint8_t, NNMK_WAVE_QUANTIZE>(st, pre, blocks, a);
      case NNMK_WAVE_I16: return wave_enc_go<TX, int16_t, NNMK_WAVE_QUANTIZE>(st, pre, blocks, a);
      case NNMK_WAVE_I32: return wave_enc_go<TX, int32_t, NNMK_WAVE_QUANTIZE>(st, pre, blocks, a);
      default: return wave_enc_go<TX, int64_t, NNMK_WAVE_QUANTIZE>(st, pre, blocks, a);
    }
  }
  if (stage == NNMK_WAVE_MULAW) {
    if (dtype_y == NNMK_WAVE_F64) return wave_enc_go<TX, double, NNMK_WAVE_MULAW>(st, pre, blocks, a);
    return wave_enc_go<TX, float, NNMK_WAVE_MULAW>(st, pre, blocks, a);
  }
  if (dtype_y == NNMK_WAVE_F64) return wave_enc_go<TX, double, NNMK_WAVE_PLAIN>(st, pre, blocks, a);
  return wave_enc_go<TX, float, NNMK_WAVE_PLAIN>(st, pre, blocks, a);
}

int launch_wave_encode(hipStream_t st, int dtype_x, int dtype_y, int pre, int stage, long items, WaveEncArgs a) {
  const long step = items_per_launch(1, kWaveThreads);
  for (long i0 = 0; i0 < items; i0 += step) {
    const unsigned cnt = (unsigned)(items - i0 < step ? items - i0 : step);
    a.item0 = i0;
    if (dtype_x == NNMK_WAVE_F64)
      wave_enc_y<double>(st, pre, stage, dtype_y, cnt, a);
    else
      wave_enc_y<float>(st, pre, stage, dtype_y, cnt, a);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  g_wave_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

// ---- decode: dtype_x x dtype_y x front end x de-emphasis
template <typename TX, typename TY, int FRONT>
void wave_dec_go(hipStream_t st, int emph, unsigned blocks, const WaveDecArgs &a) {
  if (emph)
    hipLaunchKernelGGL((wave_decode_kernel<TX, TY, FRONT, 1>), dim3(blocks), dim3(kWaveThreads), 0, st, a);
  else
    hipLaunchKernelGGL((wave_decode_kernel<TX, TY, FRONT, 0>), dim3(blocks), dim3(kWaveThreads), 0, st, a);
}

template <typename TY>
void wave_dec_x(hipStream_t st, int emph, int stage, int dtype_x, unsigned blocks, const WaveDecArgs &a) {
  if (stage == NNMK_WAVE_QUANTIZE) {
    switch (dtype_x) {
      case NNMK_WAVE_U8: return wave_dec_go<uint8_t, TY, NNMK_WAVE_QUANTIZE>(st, emph, blocks, a);
      case NNMK_WAVE_I16: return wave_dec_go<int16_t, TY, NNMK_WAVE_QUANTIZE>(st, emph, blocks, a);
      case NNMK_WAVE_I32: return wave_dec_go<int32_t, TY, NNMK_WAVE_QUANTIZE>(st, emph, blocks, a);
      default: return wave_dec_go<int64_t, TY, NNMK_WAVE_QUANTIZE>(st, emph, blocks, a);
    }
  }
  if (stage == NNMK_WAVE_MULAW) {
    if (dtype_x == NNMK_WAVE_F64) return wave_dec_go<double, TY, NNMK_WAVE_MULAW>(st, emph, blocks, a);
    return wave_dec_go<float, TY, NNMK_WAVE_MULAW>(st, emph, blocks, a);
  }
  if (dtype_x == NNMK_WAVE_F64) return wave_dec_go<double, TY, NNMK_WAVE_PLAIN>(st, emph, blocks, a);
  return wave_dec_go<float, TY, NNMK_WAVE_PLAIN>(st, emph, blocks, a);
}

int launch_wave_decode(hipStream_t st, int dtype_x, int dtype_y, int emph, int stage, long items, WaveDecArgs a) {
  const long step = items_per_launch(1, kWaveThreads);
  for (long i0 = 0; i0 < items; i0 += step) {
    const unsigned cnt = (unsigned)(items - i0 < step ? items - i0 : step);
    a.item0 = i0;
    if (dtype_y == NNMK_WAVE_F64)
      wave_dec_x<double>(st, emph, stage, dtype_x, cnt, a);
    else
      wave_dec_x<float>(st, emph, stage, dtype_x, cnt, a);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  g_wave_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

// the plan of include/nnmnkwii_wave.h; 0, or -1 with the error text set
int wave_plan(long Lmax, double coef, long segment, long *S, long *W, long *nseg) {
  // |c|^TILE by ten squarings, then the smallest k >= 1 with (|c|^TILE)^k <= 2^-80 by repeated multiplication: no
  // transcendental, so any IEEE host (and the model) finds the same W
  const double limit = 8.271806125530277e-25;   // 2^-80
  double p = fabs(coef);
  for (int i = 0; i < 10; ++i) p = p * p;
  long w = -1;
  if (p < 1.0) {   // (false for NaN)
    double q = p;
    long k = 1;
    while (q > limit && k < (1L << 20)) {
      q = q * p;
      ++k;
    }
    if (q <= limit) w = k * kWaveTile;
  }
  long s = Lmax, n = 1;
  if (segment < 0) return wave_refuse("wave: negative segment %lld", segment);
  if (segment == 0) {
    if (Lmax > kWaveAutoSegment && w > 0 && w <= kWaveAutoSegment / 4) s = kWaveAutoSegment;
  } else if (segment < Lmax) {
    if (segment % kWaveTile != 0)
      return wave_refuse("wave: segment %lld is no multiple of the tile of %lld samples", segment, kWaveTile);
    if (w < 0 || w > segment)
      return wave_refuse("wave: segment %lld is too short for this coef: the warm-up of %lld samples (-1: no decay) must fit into it", segment,
                         w);
    s = segment;
  }
  if (s < Lmax) n = (Lmax + s - 1) / s;
  if (S) *S = s;
  if (W) *W = w;
  if (nseg) *nseg = n;
  return 0;
}

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int nnmk_wave_abi_version(void) { return NNMK_WAVE_ABI_VERSION; }

__attribute__((visibility("default"))) long long nnmk_wave_launch_count(void) { return g_wave_launches.load(std::memory_order_relaxed); }

__attribute__((visibility("default"))) int nnmk_wave_plan(int64_t Lmax, double coef, int64_t segment, int64_t *S, int64_t *W,
                                                          int64_t *nseg) {
  if (Lmax < 0) return wave_refuse("wave: negative size (Lmax = %lld)", Lmax);
  long s = 0, w = 0, n = 0;
  if (int rc = wave_plan((long)Lmax, coef, (long)segment, &s, &w, &n)) return rc;
  if (S) *S = s;
  if (W) *W = w;
  if (nseg) *nseg = n;
  return 0;
}

__attribute__((visibility("default"))) int nnmk_wave_encode(int device, void *stream, int dtype_x, const void *x, int64_t ld_x,
                                                            const int32_t *lengths, int B, int Lmax, int emphasis, double coef, int stage,
                                                            int mu, int dtype_y, void *y, int64_t ld_y) {
  const char *who = "wave";
  if (wave_int(dtype_x)) return wave_refuse("wave: encode takes float32 or float64 waveforms, not integers (dtype_x = %lld)", dtype_x);
  if (!wave_float(dtype_x)) return wave_refuse("wave: unknown dtype_x %lld", dtype_x);
  if (stage < NNMK_WAVE_PLAIN || stage > NNMK_WAVE_QUANTIZE) return wave_refuse("wave: unknown stage %lld", stage);
  if (stage == NNMK_WAVE_QUANTIZE ? !wave_int(dtype_y) : !wave_float(dtype_y))
    return wave_refuse("wave: dtype_y = %lld does not go with stage %lld (classes are 2 .. 5, floats 0 and 1)", dtype_y, stage);
  if (stage != NNMK_WAVE_PLAIN && mu < 1) return wave_refuse("wave: mu must be at least 1, got %lld", mu);
  if (stage == NNMK_WAVE_QUANTIZE && dtype_y == NNMK_WAVE_U8 && mu > 255) return wave_refuse("wave: mu = %lld does not fit uint8 classes", mu);
  if (stage == NNMK_WAVE_QUANTIZE && dtype_y == NNMK_WAVE_I16 && mu > 32767) return wave_refuse("wave: mu = %lld does not fit int16 classes", mu);
  if (B < 0 || Lmax < 0) return wave_refuse("wave: negative size (B = %lld, Lmax = %lld)", B, Lmax);
  if (ld_x < Lmax || ld_y < Lmax)
    return wave_refuse("wave: the utterance strides must reach the last sample (ld_x = %lld, ld_y = %lld below Lmax)", ld_x, ld_y);
  if (emphasis && !(coef == coef)) return wave_refuse("wave: coef is NaN");
  if (int rc = check_device(who, device)) return rc;
  const bool empty = B == 0 || Lmax == 0;
  if (!empty && (!x || !y)) return wave_refuse("wave: NULL x or y");
  if (!empty && x == y && emphasis) return wave_refuse("wave: with pre-emphasis y must not be x");
  if (!empty && x == y && wave_size(dtype_x) != wave_size(dtype_y))
    return wave_refuse("wave: y may be x only when the element sizes match (dtype_x = %lld, dtype_y = %lld)", dtype_x, dtype_y);
  if (empty) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  WaveEncArgs a;
  a.x = x;
  a.y = y;
  a.ld_x = (long)ld_x;
  a.ld_y = (long)ld_y;
  a.lengths = lengths;
  a.item0 = 0;
  a.tiles = ((long)Lmax + kWaveTile - 1) / kWaveTile;
  a.Lmax = Lmax;
  a.mu = mu;
  a.vec_x = wave_vec_ok(x, a.ld_x, dtype_x);
  a.vec_y = wave_vec_ok(y, a.ld_y, dtype_y);
  a.coef = coef;
  return launch_wave_encode((hipStream_t)stream, dtype_x, dtype_y, emphasis != 0, stage, (long)B * a.tiles, a);
}

__attribute__((visibility("default"))) int nnmk_wave_decode(int device, void *stream, int dtype_x, const void *x, int64_t ld_x,
                                                            const int32_t *lengths, int B, int Lmax, int stage, int mu, const float *table,
                                                            int emphasis, double coef, int64_t segment, int dtype_y, void *y,
                                                            int64_t ld_y) {
  const char *who = "wave";
  if (stage < NNMK_WAVE_PLAIN || stage > NNMK_WAVE_QUANTIZE) return wave_refuse("wave: unknown stage %lld", stage);
  if (stage == NNMK_WAVE_QUANTIZE ? !wave_int(dtype_x) : !wave_float(dtype_x))
    return wave_refuse("wave: dtype_x = %lld does not go with stage %lld (classes are 2 .. 5, floats 0 and 1)", dtype_x, stage);
  if (!wave_float(dtype_y)) return wave_refuse("wave: decode gives float32 or float64 waveforms (dtype_y = %lld)", dtype_y);
  if (stage != NNMK_WAVE_PLAIN && mu < 1) return wave_refuse("wave: mu must be at least 1, got %lld", mu);
  if (B < 0 || Lmax < 0) return wave_refuse("wave: negative size (B = %lld, Lmax = %lld)", B, Lmax);
  if (ld_x < Lmax || ld_y < Lmax)
    return wave_refuse("wave: the utterance strides must reach the last sample (ld_x = %lld, ld_y = %lld below Lmax)", ld_x, ld_y);
  if (emphasis && !(coef == coef)) return wave_refuse("wave: coef is NaN");
  long S = kWaveTile, W = 0, nseg = ((long)Lmax + kWaveTile - 1) / kWaveTile;   // without de-emphasis every tile is a segment
  if (emphasis)
    if (int rc = wave_plan(Lmax, coef, (long)segment, &S, &W, &nseg)) return rc;
  if (int rc = check_device(who, device)) return rc;
  const bool empty = B == 0 || Lmax == 0;
  if (!empty && (!x || !y)) return wave_refuse("wave: NULL x or y");
  if (!empty && stage == NNMK_WAVE_QUANTIZE && !table) return wave_refuse("wave: NULL table");
  if (!empty && x == y && emphasis) return wave_refuse("wave: with de-emphasis y must not be x");
  if (!empty && x == y && wave_size(dtype_x) != wave_size(dtype_y))
    return wave_refuse("wave: y may be x only when the element sizes match (dtype_x = %lld, dtype_y = %lld)", dtype_x, dtype_y);
  if (empty) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  WaveDecArgs a;
  a.x = x;
  a.y = y;
  a.table = table;
  a.ld_x = (long)ld_x;
  a.ld_y = (long)ld_y;
  a.lengths = lengths;
  a.item0 = 0;
  a.S = S;
  a.W = W;
  a.nseg = nseg;
  a.Lmax = Lmax;
  a.mu = mu;
  a.vec_x = wave_vec_ok(x, a.ld_x, dtype_x);
  a.vec_y = wave_vec_ok(y, a.ld_y, dtype_y);
  a.coef = coef;
  // c^(4 2^s) by repeated squaring from c^4 = (c c) (c c), and c^1 .. c^4 by repeated multiplication: the model's numbers
  const double c2 = coef * coef;
  a.pw[0] = c2 * c2;
  for (int s = 1; s < 8; ++s) a.pw[s] = a.pw[s - 1] * a.pw[s - 1];
  a.pw[8] = coef;
  a.pw[9] = c2;
  a.pw[10] = c2 * coef;
  a.pw[11] = a.pw[0];
  return launch_wave_decode((hipStream_t)stream, dtype_x, dtype_y, emphasis != 0, stage, (long)B * nseg, a);
}

}  // extern "C"
