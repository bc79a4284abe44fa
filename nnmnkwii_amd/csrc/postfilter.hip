// K8: the Merlin post-filter for mel-cepstra (mlpg_hip_merlin_post_filter; the reference's postfilters/__init__.py:7-62 with
// SPTK's freqt, c2acr, mc2b and b2mc restated from their published definitions, tools/postfilter_model.py).  Per frame c, with
// v = weight * c:   r0 = c2acr0(freqt(c)), p0 = c2acr0(freqt(v)), b = mc2b(v), b[0] += log(r0 / p0) / 2, out = b2mc(b).
// freqt and Re DFT are linear: L = G c on the half spectrum with the host-built table G (fftlen/2 + 1, D) of postfilter_table.h,
// and r0 = (1/N) sum_k wk exp(2 L_k), wk = 1 at bins 0 and N/2 and 2 between.  Over many frames that is a GEMM with an
// exp-and-reduce epilogue, on v_mfma_f64_16x16x4_f64 (lane maps: top of gmm_em.hip): frames are the rows, bins the columns,
// K = D padded to a multiple of 4 with zeros.
//
// One workgroup (4 waves) per MLPG_HIP_POSTFILTER_FRAME_TILE = 64 frames.  The frames sit in LDS as float64 (never-loaded zeros
// for padding frames and for columns past D).  Wave w takes the bin tiles w, w + 4, ... for ALL 64 frames (four 16-row blocks,
// two accumulator tiles each: c and v), so the workgroup streams every element of G exactly once per 64 frames; the A operands
// come from LDS, v's as c * weight on the way.  Epilogue per tile: exp(2 L) times the bin weight (0 for the masked bins past
// N/2 of the last tile), added per lane in tile order; behind the last tile four xor-shuffles add the 16 lanes of a row, the
// waves' sums go through LDS and are added in wave order.  No atomics: the same bits on every call.  Thread f < 64 then runs the
// two recursions of frame f in LDS, and all threads store the rows (typed; exact zeros for padding frames; columns of out past D
// are never touched).  A frame is in LDS whole before anything is stored: out may be mgc itself.
// The exponentials are not rescaled: an input whose exp(2 L) overflows gives what the formula gives.
// Compiled with -ffp-contract=off.
#include <math.h>

#include "common.h"
#include "postfilter_table.h"

namespace mlpg {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kPfFrames = MLPG_HIP_POSTFILTER_FRAME_TILE;
constexpr int kPfLd = kPfMaxD + 1;   // odd row stride: the 16 rows of an A operand fall on different banks
static_assert(kPfFrames == 64, "four 16-row MFMA blocks per wave, one recursion thread per frame of the first wave");

__device__ inline v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

template <typename T>
__global__ __launch_bounds__(256) void postfilter_kernel(const T *mgc, long ld_in, const int32_t *__restrict__ lengths, long frames,
                                                         int Tmax, int D, double alpha, const double *__restrict__ weight,
                                                         const double *__restrict__ G, int fftlen, T *out, long ld_out) {
  __shared__ double xs[kPfFrames * kPfLd];
  __shared__ double wt[kPfMaxD];
  __shared__ double red[2][4][kPfFrames];
  __shared__ int vld[kPfFrames];
  const int tid = threadIdx.x;
  const long n0 = (long)blockIdx.x * kPfFrames;

  int mine = 0;
  if (tid < kPfFrames) {
    const long n = n0 + tid;
    if (n < frames) {
      const long b = n / Tmax;
      const int t = (int)(n - b * Tmax);
      int len = Tmax;
      if (lengths) {
        len = lengths[b];
        len = len < 0 ? 0 : (len > Tmax ? Tmax : len);
      }
      mine = t < len;
    }
    vld[tid] = mine;
    wt[tid] = tid < D ? weight[tid] : 0.0;
  }
  const int any = __syncthreads_or(mine);
  if (!any) {   // a tile of padding only: nothing is read
    for (int i = tid; i < kPfFrames * D; i += 256) {
      const int r = i / D, c = i - r * D;
      if (n0 + r < frames) out[(size_t)(n0 + r) * ld_out + c] = (T)0;
    }
    return;
  }
  for (int i = tid; i < kPfFrames * kPfLd; i += 256) {
    const int r = i / kPfLd, c = i - r * kPfLd;
    xs[i] = (c < D && vld[r]) ? (double)mgc[(size_t)(n0 + r) * ld_in + c] : 0.0;
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  const int r4 = lane >> 4, c16 = lane & 15;
  const int K4 = (D + 3) & ~3;
  const int nb = fftlen / 2 + 1, tiles = (nb + 15) >> 4;
  double sr[4][4], sp[4][4];   // [16-row block][accumulator register]: frame 16 rb + r4 + 4 g
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int g = 0; g < 4; ++g) sr[rb][g] = sp[rb][g] = 0.0;

  for (int j = wave; j < tiles; j += 4) {
    const int bin = 16 * j + c16;
    const bool bin_ok = bin < nb;
    const double *grow = G + (size_t)(bin_ok ? bin : 0) * D;
    v4d ac[4], av[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) ac[rb] = av[rb] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K4; k0 += 4) {
      const int kk = k0 + r4;
      const double b = (bin_ok && kk < D) ? grow[kk] : 0.0;
      const double wk = wt[kk];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const double a = xs[(rb * 16 + c16) * kPfLd + kk];
        ac[rb] = mfma_f64(a, b, ac[rb]);
        av[rb] = mfma_f64(a * wk, b, av[rb]);
      }
    }
    const double bw = (bin == 0 || bin == nb - 1) ? 1.0 : 2.0;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        sr[rb][g] += bin_ok ? bw * exp(2.0 * ac[rb][g]) : 0.0;
        sp[rb][g] += bin_ok ? bw * exp(2.0 * av[rb][g]) : 0.0;
      }
  }
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      double s = sr[rb][g], p = sp[rb][g];
      s += __shfl_xor(s, 1);
      p += __shfl_xor(p, 1);
      s += __shfl_xor(s, 2);
      p += __shfl_xor(p, 2);
      s += __shfl_xor(s, 4);
      p += __shfl_xor(p, 4);
      s += __shfl_xor(s, 8);
      p += __shfl_xor(p, 8);
      if (c16 == 0) {
        red[0][wave][rb * 16 + r4 + 4 * g] = s;
        red[1][wave][rb * 16 + r4 + 4 * g] = p;
      }
    }
  __syncthreads();   // every wave is done with xs as an operand; the waves' sums are in red

  if (tid < kPfFrames && vld[tid]) {
    const double inv_n = 1.0 / (double)fftlen;
    const double r0 = (((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid]) * inv_n;
    const double p0 = (((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid]) * inv_n;
    double *row = xs + tid * kPfLd;
    const int m = D - 1;
    // mc2b on v = weight * c, in place
    double nxt = wt[m] * row[m];
    row[m] = nxt;
    for (int i = m - 1; i >= 0; --i) {
      nxt = wt[i] * row[i] - alpha * nxt;
      row[i] = nxt;
    }
    row[0] = log(r0 / p0) / 2.0 + row[0];
    // b2mc, in place
    double delta = row[m];
    for (int i = m - 1; i >= 0; --i) {
      const double bi = row[i];
      row[i] = bi + alpha * delta;
      delta = bi;
    }
  }
  __syncthreads();
  for (int i = tid; i < kPfFrames * D; i += 256) {
    const int r = i / D, c = i - r * D;
    if (n0 + r < frames) out[(size_t)(n0 + r) * ld_out + c] = (T)xs[r * kPfLd + c];   // padding frames hold the zeros they were given
  }
}

}  // namespace

int launch_postfilter(hipStream_t st, int dtype, const void *mgc, long ld_in, const int32_t *lengths, int B, int Tmax, int D,
                      double alpha, const double *weight, const double *G, int fftlen, void *out, long ld_out) {
  const long frames = (long)B * Tmax;
  const unsigned blocks = (unsigned)((frames + kPfFrames - 1) / kPfFrames);
  if (dtype == MLPG_HIP_F64)
    hipLaunchKernelGGL(postfilter_kernel<double>, dim3(blocks), dim3(256), 0, st, (const double *)mgc, ld_in, lengths, frames, Tmax, D,
                       alpha, weight, G, fftlen, (double *)out, ld_out);
  else
    hipLaunchKernelGGL(postfilter_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float *)mgc, ld_in, lengths, frames, Tmax, D,
                       alpha, weight, G, fftlen, (float *)out, ld_out);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountPostfilter);
  return 0;
}

}  // namespace mlpg

using namespace mlpg;

namespace {

int refuse_limits(const char *who, int D, double alpha, int order, int fftlen) {
  switch (postfilter_check_limits(D, alpha, order, fftlen)) {
    case 0: return 0;
    case 1: set_error("%s: the number of coefficients must be in [1, %d] (got %d)", who, kPfMaxD, D); break;
    case 2: set_error("%s: fftlen must be a power of two in [%d, %d] (got %d)", who, kPfMinFft, kPfMaxFft, fftlen); break;
    case 3: set_error("%s: the order must be in [D - 1, fftlen) = [%d, %d) (got %d)", who, D - 1, fftlen, order); break;
    default: set_error("%s: |alpha| must be below 1 (got %g)", who, alpha); break;
  }
  return MLPG_HIP_EINVAL;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int mlpg_hip_postfilter_table(int D, double alpha, int order, int fftlen, double *G) {
  const char *who = "postfilter_table";
  if (int rc = refuse_limits(who, D, alpha, order, fftlen)) return rc;
  if (!G) {
    set_error("%s: NULL table pointer", who);
    return MLPG_HIP_EINVAL;
  }
  postfilter_table(D, alpha, order, fftlen, G);
  return 0;
}

__attribute__((visibility("default"))) int mlpg_hip_merlin_post_filter(int device, void *stream, int dtype, const void *mgc,
                                                                       int64_t ld_in, const int32_t *lengths, int B, int Tmax, int D,
                                                                       double alpha, const double *weight, const double *G,
                                                                       int fftlen, void *out, int64_t ld_out) {
  const char *who = "merlin_post_filter";
  // (the order went into G: any order the table builder accepts is fine here, D - 1 always is)
  if (int rc = refuse_limits(who, D, alpha, D - 1 < fftlen ? D - 1 : 0, fftlen)) return rc;
  if (int rc = check_dtype(who, dtype)) return rc;
  if (B < 0 || Tmax < 0 || ((int64_t)B * Tmax + kPfFrames - 1) / kPfFrames > 16777215LL /* 2^24 - 1 workgroups of 256 threads: a grid is 32 bits of threads, a larger one runs truncated and reports nothing */) {
    set_error("%s: bad batch shape (B = %d, Tmax = %d)", who, B, Tmax);
    return MLPG_HIP_EINVAL;
  }
  if (ld_in < D || ld_out < D) {
    set_error("%s: row strides must be at least D = %d (got ld_in = %lld, ld_out = %lld)", who, D, (long long)ld_in, (long long)ld_out);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || Tmax == 0) return 0;
  if (!mgc || !weight || !G || !out) {
    set_error("%s: NULL data pointer (mgc, weight, G and out are required)", who);
    return MLPG_HIP_EINVAL;
  }
  if (out == mgc && ld_in != ld_out) {
    set_error("%s: in place (out == mgc) needs equal row strides (got %lld and %lld)", who, (long long)ld_in, (long long)ld_out);
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_postfilter((hipStream_t)stream, dtype, mgc, (long)ld_in, lengths, B, Tmax, D, alpha, weight, G, fftlen, out, (long)ld_out);
}

}  // extern "C"
