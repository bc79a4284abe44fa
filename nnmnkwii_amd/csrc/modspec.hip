// Modulation-spectrum kernels: the step after MLPG in the reference's
// pipelines.  Replace preprocessing/modspec.py (modspec :6-53, inv_modspec :62-100,
// modspec_smoothing :103-167: numpy rfft / irfft along the time axis of a (T, D) trajectory) and
// the Python loop over feature dimensions in autograd/_impl/modspec.py:30-60.
//
// One workgroup per (utterance, PAIR of adjacent feature columns): the two real columns are
// zero-padded to the DFT length n (a power of two <= 4096) and packed as real and imaginary part
// of ONE complex sequence z = x1 + i x2, transformed by a complex FFT that lives entirely in LDS
// (n points of 16 bytes + per-pass twiddle tables), separated (X1_k = (Z_k + conj Z_{n-k}) / 2,
// X2_k = (Z_k - conj Z_{n-k}) / 2i), modified, and -- for smoothing and for the backward --
// recombined and transformed back without leaving the chip.  HBM traffic is the trajectory in and
// the result out.
//
// FFT: modspec_fft.h (in-place decimation in time on bit-reversed input, in LDS, free of bank conflicts by construction).
#include <math.h>

#include "modspec_fft.h"

namespace mlpg {
namespace {

struct ModArgs {
  const double *x;     // spec/smooth/backward: (B, T, D) trajectory
  const double *ms;    // inverse: (B, n/2+1, D) power spectrum; backward: gradient w.r.t. the power spectrum
  const double *ph;    // inverse: (B, n/2+1, D, 2) unit phasors
  double *out;         // spec: (B, n/2+1, D) power; inverse: (B, n, D); smooth/backward: (B, T, D)
  double *out_ph;      // spec: (B, n/2+1, D, 2) phasors or NULL
  int B, T, D, n, logn;
  int ortho;           // norm == "ortho"
  int limit_bin;       // smooth: first removed bin (> n/2: none)
  int log_domain;      // smooth: removed bins get unit magnitude (exp(0)) instead of zero
};

template <int MODE>
__global__ __launch_bounds__(kFftThreads) void modspec_kernel(ModArgs p) {
  extern __shared__ __align__(16) unsigned char smem[];
  Cplx *a = (Cplx *)smem;
  Cplx *tw = a + padded_len(p.n);
  const int tid = threadIdx.x;
  const int npair = (p.D + 1) / 2;
  const int d = 2 * (blockIdx.x % npair), b = blockIdx.x / npair;
  const bool two = d + 1 < p.D;  // the last pair of an odd D holds one column
  const int n = p.n, logn = p.logn, nb = n / 2 + 1, T = p.T, D = p.D;
  const double fwd_scale = p.ortho ? 1.0 / sqrt((double)n) : 1.0;
  const double inv_scale = p.ortho ? 1.0 / sqrt((double)n) : 1.0 / (double)n;

  build_twiddles(tw, logn, tid);

  if (MODE == kModeInverse) {
    // Hermitian spectra amp * phase of both columns (numpy's irfft ignores the imaginary part of bins 0 and
    // n/2), packed as H1 + i H2: one inverse transform returns column 1 in the real and column 2 in the
    // imaginary part
    const double *msb = p.ms + (size_t)b * nb * D + d;
    const double *phb = p.ph + ((size_t)b * nb * D + d) * 2;
    for (int k = tid; k < nb; k += kFftThreads) {
      const double a1 = sqrt(msb[(size_t)k * D]);
      Cplx h1 = {a1 * phb[(size_t)k * D * 2], a1 * phb[(size_t)k * D * 2 + 1]}, h2 = {0.0, 0.0};
      if (two) {
        const double a2 = sqrt(msb[(size_t)k * D + 1]);
        h2 = {a2 * phb[(size_t)k * D * 2 + 2], a2 * phb[(size_t)k * D * 2 + 3]};
      }
      if (k == 0 || k == n / 2) h1.im = h2.im = 0.0;
      Cplx zk, zm;
      pack2(h1, h2, &zk, &zm);
      a[pidx(bitrev(k, logn))] = zk;
      if (k != 0 && k != n / 2) a[pidx(bitrev(n - k, logn))] = zm;
    }
    __syncthreads();
    fft_inplace<true>(a, tw, n, logn, tid);
    double *ob = p.out + (size_t)b * n * D + d;
    for (int t = tid; t < n; t += kFftThreads) {
      ob[(size_t)t * D] = a[pidx(t)].re * inv_scale;
      if (two) ob[(size_t)t * D + 1] = a[pidx(t)].im * inv_scale;
    }
    return;
  }

  // forward transform of the two zero-padded columns
  const double *xb = p.x + (size_t)b * T * D + d;
  for (int t = tid; t < n; t += kFftThreads) {
    Cplx z = {0.0, 0.0};
    if (t < T) {
      z.re = xb[(size_t)t * D];
      if (two) z.im = xb[(size_t)t * D + 1];
    }
    a[pidx(bitrev(t, logn))] = z;
  }
  __syncthreads();
  fft_inplace<false>(a, tw, n, logn, tid);

  if (MODE == kModeSpec) {
    double *ob = p.out + (size_t)b * nb * D + d;
    for (int k = tid; k < nb; k += kFftThreads) {
      Cplx s1, s2;
      unpack2(a[pidx(k)], a[pidx((n - k) & (n - 1))], &s1, &s2);
      s1 = {s1.re * fwd_scale, s1.im * fwd_scale};
      s2 = {s2.re * fwd_scale, s2.im * fwd_scale};
      ob[(size_t)k * D] = s1.re * s1.re + s1.im * s1.im;
      if (two) ob[(size_t)k * D + 1] = s2.re * s2.re + s2.im * s2.im;
      if (p.out_ph) {
        double *pp = p.out_ph + ((size_t)b * nb * D + (size_t)k * D + d) * 2;
        const Cplx u1 = unit_phasor(s1);
        pp[0] = u1.re;
        pp[1] = u1.im;
        if (two) {
          const Cplx u2 = unit_phasor(s2);
          pp[2] = u2.re;
          pp[3] = u2.im;
        }
      }
    }
    return;
  }

  // both remaining modes rebuild Z' = H1 + i H2 from per-column Hermitian spectra, one thread per bin pair (k, n-k)
  const double *gb = MODE == kModeBackward ? p.ms + (size_t)b * nb * D + d : nullptr;
  for (int k = tid; k < nb; k += kFftThreads) {
    const int km = (n - k) & (n - 1);
    Cplx s1, s2;
    unpack2(a[pidx(k)], a[pidx(km)], &s1, &s2);
    s1 = {s1.re * fwd_scale, s1.im * fwd_scale};
    s2 = {s2.re * fwd_scale, s2.im * fwd_scale};
    Cplx h1, h2;
    if (MODE == kModeSmooth) {
      // bins >= limit_bin: power := 0, or log-power := 0 (unit magnitude, phase kept) in the log domain
      h1 = s1;
      h2 = s2;
      if (k >= p.limit_bin) {
        h1 = p.log_domain ? unit_phasor(s1) : Cplx{0.0, 0.0};
        h2 = p.log_domain ? unit_phasor(s2) : Cplx{0.0, 0.0};
      }
      if (k == 0 || k == n / 2) h1.im = h2.im = 0.0;
    } else {
      // grad[t] = C Re sum_{k <= n/2} g_k S_k e^{+2 pi i k t / n}: as a Hermitian spectrum, g_k S_k / 2 at
      // 0 < k < n/2 (and its conjugate at n-k), Re(g_k S_k) at k = 0 and n/2
      const double g1 = gb[(size_t)k * D], g2 = two ? gb[(size_t)k * D + 1] : 0.0;
      const bool edge = k == 0 || k == n / 2;
      const double f = edge ? 1.0 : 0.5;
      h1 = {f * g1 * s1.re, edge ? 0.0 : f * g1 * s1.im};
      h2 = {f * g2 * s2.re, edge ? 0.0 : f * g2 * s2.im};
    }
    if (!two) h2 = {0.0, 0.0};
    Cplx zk, zm;
    pack2(h1, h2, &zk, &zm);
    a[pidx(k)] = zk;
    if (km != k) a[pidx(km)] = zm;
  }
  __syncthreads();
  // the inverse transform wants bit-reversed input: permute in place (swap pairs)
  for (int k = tid; k < n; k += kFftThreads) {
    const int r = bitrev(k, logn);
    if (r > k) {
      const Cplx t = a[pidx(k)];
      a[pidx(k)] = a[pidx(r)];
      a[pidx(r)] = t;
    }
  }
  __syncthreads();
  fft_inplace<true>(a, tw, n, logn, tid);
  double *ob = p.out + (size_t)b * T * D + d;
  // smoothing: irfft scaling; backward: C = 2 (2 / sqrt(n) with "ortho"), autograd/_impl/modspec.py:47-49
  const double osc = MODE == kModeSmooth ? inv_scale : (p.ortho ? 2.0 / sqrt((double)n) : 2.0);
  for (int t = tid; t < T; t += kFftThreads) {
    ob[(size_t)t * D] = a[pidx(t)].re * osc;
    if (two) ob[(size_t)t * D + 1] = a[pidx(t)].im * osc;
  }
}

template <int MODE>
int launch_mode(hipStream_t st, const ModArgs &p) {
  const size_t lds = sizeof(Cplx) * ((size_t)padded_len(p.n) + (size_t)p.n);  // data + per-pass twiddle tables (< n entries)
  auto kern = modspec_kernel<MODE>;
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // one launch per slice of whole sequences, each under the grid's thread limit: the kernel sees a shorter batch at offset bases
  const long npair = (p.D + 1) / 2, step = items_per_launch(npair, kFftThreads);
  if (step < 1) {
    set_error("modspec: ceil(D / 2) = %ld workgroups of %d threads per sequence are more than one launch takes (%ld)", npair,
              kFftThreads, max_workgroups(kFftThreads));
    return MLPG_HIP_EINVAL;
  }
  const size_t nb = (size_t)p.n / 2 + 1, D = (size_t)p.D;
  const size_t out_rows = MODE == kModeSpec ? nb : MODE == kModeInverse ? (size_t)p.n : (size_t)p.T;
  for (long b0 = 0; b0 < p.B; b0 += step) {
    ModArgs q = p;
    q.B = (int)(p.B - b0 < step ? p.B - b0 : step);
    if (p.x) q.x = p.x + (size_t)b0 * p.T * D;
    if (p.ms) q.ms = p.ms + (size_t)b0 * nb * D;
    if (p.ph) q.ph = p.ph + (size_t)b0 * nb * D * 2;
    if (p.out_ph) q.out_ph = p.out_ph + (size_t)b0 * nb * D * 2;
    q.out = p.out + (size_t)b0 * out_rows * D;
    hipLaunchKernelGGL(kern, dim3((unsigned)(q.B * npair)), dim3(kFftThreads), lds, st, q);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace

int launch_modspec(hipStream_t st, int mode, const double *x, const double *ms, const double *ph, double *out,
                   double *out_ph, int B, int T, int D, int n, int ortho, int limit_bin, int log_domain) {
  int logn = 0;
  while ((1 << logn) < n) ++logn;
  if (n < 2 || n > 4096 || (1 << logn) != n) {
    set_error("modspec: the DFT length must be a power of two in [2, 4096] (got %d)", n);
    return MLPG_HIP_EINVAL;
  }
  ModArgs p;
  p.x = x; p.ms = ms; p.ph = ph; p.out = out; p.out_ph = out_ph;
  p.B = B; p.T = T; p.D = D; p.n = n; p.logn = logn;
  p.ortho = ortho; p.limit_bin = limit_bin; p.log_domain = log_domain;
  switch (mode) {
    case kModeSpec: return launch_mode<kModeSpec>(st, p);
    case kModeInverse: return launch_mode<kModeInverse>(st, p);
    case kModeSmooth: return launch_mode<kModeSmooth>(st, p);
    case kModeBackward: return launch_mode<kModeBackward>(st, p);
  }
  set_error("modspec: bad mode %d", mode);
  return MLPG_HIP_EINVAL;
}

// ---- padded minibatches, typed (mlpg_hip_modspec_batch, _batch_backward, _loss_step) -----------------------------------
// What a training loop needs behind the batched MLPG nodes and the reference does not have (autograd/_impl/modspec.py:9-72 and
// preprocessing/modspec.py:6-53 take ONE (T, D) array): the same workgroup per (utterance, pair of columns) and the same FFT,
// with x loaded and the result stored as float32 or float64 (arithmetic in float64), an optional per-utterance length, and the
// whole log-MS loss step as one mode.  Utterance b contributes the frames t < live = min(lengths[b], n, Tmax) -- rfft(x[:len], n)
// with its crop at n; a row at or past `live` is never loaded.  The gradient modes write every row of grad_x: the value below
// `live`, 0 from there to Tmax (the row stride; Tmax > n is fine).
//
// kBatchLoss, per workgroup:  z = x1 + i x2 -> FFT -> S1, S2 (unpack2, forward scale) -> P = |S|^2, Pt = target_ms ->
//   r = f(P) - f(Pt), f = log(. + eps) | identity -> sum r^2 (registers -> wave shuffle -> 16 doubles of LDS -> partial[wg]);
//   g = 2 r f'(P) / n_elems -> Hermitian g S (interior bins halved, edge bins real: the backward mode's rule) -> pack2 ->
//   bit reversal -> inverse FFT -> grad_x.  Nothing but x, target_ms and grad_x touches HBM.  modspec_loss_finalize then adds
//   the partials in a fixed order (one workgroup, strided sums, LDS tree) and writes sum / n_elems: repeatable bit for bit.
namespace {

enum { kBatchSpec = 0, kBatchBackward = 1, kBatchLoss = 2 };

struct BatchArgs {
  const void *x;           // (B, Tmax, D) of TX
  const void *aux;         // backward: grad_ms, loss: target_ms -- (B, n/2+1, D) of TX
  const int32_t *lengths;  // int32[B] or NULL
  void *out;               // spec: ms (B, n/2+1, D); backward / loss: grad_x (B, Tmax, D) -- of TX
  double *partial;         // loss: sum of r^2 per workgroup
  int B, T, D, n, logn;    // T: Tmax, the row count of x and grad_x
  int ortho, log_domain;
  double eps, inv_elems;   // loss: 1 / n_elems
};

template <int MODE, typename TX>
__global__ __launch_bounds__(kFftThreads) void modspec_batch_kernel(BatchArgs p) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red[kFftThreads / 64];
  Cplx *a = (Cplx *)smem;
  Cplx *tw = a + padded_len(p.n);
  const int tid = threadIdx.x;
  const int npair = (p.D + 1) / 2;
  const int d = 2 * (blockIdx.x % npair), b = blockIdx.x / npair;
  const bool two = d + 1 < p.D;  // the last pair of an odd D holds one column
  const int n = p.n, logn = p.logn, nb = n / 2 + 1, T = p.T, D = p.D;
  const double fwd_scale = p.ortho ? 1.0 / sqrt((double)n) : 1.0;
  int live = T < n ? T : n;
  if (p.lengths) {
    const int len = p.lengths[b];
    live = len < live ? (len > 0 ? len : 0) : live;
  }

  build_twiddles(tw, logn, tid);

  const TX *xb = (const TX *)p.x + (size_t)b * T * D + d;
  for (int t = tid; t < n; t += kFftThreads) {
    Cplx z = {0.0, 0.0};
    if (t < live) {
      z.re = (double)xb[(size_t)t * D];
      if (two) z.im = (double)xb[(size_t)t * D + 1];
    }
    a[pidx(bitrev(t, logn))] = z;
  }
  __syncthreads();
  fft_inplace_body<false, true>(a, tw, n, logn, tid);

  if (MODE == kBatchSpec) {
    TX *ob = (TX *)p.out + (size_t)b * nb * D + d;
    for (int k = tid; k < nb; k += kFftThreads) {
      Cplx s1, s2;
      unpack2(a[pidx(k)], a[pidx((n - k) & (n - 1))], &s1, &s2);
      s1 = {s1.re * fwd_scale, s1.im * fwd_scale};
      s2 = {s2.re * fwd_scale, s2.im * fwd_scale};
      ob[(size_t)k * D] = (TX)(s1.re * s1.re + s1.im * s1.im);
      if (two) ob[(size_t)k * D + 1] = (TX)(s2.re * s2.re + s2.im * s2.im);
    }
    return;
  }

  // one thread per bin pair (k, n-k): Z' = H1 + i H2 of the Hermitian spectra g S of both columns
  const TX *gb = (const TX *)p.aux + (size_t)b * nb * D + d;
  double rsum = 0.0;
  for (int k = tid; k < nb; k += kFftThreads) {
    const int km = (n - k) & (n - 1);
    Cplx s1, s2;
    unpack2(a[pidx(k)], a[pidx(km)], &s1, &s2);
    s1 = {s1.re * fwd_scale, s1.im * fwd_scale};
    s2 = {s2.re * fwd_scale, s2.im * fwd_scale};
    double g1 = (double)gb[(size_t)k * D], g2 = two ? (double)gb[(size_t)k * D + 1] : 0.0;
    if (MODE == kBatchLoss) {
      // g1, g2 hold the target powers: r = f(P) - f(Pt), g = 2 r f'(P) / n_elems
      const double p1 = s1.re * s1.re + s1.im * s1.im, p2 = s2.re * s2.re + s2.im * s2.im;
      double r1, r2, f1 = 1.0, f2 = 1.0;
      if (p.log_domain) {
        r1 = log(p1 + p.eps) - log(g1 + p.eps);
        r2 = log(p2 + p.eps) - log(g2 + p.eps);
        f1 = 1.0 / (p1 + p.eps);
        f2 = 1.0 / (p2 + p.eps);
      } else {
        r1 = p1 - g1;
        r2 = p2 - g2;
      }
      if (!two) r2 = 0.0;
      rsum += r1 * r1 + r2 * r2;
      g1 = 2.0 * r1 * f1 * p.inv_elems;
      g2 = 2.0 * r2 * f2 * p.inv_elems;
    }
    const bool edge = k == 0 || k == n / 2;
    const double f = edge ? 1.0 : 0.5;
    const Cplx h1 = {f * g1 * s1.re, edge ? 0.0 : f * g1 * s1.im};
    const Cplx h2 = two ? Cplx{f * g2 * s2.re, edge ? 0.0 : f * g2 * s2.im} : Cplx{0.0, 0.0};
    Cplx zk, zm;
    pack2(h1, h2, &zk, &zm);
    a[pidx(k)] = zk;
    if (km != k) a[pidx(km)] = zm;
  }
  if (MODE == kBatchLoss) {
    // fixed order: lanes of a wave by xor shuffles, then the 16 wave sums by thread 0
    for (int off = 32; off > 0; off >>= 1) rsum += __shfl_xor(rsum, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = rsum;
  }
  __syncthreads();
  if (MODE == kBatchLoss && tid == 0) {
    double s = 0.0;
    for (int w = 0; w < kFftThreads / 64; ++w) s += red[w];
    p.partial[blockIdx.x] = s;
  }
  // the inverse transform wants bit-reversed input: permute in place (swap pairs)
  for (int k = tid; k < n; k += kFftThreads) {
    const int r = bitrev(k, logn);
    if (r > k) {  // (member by member: a struct temporary of the swap would be the kernel's only private memory)
      const double kre = a[pidx(k)].re, kim = a[pidx(k)].im, rre = a[pidx(r)].re, rim = a[pidx(r)].im;
      a[pidx(k)] = {rre, rim};
      a[pidx(r)] = {kre, kim};
    }
  }
  __syncthreads();
  fft_inplace_body<true, true>(a, tw, n, logn, tid);
  TX *ob = (TX *)p.out + (size_t)b * T * D + d;
  const double osc = p.ortho ? 2.0 / sqrt((double)n) : 2.0;  // C of autograd/_impl/modspec.py:47-49
  for (int t = tid; t < T; t += kFftThreads) {
    const bool on = t < live;  // (live <= n: a[] is only read inside the transform)
    ob[(size_t)t * D] = (TX)(on ? a[pidx(t)].re * osc : 0.0);
    if (two) ob[(size_t)t * D + 1] = (TX)(on ? a[pidx(t)].im * osc : 0.0);
  }
}

// loss = (sum of the workgroups' partial sums) / n_elems, in one fixed order: thread i adds partial[i], partial[i + 256], ...,
// then a tree over the 256 sums
__global__ __launch_bounds__(256) void modspec_loss_finalize(const double *partial, int count, double inv_elems, double *loss) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < count; i += 256) acc += partial[i];
  s[tid] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) s[tid] += s[tid + h];
    __syncthreads();
  }
  if (tid == 0) *loss = s[0] * inv_elems;
}

template <int MODE, typename TX>
int launch_batch_mode(hipStream_t st, const BatchArgs &p) {
  const size_t lds = sizeof(Cplx) * ((size_t)padded_len(p.n) + (size_t)p.n);  // data + per-pass twiddle tables (< n entries)
  auto kern = modspec_batch_kernel<MODE, TX>;
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // one launch per slice of whole utterances, each under the grid's thread limit: the kernel sees a shorter batch at offset
  // bases (the loss mode's partial sums keep their places, so the finish step adds them in the order of one launch)
  const long npair = (p.D + 1) / 2, step = items_per_launch(npair, kFftThreads);
  if (step < 1) {
    set_error("modspec_batch: ceil(D / 2) = %ld workgroups of %d threads per utterance are more than one launch takes (%ld)", npair,
              kFftThreads, max_workgroups(kFftThreads));
    return MLPG_HIP_EINVAL;
  }
  const size_t nb = (size_t)p.n / 2 + 1, D = (size_t)p.D;
  for (long b0 = 0; b0 < p.B; b0 += step) {
    BatchArgs q = p;
    q.B = (int)(p.B - b0 < step ? p.B - b0 : step);
    if (p.x) q.x = (const TX *)p.x + (size_t)b0 * p.T * D;
    if (p.aux) q.aux = (const TX *)p.aux + (size_t)b0 * nb * D;
    if (p.lengths) q.lengths = p.lengths + b0;
    if (p.out) q.out = (TX *)p.out + (size_t)b0 * (MODE == kBatchSpec ? nb : (size_t)p.T) * D;
    if (p.partial) q.partial = p.partial + (size_t)b0 * npair;
    hipLaunchKernelGGL(kern, dim3((unsigned)(q.B * npair)), dim3(kFftThreads), lds, st, q);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

template <typename TX>
int launch_batch_typed(hipStream_t st, int mode, const BatchArgs &p) {
  switch (mode) {
    case kBatchSpec: return launch_batch_mode<kBatchSpec, TX>(st, p);
    case kBatchBackward: return launch_batch_mode<kBatchBackward, TX>(st, p);
    case kBatchLoss: return launch_batch_mode<kBatchLoss, TX>(st, p);
  }
  set_error("modspec_batch: bad mode %d", mode);
  return MLPG_HIP_EINVAL;
}

}  // namespace

bool modspec_fft_takes(int n) { return n >= 2 && n <= 4096 && !(n & (n - 1)); }

int launch_modspec_batch(hipStream_t st, int mode, int dtype, const void *x, const void *aux, const int32_t *lengths, void *out,
                         int B, int Tmax, int D, int n, int ortho, int log_domain, double eps, double n_elems, double *partial,
                         double *loss) {
  if (!modspec_fft_takes(n)) {
    set_error("modspec_batch: the in-LDS FFT takes a power of two in [2, 4096] (got %d)", n);
    return MLPG_HIP_EINVAL;
  }
  int logn = 0;
  while ((1 << logn) < n) ++logn;
  BatchArgs p;
  p.x = x; p.aux = aux; p.lengths = lengths; p.out = out; p.partial = partial;
  p.B = B; p.T = Tmax; p.D = D; p.n = n; p.logn = logn;
  p.ortho = ortho; p.log_domain = log_domain;
  p.eps = eps; p.inv_elems = mode == kBatchLoss ? 1.0 / n_elems : 0.0;
  if (int rc = dtype == MLPG_HIP_F32 ? launch_batch_typed<float>(st, mode, p) : launch_batch_typed<double>(st, mode, p)) return rc;
  note_launch(mode == kBatchLoss ? kCountModspecLoss : kCountModspecBatch);
  if (mode == kBatchLoss) {
    hipLaunchKernelGGL(modspec_loss_finalize, dim3(1), dim3(256), 0, st, (const double *)partial, B * ((D + 1) / 2), p.inv_elems, loss);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace mlpg
