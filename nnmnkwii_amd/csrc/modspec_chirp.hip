// Modulation spectrum at the DFT lengths that are no power of two, up to 2048: the chirp-z (Bluestein) transform on the in-LDS
// FFT of modspec_fft.h.  numpy's rfft / irfft, which the reference calls at preprocessing/modspec.py:44,104,156-166 and
// autograd/_impl/modspec.py:30-60, accept every n; so do the float64 entries, and this file is what keeps such an n off the
// O(n^2) sum of modspec_dft.hip.  Same workgroup as modspec_kernel -- 1024 threads per (utterance, PAIR of adjacent columns),
// z = x1 + i x2, the last pair of an odd D carries one column -- same four modes, same scalings and edge rules.
//
// With j k = (j^2 + k^2 - (k - j)^2) / 2 and w_j = exp(-i pi j^2 / n) the n-point DFT is
//
//   Z_k = w_k * sum_j (z_j w_j) conj(w_{k-j}),
//
// a convolution that a circular one of length M = 2^ceil(log2(2n - 1)) holds (n <= 2048: M <= 4096, the largest transform the
// LDS takes: (padded_len(M) + M) * 16 B = 135184 B at M = 4096, the footprint of modspec_kernel at n = 4096):
//
//   1. a_j = z_j w_j, j < T; 0 up to M                                   (stored bit-reversed)
//   2. A = FFT_M(a)
//   3. A_m *= F_m / M,  F = FFT_M(f),  f_m = f_{M-m} = conj(w_m), m < n; 0 in between   (stored bit-reversed again)
//   4. c = M * IFFT_M(A)
//   5. Z_k = w_k c_k, k < n
//
// The inverse n-point DFT is conj(DFT(conj Z)), so one pair of tables serves both directions.  Spectrum and inverse take two
// M-point FFTs per workgroup; smoothing and backward four (chirp forward, unpack2 / modify / pack2 at length n, chirp back).
// Nothing but the inputs, the two tables and the result touches HBM.
//
// The tables: w (n entries) and F / M (M entries; M is a power of two, so the division is exact), double2, <= 32 KB + 64 KB and
// therefore L2-resident across the workgroups of a launch.  chirp_table and chirp_filter build them in the stream's scratch in
// front of every launch, as launch_dft does with its roots of unity: nothing is remembered between calls, so nothing can go
// stale under stream capture or when the scratch moves.  The phase of w_j is reduced exactly as the integer j^2 mod 2n (32-bit
// arithmetic: j < 2048) before sincospi sees it -- the discipline of modspec_dft.hip's integer phase.
#include <math.h>

#include "modspec_fft.h"

namespace mlpg {
namespace chirp {

struct ChirpArgs {
  const double *x;     // spec/smooth/backward: (B, T, D) trajectory
  const double *ms;    // inverse: (B, n/2+1, D) power spectrum; backward: gradient w.r.t. the power spectrum
  const double *ph;    // inverse: (B, n/2+1, D, 2) unit phasors
  double *out;         // spec: (B, n/2+1, D) power; inverse: (B, n, D); smooth/backward: (B, T, D)
  double *out_ph;      // spec: (B, n/2+1, D, 2) phasors or NULL
  const double2 *w;    // w[j] = exp(-i pi j^2 / n), j < n
  const double2 *F;    // F[m] = FFT_M(f)[m] / M, m < M
  int B, T, D, n, M, logM;
  int ortho;           // norm == "ortho"
  int limit_bin;       // smooth: first removed bin (> n/2: none)
  int log_domain;      // smooth: removed bins get unit magnitude (exp(0)) instead of zero
};

// exp(-i pi j^2 / n), 0 <= j < n <= 2048: j^2 < 2^22, reduced mod 2n exactly
__device__ __forceinline__ Cplx chirp_phasor(int j, int n) {
  const unsigned r = ((unsigned)j * (unsigned)j) % (unsigned)(2 * n);
  double sn, cs;
  sincospi(-(double)r / (double)n, &sn, &cs);
  return {cs, sn};
}

__device__ __forceinline__ Cplx cmul2(Cplx a, double2 b) { return cmul(a, Cplx{b.x, b.y}); }
// conj(z) * w: the input side of the inverse transform, conj(DFT(conj Z))
__device__ __forceinline__ Cplx cmul2_conj(Cplx z, double2 w) { return {z.re * w.x + z.im * w.y, z.re * w.y - z.im * w.x}; }

__global__ void chirp_table(double2 *w, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const Cplx c = chirp_phasor(j, n);
  w[j] = make_double2(c.re, c.im);
}

// The M-point transforms of the chirp-z kernels, inlined into them: a call would put the callee's frame in private memory (the
// float64 power-of-two kernel's fft_inplace does), and a 1024-thread workgroup leaves a lane 128 registers.  With the radix-16
// first pass in registers (16 live complex values) the four instantiations take 98 / 122 / 100 / 100 VGPRs and no scratch; as
// fft16_two_sweeps (MLPG_CHIRP_SWEEPS=1) 78 / 98 / 80 / 80, at twice the LDS traffic of that pass.  Either way the LDS, not the
// registers, sets the occupancy (one workgroup per CU at M = 4096), so the default is the pass with less LDS traffic.
#ifndef MLPG_CHIRP_SWEEPS
#define MLPG_CHIRP_SWEEPS 0
#endif
template <bool INV>
__device__ __forceinline__ void chirp_fft(Cplx *a, const Cplx *tw, int M, int logM, int tid) {
  fft_inplace_body<INV, MLPG_CHIRP_SWEEPS != 0>(a, tw, M, logM, tid);
}

// One workgroup: f at its bit-reversed places, FFT_M in LDS, F / M out.  M >= 2n - 1 keeps the two wings of f apart.
__global__ __launch_bounds__(kFftThreads) void chirp_filter(double2 *F, int n, int M, int logM) {
  extern __shared__ __align__(16) unsigned char smem[];
  Cplx *a = (Cplx *)smem;
  Cplx *tw = a + padded_len(M);
  const int tid = threadIdx.x;
  build_twiddles(tw, logM, tid);
  for (int m = tid; m < M; m += kFftThreads) {
    const int q = m < n ? m : (M - m < n ? M - m : -1);
    Cplx f = {0.0, 0.0};
    if (q >= 0) {
      const Cplx c = chirp_phasor(q, n);
      f = {c.re, -c.im};
    }
    a[pidx(bitrev(m, logM))] = f;
  }
  __syncthreads();
  chirp_fft<false>(a, tw, M, logM, tid);
  const double inv_m = 1.0 / (double)M;
  for (int m = tid; m < M; m += kFftThreads) F[m] = make_double2(a[pidx(m)].re * inv_m, a[pidx(m)].im * inv_m);
}

// a (bit-reversed a_j in) -> c (natural order out, c_k for k < n; the rest is the convolution's wrap-around): steps 2-4.  The
// pointwise product and the bit reversal the inverse transform wants are one sweep: the thread of k < rev(k) owns both places.
__device__ __forceinline__ void chirp_convolve(Cplx *a, const Cplx *tw, const double2 *F, int M, int logM, int tid) {
  chirp_fft<false>(a, tw, M, logM, tid);
  for (int k = tid; k < M; k += kFftThreads) {
    const int r = bitrev(k, logM);
    if (r < k) continue;
    const Cplx ak = cmul2(a[pidx(k)], F[k]);
    if (r == k) {
      a[pidx(k)] = ak;
    } else {
      const Cplx ar = cmul2(a[pidx(r)], F[r]);
      a[pidx(k)] = ar;
      a[pidx(r)] = ak;
    }
  }
  __syncthreads();
  chirp_fft<true>(a, tw, M, logM, tid);
}

template <int MODE>
__global__ __launch_bounds__(kFftThreads) void modspec_chirp_kernel(ChirpArgs p) {
  extern __shared__ __align__(16) unsigned char smem[];
  Cplx *a = (Cplx *)smem;
  Cplx *tw = a + padded_len(p.M);
  const int tid = threadIdx.x;
  const int npair = (p.D + 1) / 2;
  const int d = 2 * (blockIdx.x % npair), b = blockIdx.x / npair;
  const bool two = d + 1 < p.D;  // the last pair of an odd D holds one column
  const int n = p.n, M = p.M, logM = p.logM, nb = n / 2 + 1, T = p.T, D = p.D;
  const int nyq = (n & 1) ? -1 : n / 2;  // the bin that is its own mirror besides 0 (even n only)
  const double2 *w = p.w;
  const double fwd_scale = p.ortho ? 1.0 / sqrt((double)n) : 1.0;
  const double inv_scale = p.ortho ? 1.0 / sqrt((double)n) : 1.0 / (double)n;

  build_twiddles(tw, logM, tid);

  if (MODE == kModeInverse) {
    // Hermitian spectra amp * phase of both columns (numpy's irfft ignores the imaginary part of bins 0 and, for even n,
    // n/2), packed as H1 + i H2; conj(DFT(conj .)) returns column 1 in the real and column 2 in the imaginary part
    const double *msb = p.ms + (size_t)b * nb * D + d;
    const double *phb = p.ph + ((size_t)b * nb * D + d) * 2;
    for (int k = tid; k < nb; k += kFftThreads) {
      const double a1 = sqrt(msb[(size_t)k * D]);
      Cplx h1 = {a1 * phb[(size_t)k * D * 2], a1 * phb[(size_t)k * D * 2 + 1]}, h2 = {0.0, 0.0};
      if (two) {
        const double a2 = sqrt(msb[(size_t)k * D + 1]);
        h2 = {a2 * phb[(size_t)k * D * 2 + 2], a2 * phb[(size_t)k * D * 2 + 3]};
      }
      if (k == 0 || k == nyq) h1.im = h2.im = 0.0;
      Cplx zk, zm;
      pack2(h1, h2, &zk, &zm);
      const int km = (n - k) % n;
      a[pidx(bitrev(k, logM))] = cmul2_conj(zk, w[k]);
      if (km != k) a[pidx(bitrev(km, logM))] = cmul2_conj(zm, w[km]);
    }
    for (int j = n + tid; j < M; j += kFftThreads) a[pidx(bitrev(j, logM))] = {0.0, 0.0};
    __syncthreads();
    chirp_convolve(a, tw, p.F, M, logM, tid);
    double *ob = p.out + (size_t)b * n * D + d;
    for (int t = tid; t < n; t += kFftThreads) {
      const Cplx y = cmul2(a[pidx(t)], w[t]);
      ob[(size_t)t * D] = y.re * inv_scale;
      if (two) ob[(size_t)t * D + 1] = -y.im * inv_scale;
    }
    return;
  }

  // forward transform of the two columns (T <= n frames; a_j = 0 from there to M)
  const double *xb = p.x + (size_t)b * T * D + d;
  for (int t = tid; t < M; t += kFftThreads) {
    Cplx z = {0.0, 0.0};
    if (t < T) {
      z.re = xb[(size_t)t * D];
      if (two) z.im = xb[(size_t)t * D + 1];
      z = cmul2(z, w[t]);
    }
    a[pidx(bitrev(t, logM))] = z;
  }
  __syncthreads();
  chirp_convolve(a, tw, p.F, M, logM, tid);

  if (MODE == kModeSpec) {
    double *ob = p.out + (size_t)b * nb * D + d;
    for (int k = tid; k < nb; k += kFftThreads) {
      const int km = (n - k) % n;
      Cplx s1, s2;
      unpack2(cmul2(a[pidx(k)], w[k]), cmul2(a[pidx(km)], w[km]), &s1, &s2);
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

  // both remaining modes rebuild Z' = H1 + i H2 from per-column Hermitian spectra, one thread per bin pair (k, n-k), and leave
  // conj(Z'_j) w_j -- the input of the transform back -- in natural order, zeros from n to M
  const double *gb = MODE == kModeBackward ? p.ms + (size_t)b * nb * D + d : nullptr;
  for (int k = tid; k < nb; k += kFftThreads) {
    const int km = (n - k) % n;
    const double2 wk = w[k], wm = w[km];
    Cplx s1, s2;
    unpack2(cmul2(a[pidx(k)], wk), cmul2(a[pidx(km)], wm), &s1, &s2);
    s1 = {s1.re * fwd_scale, s1.im * fwd_scale};
    s2 = {s2.re * fwd_scale, s2.im * fwd_scale};
    const bool edge = k == 0 || k == nyq;
    Cplx h1, h2;
    if (MODE == kModeSmooth) {
      // bins >= limit_bin: power := 0, or log-power := 0 (unit magnitude, phase kept) in the log domain
      h1 = s1;
      h2 = s2;
      if (k >= p.limit_bin) {
        h1 = p.log_domain ? unit_phasor(s1) : Cplx{0.0, 0.0};
        h2 = p.log_domain ? unit_phasor(s2) : Cplx{0.0, 0.0};
      }
      if (edge) h1.im = h2.im = 0.0;
    } else {
      // grad[t] = C Re sum_{k <= n/2} g_k S_k e^{+2 pi i k t / n}: as a Hermitian spectrum, g_k S_k / 2 at the bins that have
      // a mirror (and its conjugate there), Re(g_k S_k) at k = 0 and, for even n, n/2
      const double g1 = gb[(size_t)k * D], g2 = two ? gb[(size_t)k * D + 1] : 0.0;
      const double f = edge ? 1.0 : 0.5;
      h1 = {f * g1 * s1.re, edge ? 0.0 : f * g1 * s1.im};
      h2 = {f * g2 * s2.re, edge ? 0.0 : f * g2 * s2.im};
    }
    if (!two) h2 = {0.0, 0.0};
    Cplx zk, zm;
    pack2(h1, h2, &zk, &zm);
    a[pidx(k)] = cmul2_conj(zk, wk);
    if (km != k) a[pidx(km)] = cmul2_conj(zm, wm);
  }
  for (int j = n + tid; j < M; j += kFftThreads) a[pidx(j)] = {0.0, 0.0};
  __syncthreads();
  // the transform wants bit-reversed input: permute in place (swap pairs; member by member, so that no struct temporary of
  // the swap lands in private memory)
  for (int k = tid; k < M; k += kFftThreads) {
    const int r = bitrev(k, logM);
    if (r > k) {
      const double kre = a[pidx(k)].re, kim = a[pidx(k)].im, rre = a[pidx(r)].re, rim = a[pidx(r)].im;
      a[pidx(k)] = {rre, rim};
      a[pidx(r)] = {kre, kim};
    }
  }
  __syncthreads();
  chirp_convolve(a, tw, p.F, M, logM, tid);
  double *ob = p.out + (size_t)b * T * D + d;
  // smoothing: irfft scaling; backward: C = 2 (2 / sqrt(n) with "ortho"), autograd/_impl/modspec.py:47-49
  const double osc = MODE == kModeSmooth ? inv_scale : (p.ortho ? 2.0 / sqrt((double)n) : 2.0);
  for (int t = tid; t < T; t += kFftThreads) {
    const Cplx y = cmul2(a[pidx(t)], w[t]);
    ob[(size_t)t * D] = y.re * osc;
    if (two) ob[(size_t)t * D + 1] = -y.im * osc;
  }
}

template <int MODE>
int launch_mode(hipStream_t st, const ChirpArgs &p, size_t lds) {
  auto kern = modspec_chirp_kernel<MODE>;
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
    ChirpArgs q = p;
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

}  // namespace chirp

bool modspec_chirp_takes(int n) { return n >= 3 && n <= 2048 && (n & (n - 1)); }

int modspec_chirp_length(int n) {
  int M = 1;
  while (M < 2 * n - 1) M <<= 1;
  return M;
}

int launch_modspec_chirp(hipStream_t st, int device, int mode, const double *x, const double *ms, const double *ph, double *out,
                         double *out_ph, int B, int T, int D, int n, int ortho, int limit_bin, int log_domain) {
  using namespace chirp;
  if (!modspec_chirp_takes(n)) {
    set_error("modspec: the chirp-z transform takes a DFT length in [3, 2048] that is no power of two (got %d)", n);
    return MLPG_HIP_EINVAL;
  }
  if (mode < kModeSpec || mode > kModeBackward) {
    set_error("modspec: bad mode %d", mode);
    return MLPG_HIP_EINVAL;
  }
  if ((double)B * (double)((D + 1) / 2) > 2147483647.0) {
    set_error("modspec: B * ceil(D / 2) = %d * %d workgroups are more than one launch takes", B, (D + 1) / 2);
    return MLPG_HIP_EINVAL;
  }
  ChirpArgs p;
  p.x = x; p.ms = ms; p.ph = ph; p.out = out; p.out_ph = out_ph;
  p.B = B; p.T = T; p.D = D; p.n = n; p.M = modspec_chirp_length(n); p.logM = 0;
  while ((1 << p.logM) < p.M) ++p.logM;
  p.ortho = ortho; p.limit_bin = limit_bin; p.log_domain = log_domain;
  const size_t w_bytes = ((size_t)n * sizeof(double2) + 255) / 256 * 256;
  char *sc = (char *)scratch(device, st, 0, w_bytes + (size_t)p.M * sizeof(double2));
  if (!sc) return MLPG_HIP_ENOMEM;
  p.w = (const double2 *)sc;
  p.F = (const double2 *)(sc + w_bytes);
  const size_t lds = sizeof(Cplx) * ((size_t)padded_len(p.M) + (size_t)p.M);  // data + per-pass twiddle tables (< M entries)
  hipLaunchKernelGGL(chirp_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (double2 *)sc, n);
  MLPG_HIP_CHECK(hipGetLastError());
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)chirp_filter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(chirp_filter, dim3(1), dim3(kFftThreads), lds, st, (double2 *)(sc + w_bytes), n, p.M, p.logM);
  MLPG_HIP_CHECK(hipGetLastError());
  switch (mode) {
    case kModeSpec: return launch_mode<kModeSpec>(st, p, lds);
    case kModeInverse: return launch_mode<kModeInverse>(st, p, lds);
    case kModeSmooth: return launch_mode<kModeSmooth>(st, p, lds);
    default: return launch_mode<kModeBackward>(st, p, lds);
  }
}

}  // namespace mlpg
