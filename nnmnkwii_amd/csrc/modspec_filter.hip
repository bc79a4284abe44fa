// The modulation-spectrum filter over a padded minibatch (K9; mlpg_hip_modspec_filter, declared in include/mlpg_hip.h): the
// post-filter that moves the log modulation spectrum of a generated trajectory toward natural-speech statistics (Takamichi et
// al., ICASSP 2014 / TASLP 2016 -- the application preprocessing/modspec.py's docstring cites) and the low-pass smoothing of
// modspec_smoothing (:103-167), in one launch, on the primitives of modspec_fft.h.
//
// One workgroup per (utterance, PAIR of adjacent feature columns), z = x1 + i x2 as in modspec.hip:
//   typed load of the rows t < live = min(lengths[b], Tmax) (zero from there to n) -> forward FFT in LDS -> unpack2, forward scale
//   -> per bin k and column d, with P = |S|^2:
//        k <  limit_bin, tables given:  S' = S * exp(((A[k,d] - 1) log P + C[k,d]) / 2)   (P' = exp(A log P + C), phase kept;
//                                       a bin with P == 0 stays 0)
//        k <  limit_bin, no tables:     S' = S
//        k >= limit_bin:                S' = S / |S| in the log domain (log-power := 0; a zero bin gives 1, numpy's angle(0) = 0),
//                                       else 0 -- the rule of modspec.hip's smoothing mode
//   -> edge bins real -> pack2 -> bit reversal -> inverse FFT -> typed store: y[t] for t < live, exactly 0 for live <= t < Tmax.
// x and out are column slices of wider row-major matrices (row strides ld_x, ld_out in elements); out == x with equal strides is
// in place: a workgroup holds its two columns in LDS before it stores them and no other workgroup touches them.  Only x, the two
// tables and the result touch HBM.  A row at or past `live` is never loaded.
#include <math.h>

#include "modspec_fft.h"

namespace mlpg {
namespace {

struct FilterArgs {
  const void *x;           // (B, T, ld_x) of TX, columns [0, D)
  const int32_t *lengths;  // int32[B] or NULL
  const double *A, *C;     // (n/2+1, D) tables, both or neither
  void *out;               // (B, T, ld_out) of TX, columns [0, D)
  long ld_x, ld_out;
  int B, T, D, n, logn;    // T: Tmax <= n
  int ortho, limit_bin, log_domain;
};

// S' of one column at bin k (s: the scaled spectrum value)
__device__ __forceinline__ Cplx filter_bin(Cplx s, bool removed, bool log_domain, const double *A, const double *C, size_t at) {
  if (removed) return log_domain ? unit_phasor(s) : Cplx{0.0, 0.0};
  if (!A) return s;
  const double pw = s.re * s.re + s.im * s.im;
  if (!(pw > 0.0)) return pw == 0.0 ? Cplx{0.0, 0.0} : s;  // (a NaN goes through as it is)
  const double g = exp(0.5 * ((A[at] - 1.0) * log(pw) + C[at]));
  return {s.re * g, s.im * g};
}

template <typename TX>
__global__ __launch_bounds__(kFftThreads) void modspec_filter_kernel(FilterArgs p) {
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
  int live = T;  // (T <= n: the entry point refuses anything else)
  if (p.lengths) {
    const int len = p.lengths[b];
    live = len < live ? (len > 0 ? len : 0) : live;
  }
  TX *ob = (TX *)p.out + (size_t)b * T * p.ld_out + d;
  if (live == 0) {  // nothing to compute (uniform over the workgroup)
    for (int t = tid; t < T; t += kFftThreads) {
      ob[(size_t)t * p.ld_out] = (TX)0.0;
      if (two) ob[(size_t)t * p.ld_out + 1] = (TX)0.0;
    }
    return;
  }

  build_twiddles(tw, logn, tid);

  const TX *xb = (const TX *)p.x + (size_t)b * T * p.ld_x + d;
  for (int t = tid; t < n; t += kFftThreads) {
    Cplx z = {0.0, 0.0};
    if (t < live) {
      z.re = (double)xb[(size_t)t * p.ld_x];
      if (two) z.im = (double)xb[(size_t)t * p.ld_x + 1];
    }
    a[pidx(bitrev(t, logn))] = z;
  }
  __syncthreads();
  fft_inplace_body<false, true>(a, tw, n, logn, tid);

  // one thread per bin pair (k, n-k): Z' = H1 + i H2 of the filtered Hermitian spectra of both columns
  for (int k = tid; k < nb; k += kFftThreads) {
    const int km = (n - k) & (n - 1);
    Cplx s1, s2;
    unpack2(a[pidx(k)], a[pidx(km)], &s1, &s2);
    s1 = {s1.re * fwd_scale, s1.im * fwd_scale};
    s2 = {s2.re * fwd_scale, s2.im * fwd_scale};
    const bool removed = k >= p.limit_bin;
    const size_t at = (size_t)k * D + d;
    Cplx h1 = filter_bin(s1, removed, p.log_domain != 0, p.A, p.C, at);
    Cplx h2 = two ? filter_bin(s2, removed, p.log_domain != 0, p.A, p.C, at + 1) : Cplx{0.0, 0.0};
    if (k == 0 || k == n / 2) h1.im = h2.im = 0.0;
    Cplx zk, zm;
    pack2(h1, h2, &zk, &zm);
    a[pidx(k)] = zk;
    if (km != k) a[pidx(km)] = zm;
  }
  __syncthreads();
  // the inverse transform wants bit-reversed input: permute in place (swap pairs)
  for (int k = tid; k < n; k += kFftThreads) {
    const int r = bitrev(k, logn);
    if (r > k) {  // (member by member, as modspec_batch_kernel: no struct temporary in private memory)
      const double kre = a[pidx(k)].re, kim = a[pidx(k)].im, rre = a[pidx(r)].re, rim = a[pidx(r)].im;
      a[pidx(k)] = {rre, rim};
      a[pidx(r)] = {kre, kim};
    }
  }
  __syncthreads();
  fft_inplace_body<true, true>(a, tw, n, logn, tid);
  for (int t = tid; t < T; t += kFftThreads) {
    const bool on = t < live;  // (live <= T <= n)
    ob[(size_t)t * p.ld_out] = (TX)(on ? a[pidx(t)].re * inv_scale : 0.0);
    if (two) ob[(size_t)t * p.ld_out + 1] = (TX)(on ? a[pidx(t)].im * inv_scale : 0.0);
  }
}

template <typename TX>
int launch_filter_typed(hipStream_t st, const FilterArgs &p) {
  const size_t lds = sizeof(Cplx) * ((size_t)padded_len(p.n) + (size_t)p.n);  // data + per-pass twiddle tables (< n entries)
  auto kern = modspec_filter_kernel<TX>;
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // one launch per slice of whole utterances, each under the grid's thread limit: the kernel sees a shorter batch at offset bases
  const long npair = (p.D + 1) / 2, step = items_per_launch(npair, kFftThreads);
  if (step < 1) {
    set_error("modspec_filter: ceil(D / 2) = %ld workgroups of %d threads per utterance are more than one launch takes (%ld)", npair,
              kFftThreads, max_workgroups(kFftThreads));
    return MLPG_HIP_EINVAL;
  }
  for (long b0 = 0; b0 < p.B; b0 += step) {
    FilterArgs q = p;
    q.B = (int)(p.B - b0 < step ? p.B - b0 : step);
    q.x = (const TX *)p.x + (size_t)b0 * p.T * p.ld_x;
    q.out = (TX *)p.out + (size_t)b0 * p.T * p.ld_out;
    if (p.lengths) q.lengths = p.lengths + b0;
    hipLaunchKernelGGL(kern, dim3((unsigned)(q.B * npair)), dim3(kFftThreads), lds, st, q);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

int launch_modspec_filter(hipStream_t st, int dtype, const FilterArgs &p) {
  if (int rc = dtype == MLPG_HIP_F32 ? launch_filter_typed<float>(st, p) : launch_filter_typed<double>(st, p)) return rc;
  note_launch(kCountModspecFilter);
  return 0;
}

bool filter_form(int n) { return modspec_fft_takes(n) && !modspec_direct(); }

}  // namespace
}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int mlpg_hip_modspec_filter_form(int n) { return filter_form(n) ? 1 : 0; }

__attribute__((visibility("default"))) int mlpg_hip_modspec_filter(int device, void *stream, int dtype, const void *x, int64_t ld_x,
                                                                   const int32_t *lengths, int B, int Tmax, int D, int n, int ortho,
                                                                   const double *A, const double *C, int limit_bin, int log_domain,
                                                                   void *out, int64_t ld_out) {
  const char *who = "modspec_filter";
  if (int rc = check_dtype(who, dtype)) return rc;
  if (B < 0 || Tmax < 0 || D < 0) {
    set_error("%s: negative size (B=%d, Tmax=%d, D=%d)", who, B, Tmax, D);
    return MLPG_HIP_EINVAL;
  }
  if (!filter_form(n)) {
    set_error("%s: takes a power of two in [2, 4096] on the FFT route (n=%d, mlpg_hip_modspec_filter_form answers 0): compose "
              "mlpg_hip_modspec and mlpg_hip_inv_modspec", who, n);
    return MLPG_HIP_EINVAL;
  }
  if (Tmax > n) {
    set_error("%s: DFT length %d must not be smaller than the time length %d", who, n, Tmax);
    return MLPG_HIP_EINVAL;
  }
  if (ld_x < D || ld_out < D) {
    set_error("%s: row strides must be at least D = %d (got ld_x = %lld, ld_out = %lld)", who, D, (long long)ld_x, (long long)ld_out);
    return MLPG_HIP_EINVAL;
  }
  if ((A == nullptr) != (C == nullptr)) {
    set_error("%s: the tables A and C go together (both or neither)", who);
    return MLPG_HIP_EINVAL;
  }
  if (limit_bin < 0 || limit_bin > n / 2 + 1) {
    set_error("%s: limit_bin must be in [0, n/2 + 1] = [0, %d] (got %d)", who, n / 2 + 1, limit_bin);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || D == 0) return 0;
  if ((double)B * (double)((D + 1) / 2) > 2147483647.0) {
    set_error("%s: B * ceil(D / 2) = %d * %d workgroups are more than one launch takes", who, B, (D + 1) / 2);
    return MLPG_HIP_EINVAL;
  }
  if (Tmax == 0) return 0;  // no row to write
  if (!x || !out) {
    set_error("%s: NULL data pointer (x and out are required)", who);
    return MLPG_HIP_EINVAL;
  }
  if (out == x && ld_x != ld_out) {
    set_error("%s: in place (out == x) needs equal row strides (got %lld and %lld)", who, (long long)ld_x, (long long)ld_out);
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  FilterArgs p;
  p.x = x; p.lengths = lengths; p.A = A; p.C = C; p.out = out;
  p.ld_x = (long)ld_x; p.ld_out = (long)ld_out;
  p.B = B; p.T = Tmax; p.D = D; p.n = n; p.logn = 0;
  while ((1 << p.logn) < n) ++p.logn;
  p.ortho = ortho != 0; p.limit_bin = limit_bin; p.log_domain = log_domain != 0;
  return launch_modspec_filter((hipStream_t)stream, dtype, p);
}

}  // extern "C"
