// K6: float64 EM for full-covariance Gaussian mixtures (mlpg_hip_gmm_estep / _mstep / _precisions), scikit-learn's _e_step /
// _m_step restated on the device.  The two F^2-per-row-and-component contractions -- (X - mu_k) U_k in the E-step, the weighted
// outer products in the M-step -- run on v_mfma_f64_16x16x4_f64.  Lane maps of that instruction (lane l of the wave):
//   A operand: A[row l & 15][k = l >> 4]        B operand: B[k = l >> 4][col l & 15]         (one double per lane each)
//   C/D: 4 doubles per lane, register g holds D[row (l >> 4) + 4 g][col l & 15]              (NOT the f32 map (l >> 4) * 4 + g)
// No floating-point atomics: every sum over rows goes through per-workgroup (E-step mean) or per-slice (M-step) partial results
// in the caller's workspace, added by a finalize kernel in one fixed order; two calls on the same inputs give the same bits.
// Compiled with -ffp-contract=off.
#include <math.h>

#include "common.h"

namespace mlpg {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kERows = 64;      // rows of X per E-step workgroup: 4 waves x one 16-row MFMA tile
// the E-step's workgroups (256 threads) one launch takes: a grid is 32 bits of threads, a larger one runs truncated and reports nothing
constexpr long long kEMaxBlocks = 16777215LL;  // 2^24 - 1
constexpr int kMaxF = 128, kMaxK = 64;

__device__ inline v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// ---------------------------------------------------------------------------------------------------------------------------
// E-step.  One workgroup per 64 rows; the rows sit in LDS (zero-filled past N and past F), wave w owns rows 16 w .. 16 w + 15.
// Per component k and 16-column tile j of Y = (X - mu_k) U_k the wave sums over the k-steps 0 .. min(F, 16 (j + 1)) only: U_k is
// upper triangular, the tiles below its diagonal are all zero and are skipped.  Squares are added per lane over the column tiles,
// then over the 16 lanes of a row by four xor-shuffles (a fixed tree).  log p + log w goes to LDS; behind a barrier thread r
// takes row r through the log-sum-exp, and all threads write the responsibilities coalesced.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmm_estep_kernel(const double *__restrict__ X, const double *__restrict__ weights,
                                                        const double *__restrict__ means, const double *__restrict__ U,
                                                        const double *__restrict__ log_det, long N, int F, int K,
                                                        double *__restrict__ resp, double *__restrict__ lpn_out,
                                                        int32_t *__restrict__ label_out, double *__restrict__ partial) {
  extern __shared__ double lds[];
  const int F4 = (F + 3) & ~3;
  const int ldx = F4 + 1;             // odd row stride: the 16 rows of an A operand fall on different banks
  const int ldp = K | 1;
  double *xs = lds;                   // [kERows][ldx]
  double *lp = xs + kERows * ldx;     // [kERows][ldp]   log p + log w
  double *ln = lp + kERows * ldp;     // [kERows]        log_prob_norm
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * kERows;

  for (int i = tid; i < kERows * ldx; i += 256) {
    const int r = i / ldx, c = i - r * ldx;
    const long n = row0 + r;
    xs[i] = (n < N && c < F) ? X[(size_t)n * F + c] : 0.0;
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  const int r4 = lane >> 4, c16 = lane & 15;
  const double *xrow = xs + (wave * 16 + c16) * ldx;   // the A operand's row
  const int FT = (F + 15) >> 4;
  const double half_const = F * log(2.0 * M_PI);
  for (int k = 0; k < K; ++k) {
    const double *mu = means + (size_t)k * F;
    const double *Uk = U + (size_t)k * F * F;
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < FT; ++j) {
      const int col = 16 * j + c16;
      const bool col_ok = col < F;
      const int kend = min(F4, 16 * (j + 1));
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      for (int k0 = 0; k0 < kend; k0 += 4) {
        const int kk = k0 + r4;
        const bool k_ok = kk < F;
        const double a = k_ok ? xrow[kk] - mu[kk] : 0.0;
        const double b = (k_ok && col_ok) ? Uk[(size_t)kk * F + col] : 0.0;
        acc = mfma_f64(a, b, acc);
      }
      for (int g = 0; g < 4; ++g) sq[g] += acc[g] * acc[g];
    }
    const double lw = log(weights[k]), ld = log_det[k];
    for (int g = 0; g < 4; ++g) {
      double s = sq[g];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 4);
      s += __shfl_xor(s, 8);
      if (c16 == 0) lp[(wave * 16 + r4 + 4 * g) * ldp + k] = (-0.5 * (half_const + s) + ld) + lw;
    }
  }
  __syncthreads();

  if (tid < kERows) {
    const long n = row0 + tid;
    const double *p = lp + tid * ldp;
    double m = p[0];
    int best = 0;
    for (int k = 1; k < K; ++k)
      if (p[k] > m) {
        m = p[k];
        best = k;
      }
    // scipy's logsumexp: a non-finite maximum is replaced by 0 before it is subtracted
    const double mm = isfinite(m) ? m : 0.0;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp(p[k] - mm);
    const double v = log(s) + mm;
    ln[tid] = v;
    if (n < N) {
      if (lpn_out) lpn_out[n] = v;
      if (label_out) label_out[n] = best;
    }
  }
  __syncthreads();
  if (resp) {
    const long left = N - row0;
    const int rows = left < kERows ? (int)left : kERows;
    double *dst = resp + (size_t)row0 * K;
    for (int i = tid; i < rows * K; i += 256) {
      const int r = i / K, k = i - r * K;
      dst[i] = exp(lp[r * ldp + k] - ln[r]);
    }
  }
  if (partial && tid == 0) {
    const long left = N - row0;
    const int rows = left < kERows ? (int)left : kERows;
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += ln[r];
    partial[blockIdx.x] = s;
  }
}

// mean = (sum of the workgroups' partial sums) / N in one fixed order (as modspec_loss_finalize)
__global__ __launch_bounds__(256) void gmm_mean_finalize(const double *partial, long count, double inv_n, double *out) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (long i = tid; i < count; i += 256) acc += partial[i];
  s[tid] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) s[tid] += s[tid + h];
    __syncthreads();
  }
  if (tid == 0) *out = s[0] * inv_n;
}

// ---------------------------------------------------------------------------------------------------------------------------
// M-step, pass 1: per slice s, component k and column f the sums  sum_n r_nk x_nf  (f < F)  and  sum_n r_nk  (f == F).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmm_sums_kernel(const double *__restrict__ X, const double *__restrict__ resp, long N, int F,
                                                       int K, long rows_per_slice, double *__restrict__ mpart) {
  const int t = blockIdx.y * 256 + threadIdx.x;
  if (t >= K * (F + 1)) return;
  const int k = t / (F + 1), f = t - k * (F + 1);
  const long nb = (long)blockIdx.x * rows_per_slice;
  long ne = nb + rows_per_slice;
  if (ne > N) ne = N;
  double acc = 0.0;
  if (f < F)
    for (long n = nb; n < ne; ++n) acc += resp[(size_t)n * K + k] * X[(size_t)n * F + f];
  else
    for (long n = nb; n < ne; ++n) acc += resp[(size_t)n * K + k];
  mpart[((size_t)blockIdx.x * K + k) * (F + 1) + f] = acc;
}

// nk = sum over slices + 10 eps; means = sums / nk; weights = nk / sum_k nk.  One workgroup per component; workgroup 0 also
// writes the weights.  Slices are added in index order.
__global__ __launch_bounds__(128) void gmm_means_finalize(const double *__restrict__ mpart, int S, int F, int K,
                                                          double *__restrict__ nk_out, double *__restrict__ means,
                                                          double *__restrict__ weights) {
  __shared__ double snk[kMaxK];
  const int k = blockIdx.x, tid = threadIdx.x;
  const double tiny = 10.0 * 2.220446049250313e-16;
  double nk = 0.0;
  for (int s = 0; s < S; ++s) nk += mpart[((size_t)s * K + k) * (F + 1) + F];
  nk += tiny;
  if (tid < F) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += mpart[((size_t)s * K + k) * (F + 1) + tid];
    means[(size_t)k * F + tid] = acc / nk;
  }
  if (tid == 0) nk_out[k] = nk;
  if (k == 0) {
    if (tid < K) {
      double a = 0.0;
      for (int s = 0; s < S; ++s) a += mpart[((size_t)s * K + tid) * (F + 1) + F];
      snk[tid] = a + tiny;
    }
    __syncthreads();
    if (tid < K) {
      double tot = 0.0;
      for (int q = 0; q < K; ++q) tot += snk[q];
      weights[tid] = snk[tid] / tot;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// M-step, pass 2: the weighted outer products.  Workgroup (slice s, component k, tile row ti); its 4 waves take the slice's rows
// four at a time (wave w: rows 4 w + 16 i), A = r_nk (x_n - mu_k) on the 16 columns of tile row ti, B = x_n - mu_k on the columns
// of tile tj, one accumulator tile per tj >= ti (the tiles below the diagonal are skipped).  The waves' tiles are added in wave
// order through LDS and written to partial[s][k][i][j].
// ---------------------------------------------------------------------------------------------------------------------------
template <int FT>
__global__ __launch_bounds__(256) void gmm_cov_kernel(const double *__restrict__ X, const double *__restrict__ resp,
                                                      const double *__restrict__ means, long N, int F, int K, long rows_per_slice,
                                                      double *__restrict__ cpart) {
  __shared__ double red[3 * FT * 4 * 64];
  const int s = blockIdx.x, k = blockIdx.y, ti = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r4 = lane >> 4, c16 = lane & 15;
  const long nb = (long)s * rows_per_slice;
  long ne = nb + rows_per_slice;
  if (ne > N) ne = N;
  const int ci = 16 * ti + c16;
  const bool ci_ok = ci < F;
  const double mu_i = ci_ok ? means[(size_t)k * F + ci] : 0.0;
  double mu_j[FT];
  v4d acc[FT];
#pragma unroll
  for (int tj = 0; tj < FT; ++tj) {
    const int cj = 16 * tj + c16;
    mu_j[tj] = cj < F ? means[(size_t)k * F + cj] : 0.0;
    acc[tj] = v4d{0.0, 0.0, 0.0, 0.0};
  }
  for (long n0 = nb + 4 * wave; n0 < ne; n0 += 16) {
    const long n = n0 + r4;
    const bool ok = n < ne;
    const double *xr = X + (size_t)(ok ? n : nb) * F;
    const double r = ok ? resp[(size_t)n * K + k] : 0.0;
    const double a = (ok && ci_ok) ? r * (xr[ci] - mu_i) : 0.0;
#pragma unroll
    for (int tj = 0; tj < FT; ++tj) {
      if (tj >= ti) {
        const int cj = 16 * tj + c16;
        const double b = (ok && cj < F) ? xr[cj] - mu_j[tj] : 0.0;
        acc[tj] = mfma_f64(a, b, acc[tj]);
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int tj = 0; tj < FT; ++tj)
#pragma unroll
      for (int g = 0; g < 4; ++g) red[(((wave - 1) * FT + tj) * 4 + g) * 64 + lane] = acc[tj][g];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int tj = 0; tj < FT; ++tj) {
      if (tj >= ti) {
        const int j = 16 * tj + c16;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          double v = acc[tj][g];
          for (int w = 0; w < 3; ++w) v += red[((w * FT + tj) * 4 + g) * 64 + lane];
          const int i = 16 * ti + r4 + 4 * g;
          if (i < F && j < F) cpart[(((size_t)s * K + k) * F + i) * F + j] = v;
        }
      }
    }
  }
}

// covariances[k][i][j] = sum over slices / nk + reg_covar (i == j), for j >= i, mirrored to [j][i]
__global__ __launch_bounds__(256) void gmm_cov_finalize(const double *__restrict__ cpart, const double *__restrict__ nk, int S, int F,
                                                        int K, double reg_covar, double *__restrict__ cov) {
  const int k = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= F * F) return;
  const int i = e / F, j = e - i * F;
  if (j < i) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += cpart[(((size_t)s * K + k) * F + i) * F + j];
  double v = acc / nk[k];
  if (i == j) v += reg_covar;
  cov[((size_t)k * F + i) * F + j] = v;
  cov[((size_t)k * F + j) * F + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Precisions.  One workgroup per component, the covariance in LDS (row stride F | 1).  Column Cholesky (lower L, in place), a
// pivot that is <= 0 or NaN sets the status word to its 1-based index and ends the component (LAPACK dpotrf's rule).  Then L is
// inverted in place from the last column to the first (LAPACK dtrti2's order), U = L^-T is written with exact zeros below the
// diagonal, and log_det = sum_i log U_ii in index order.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmm_precisions_kernel(const double *__restrict__ cov, int F, double *__restrict__ U,
                                                             double *__restrict__ log_det, int32_t *__restrict__ status) {
  extern __shared__ double lds[];
  const int ld = F | 1;
  double *a = lds;  // [F][ld]
  const int k = blockIdx.x, tid = threadIdx.x;
  const double *c = cov + (size_t)k * F * F;
  for (int e = tid; e < F * F; e += 256) {
    const int i = e / F, j = e - i * F;
    a[i * ld + j] = c[e];
  }
  __syncthreads();
  for (int j = 0; j < F; ++j) {
    const int i = tid;
    double sv = 0.0;
    if (i >= j && i < F) {
      sv = a[i * ld + j];
      for (int m = 0; m < j; ++m) sv -= a[i * ld + m] * a[j * ld + m];
      a[i * ld + j] = sv;
    }
    __syncthreads();
    const double d = a[j * ld + j];
    if (!(d > 0.0)) {   // the same for every thread of the workgroup
      if (tid == 0) status[k] = j + 1;
      return;
    }
    const double piv = sqrt(d);
    __syncthreads();
    if (i == j) a[i * ld + j] = piv;
    if (i > j && i < F) a[i * ld + j] = sv / piv;
    __syncthreads();
  }
  // in-place inverse of the lower factor, last column first
  for (int j = F - 1; j >= 0; --j) {
    const int i = tid;
    const double inv = 1.0 / a[j * ld + j];
    double v = 0.0;
    if (i > j && i < F) {
      for (int m = j + 1; m <= i; ++m) v += a[i * ld + m] * a[m * ld + j];
      v = -(v * inv);
    }
    __syncthreads();
    if (i == j) a[i * ld + j] = inv;
    if (i > j && i < F) a[i * ld + j] = v;
    __syncthreads();
  }
  double *u = U + (size_t)k * F * F;
  for (int e = tid; e < F * F; e += 256) {
    const int r = e / F, q = e - r * F;
    u[e] = q >= r ? a[q * ld + r] : 0.0;   // U[r][q] = Linv[q][r]
  }
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < F; ++i) s += log(a[i * ld + i]);
    log_det[k] = s;
    status[k] = 0;
  }
}

size_t round256(size_t b) { return (b + 255) / 256 * 256; }

template <int FT>
void launch_cov(hipStream_t st, int S, int K, int ti_count, const double *X, const double *resp, const double *means, long N, int F,
                long rps, double *cpart) {
  hipLaunchKernelGGL(gmm_cov_kernel<FT>, dim3((unsigned)S, (unsigned)K, (unsigned)ti_count), dim3(256), 0, st, X, resp, means, N, F, K,
                     rps, cpart);
}

}  // namespace

// The slice rule: the number of row slices of the M-step depends on (N, F, K) alone -- about 256 rows per slice at least, and no
// more slices than give 2048 workgroups of the outer-product kernel (which bounds the workspace: S K F^2 doubles).
int gmm_slices(long N, int F, int K) {
  const int FT = (F + 15) / 16;
  long cap = 2048 / ((long)K * FT);
  if (cap < 1) cap = 1;
  long s = (N + 255) / 256;
  if (s > cap) s = cap;
  return s < 1 ? 1 : (int)s;
}

// Pass 1 of the M-step is cheap per row and its partial results are small: it takes its own, finer cut (64 rows per slice at
// least, 1024 slices at most).
int gmm_sum_slices(long N) {
  long s = (N + 63) / 64;
  if (s > 1024) s = 1024;
  return s < 1 ? 1 : (int)s;
}

// workspace layout: [E-step partial sums: ceil(N / 64)] [pass-1 partials: S1 K (F + 1)] [nk: K] [pass-2 partials: S K F F], each
// region rounded up to 256 bytes
struct GmmLayout {
  size_t e_off, m_off, nk_off, c_off, total;
};
static GmmLayout gmm_layout(long N, int F, int K) {
  const size_t S = (size_t)gmm_slices(N, F, K), S1 = (size_t)gmm_sum_slices(N);
  GmmLayout l;
  l.e_off = 0;
  l.m_off = l.e_off + round256(sizeof(double) * (size_t)((N + kERows - 1) / kERows));
  l.nk_off = l.m_off + round256(sizeof(double) * S1 * K * (F + 1));
  l.c_off = l.nk_off + round256(sizeof(double) * K);
  l.total = l.c_off + round256(sizeof(double) * S * K * F * F);
  return l;
}

size_t gmm_workspace_bytes(long N, int F, int K) { return gmm_layout(N, F, K).total; }

int launch_gmm_estep(hipStream_t st, const double *X, const double *weights, const double *means, const double *U,
                     const double *log_det, long N, int F, int K, double *resp, double *log_prob_norm, int32_t *labels,
                     double *mean_out, void *workspace) {
  const int F4 = (F + 3) & ~3;
  const size_t lds = sizeof(double) * ((size_t)kERows * (F4 + 1) + (size_t)kERows * (K | 1) + kERows);
  // the largest shape (F = 128, K = 64) takes 99.5 KB: above the 64 KB a kernel gets unasked
  const size_t lds_max = sizeof(double) * ((size_t)kERows * (kMaxF + 1) + (size_t)kERows * (kMaxK | 1) + kERows);
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)gmm_estep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
  const long blocks = (N + kERows - 1) / kERows;
  double *partial = mean_out ? (double *)((char *)workspace + gmm_layout(N, F, K).e_off) : nullptr;
  hipLaunchKernelGGL(gmm_estep_kernel, dim3((unsigned)blocks), dim3(256), lds, st, X, weights, means, U, log_det, N, F, K, resp,
                     log_prob_norm, labels, partial);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountGmmEstep);
  if (mean_out) {
    hipLaunchKernelGGL(gmm_mean_finalize, dim3(1), dim3(256), 0, st, (const double *)partial, blocks, 1.0 / (double)N, mean_out);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

int launch_gmm_mstep(hipStream_t st, const double *X, const double *resp, long N, int F, int K, double reg_covar, double *weights,
                     double *means, double *cov, void *workspace) {
  const GmmLayout l = gmm_layout(N, F, K);
  const int S = gmm_slices(N, F, K), S1 = gmm_sum_slices(N);
  const long rps = (N + S - 1) / S, rps1 = (N + S1 - 1) / S1;
  double *mpart = (double *)((char *)workspace + l.m_off);
  double *nk = (double *)((char *)workspace + l.nk_off);
  double *cpart = (double *)((char *)workspace + l.c_off);
  const int FT = (F + 15) / 16;
  hipLaunchKernelGGL(gmm_sums_kernel, dim3((unsigned)S1, (unsigned)((K * (F + 1) + 255) / 256)), dim3(256), 0, st, X, resp, N, F, K, rps1,
                     mpart);
  MLPG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(gmm_means_finalize, dim3((unsigned)K), dim3(128), 0, st, (const double *)mpart, S1, F, K, nk, means, weights);
  MLPG_HIP_CHECK(hipGetLastError());
  switch (FT) {
    case 1: launch_cov<1>(st, S, K, FT, X, resp, means, N, F, rps, cpart); break;
    case 2: launch_cov<2>(st, S, K, FT, X, resp, means, N, F, rps, cpart); break;
    case 3: launch_cov<3>(st, S, K, FT, X, resp, means, N, F, rps, cpart); break;
    case 4: launch_cov<4>(st, S, K, FT, X, resp, means, N, F, rps, cpart); break;
    case 5: launch_cov<5>(st, S, K, FT, X, resp, means, N, F, rps, cpart); break;
    case 6: launch_cov<6>(st, S, K, FT, X, resp, means, N, F, rps, cpart); break;
    case 7: launch_cov<7>(st, S, K, FT, X, resp, means, N, F, rps, cpart); break;
    default: launch_cov<8>(st, S, K, FT, X, resp, means, N, F, rps, cpart); break;
  }
  MLPG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(gmm_cov_finalize, dim3((unsigned)((F * F + 255) / 256), (unsigned)K), dim3(256), 0, st, (const double *)cpart,
                     (const double *)nk, S, F, K, reg_covar, cov);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountGmmMstep);
  return 0;
}

int launch_gmm_precisions(hipStream_t st, const double *cov, int F, int K, double *U, double *log_det, int32_t *status) {
  const size_t lds = sizeof(double) * (size_t)F * (F | 1);
  const size_t lds_max = sizeof(double) * (size_t)kMaxF * (kMaxF | 1);   // 129 KB of a CU's 160 KB
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)gmm_precisions_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
  hipLaunchKernelGGL(gmm_precisions_kernel, dim3((unsigned)K), dim3(256), lds, st, cov, F, U, log_det, status);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountGmmPrecisions);
  return 0;
}

}  // namespace mlpg

using namespace mlpg;

namespace {

// what the entries share: 0 go on, 1 nothing to do (N == 0), < 0 refused.  Nothing here touches the runtime.
int check_gmm(const char *who, int device, int64_t N, int F, int K) {
  if (F < 1 || F > kMaxF) {
    set_error("%s: the number of features must be in [1, %d] (got %d)", who, kMaxF, F);
    return MLPG_HIP_EINVAL;
  }
  if (K < 1 || K > kMaxK) {
    set_error("%s: the number of components must be in [1, %d] (got %d)", who, kMaxK, K);
    return MLPG_HIP_EINVAL;
  }
  if (N < 0) {
    set_error("%s: bad number of rows (%lld)", who, (long long)N);
    return MLPG_HIP_EINVAL;
  }
  if ((N + kERows - 1) / kERows > kEMaxBlocks) {
    set_error("%s: %lld rows are more than the %lld workgroups of 256 threads (%d rows each) one launch of the E-step takes: a grid is "
              "32 bits of threads", who, (long long)N, kEMaxBlocks, kERows);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  return N == 0 ? 1 : 0;
}

int check_workspace(const char *who, const void *workspace, size_t bytes, int64_t N, int F, int K) {
  const size_t need = gmm_workspace_bytes((long)N, F, K);
  if (!workspace || bytes < need || ((uintptr_t)workspace & 7)) {
    set_error("%s: workspace of %zu bytes (8-byte aligned) needed, see mlpg_hip_gmm_workspace_bytes", who, need);
    return MLPG_HIP_EINVAL;
  }
  return 0;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) size_t mlpg_hip_gmm_workspace_bytes(int64_t N, int F, int K) {
  if (N < 0 || F < 1 || F > kMaxF || K < 1 || K > kMaxK || (N + kERows - 1) / kERows > kEMaxBlocks) return 0;
  return gmm_workspace_bytes((long)N, F, K);
}

__attribute__((visibility("default"))) int mlpg_hip_gmm_estep(int device, void *stream, const double *X, const double *weights,
                                                              const double *means, const double *prec_chol, const double *log_det,
                                                              int64_t N, int F, int K, double *resp, double *log_prob_norm,
                                                              int32_t *labels, double *mean_log_prob, void *workspace,
                                                              size_t workspace_bytes) {
  const char *who = "gmm_estep";
  if (int rc = check_gmm(who, device, N, F, K)) return rc < 0 ? rc : 0;
  if (!X || !weights || !means || !prec_chol || !log_det) {
    set_error("%s: NULL data pointer (X, weights, means, prec_chol and log_det are required)", who);
    return MLPG_HIP_EINVAL;
  }
  if (mean_log_prob)
    if (int rc = check_workspace(who, workspace, workspace_bytes, N, F, K)) return rc;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_gmm_estep((hipStream_t)stream, X, weights, means, prec_chol, log_det, (long)N, F, K, resp, log_prob_norm, labels,
                          mean_log_prob, workspace);
}

__attribute__((visibility("default"))) int mlpg_hip_gmm_mstep(int device, void *stream, const double *X, const double *resp, int64_t N,
                                                              int F, int K, double reg_covar, double *weights, double *means,
                                                              double *covariances, void *workspace, size_t workspace_bytes) {
  const char *who = "gmm_mstep";
  if (int rc = check_gmm(who, device, N, F, K)) return rc < 0 ? rc : 0;
  if (!(reg_covar >= 0.0) || !isfinite(reg_covar)) {
    set_error("%s: reg_covar must be finite and not negative (got %g)", who, reg_covar);
    return MLPG_HIP_EINVAL;
  }
  if (!X || !resp || !weights || !means || !covariances) {
    set_error("%s: NULL data pointer (X, resp, weights, means and covariances are required)", who);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_workspace(who, workspace, workspace_bytes, N, F, K)) return rc;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_gmm_mstep((hipStream_t)stream, X, resp, (long)N, F, K, reg_covar, weights, means, covariances, workspace);
}

__attribute__((visibility("default"))) int mlpg_hip_gmm_precisions(int device, void *stream, const double *covariances, int F, int K,
                                                                   double *prec_chol, double *log_det, int32_t *status) {
  const char *who = "gmm_precisions";
  if (int rc = check_gmm(who, device, 1, F, K)) return rc < 0 ? rc : 0;
  if (!covariances || !prec_chol || !log_det || !status) {
    set_error("%s: NULL data pointer (covariances, prec_chol, log_det and status are required)", who);
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_gmm_precisions((hipStream_t)stream, covariances, F, K, prec_chol, log_det, status);
}

}  // extern "C"
