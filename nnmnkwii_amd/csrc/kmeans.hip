// K7: float64 k-means for the start of the joint mixture (mlpg_hip_kmeans_seed_step / _lloyd_step): scikit-learn's k-means++
// seeding and Lloyd iteration restated on the device.  Plain float64 vector arithmetic, no MFMA: the assignment is N K F
// multiply-adds against N F doubles read, so both steps are bound by reading X once.  Rows are cut into slices of whole 64-row
// tiles (their number depends on N alone); a workgroup walks its slice tile by tile in row order.  No floating-point atomics:
// every sum over rows is kept per slice in row order and added over the slices in index order by a finalize kernel, so two calls
// on the same inputs give the same bits.  Compiled with -ffp-contract=off.
#include <math.h>

#include "common.h"

namespace mlpg {

namespace {

constexpr int kRows = 64;        // rows of X per tile
constexpr int kMaxF = 128, kMaxK = 64, kMaxC = 8, kMaxSlices = 1024;

struct KmeansStats {
  double shift, inertia;
  long long changed, empty;
};

// rows row0 .. row0 + 63 of X - shift into xs[kRows][ldx], zeros from row ne on
__device__ inline void load_tile(const double *__restrict__ X, const double *__restrict__ shift, long row0, long ne, int F, int ldx,
                                 double *xs, int tid) {
  for (int i = tid; i < kRows * F; i += 256) {
    const int r = i / F, f = i - r * F;
    const long n = row0 + r;
    xs[r * ldx + f] = n < ne ? X[(size_t)n * F + f] - (shift ? shift[f] : 0.0) : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Seed step.  d[j][n] = min(closest_in[n], sum_f (x_n - x_cand[j])^2) for C <= 8 candidate rows, and per slice the sums of d[j]
// over its rows.  The candidate rows (shifted like every row) go to LDS once per workgroup; a tile of X is read once for all
// candidates: thread (r = tid & 63, w = tid >> 6) takes row r against the candidates w, w + 4.  Thread j < C adds the tile's 64
// values of candidate j in row order.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_seed_kernel(const double *__restrict__ X, const double *__restrict__ shift,
                                                          const int32_t *__restrict__ cand, const double *__restrict__ closest_in,
                                                          long N, int F, int C, long rows_per_slice, double *__restrict__ d,
                                                          double *__restrict__ partial) {
  extern __shared__ double lds[];
  const int ldx = F | 1;
  double *xs = lds;                  // [kRows][ldx]
  double *cs = xs + kRows * ldx;     // [C][F]
  double *dd = cs + C * F;           // [C][kRows]
  const int tid = threadIdx.x;
  for (int i = tid; i < C * F; i += 256) {
    const int j = i / F, f = i - j * F;
    long n = cand[j];
    n = n < 0 ? 0 : (n >= N ? N - 1 : n);      // an index outside the rows reads no memory outside them
    cs[i] = X[(size_t)n * F + f] - (shift ? shift[f] : 0.0);
  }
  const long nb = (long)blockIdx.x * rows_per_slice;
  long ne = nb + rows_per_slice;
  if (ne > N) ne = N;
  double pot = 0.0;
  for (long row0 = nb; row0 < ne; row0 += kRows) {
    __syncthreads();
    load_tile(X, shift, row0, ne, F, ldx, xs, tid);
    __syncthreads();
    const int r = tid & 63;
    const long n = row0 + r;
    for (int j = tid >> 6; j < C; j += 4) {
      double s = 0.0;
      for (int f = 0; f < F; ++f) {
        const double t = xs[r * ldx + f] - cs[j * F + f];
        s += t * t;
      }
      if (n < ne) {
        if (closest_in) {
          const double c = closest_in[n];
          s = c < s ? c : s;
        }
        d[(size_t)j * N + n] = s;
      } else {
        s = 0.0;
      }
      dd[j * kRows + r] = s;
    }
    __syncthreads();
    if (tid < C)
      for (int q = 0; q < kRows; ++q) pot += dd[tid * kRows + q];
  }
  if (tid < C) partial[(size_t)blockIdx.x * kMaxC + tid] = pot;
}

// pots[j] = the slices' sums in index order
__global__ __launch_bounds__(64) void kmeans_pots_finalize(const double *__restrict__ partial, int S, int C, double *__restrict__ pots) {
  const int j = threadIdx.x;
  if (j >= C) return;
  double a = 0.0;
  for (int s = 0; s < S; ++s) a += partial[(size_t)s * kMaxC + j];
  pots[j] = a;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Lloyd step.  A tile of rows sits in LDS; thread (r = tid & 63, w = tid >> 6) takes row r against the centres w, w + 4, ...:
// v = |c_k|^2 - 2 x.c_k, the smallest kept (the first of equals).  Thread r < 64 merges the four candidates of row r (equal
// values: the smaller k), writes the label, compares it with the previous one and takes |x - c_label|^2 in the direct form.
// Then the rows are added to the slice's per-cluster sums in LDS: thread (f = tid % (F + 1), g = tid / (F + 1)) owns column f of
// the clusters k with k % G == g (G = 256 / (F + 1)) and walks the tile's rows in order -- column F counts the rows -- so every
// accumulator is added to by one thread, in row order.  The centres are read through the cache (K F doubles, 64 KB at most): with
// the accumulators they would not fit next to the tile in a CU's 160 KB at F = 128, K = 64.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_lloyd_kernel(const double *__restrict__ X, const double *__restrict__ shift,
                                                           const double *__restrict__ centers, const int32_t *labels_prev, long N,
                                                           int F, int K, long rows_per_slice, int32_t *labels,
                                                           double *__restrict__ min_dist, double *__restrict__ spart,
                                                           double *__restrict__ ipart, long long *__restrict__ cpart) {
  extern __shared__ double lds[];
  const int ldx = F | 1, F1 = F + 1;
  double *xs = lds;                        // [kRows][ldx]
  double *acc = xs + kRows * ldx;          // [K][F1]   sums; column F: the number of rows
  double *cn = acc + K * F1;               // [K]       |c_k|^2
  double *bv = cn + K;                     // [4][kRows]
  double *md = bv + 4 * kRows;             // [kRows]
  int *bk = (int *)(md + kRows);           // [4][kRows]
  int *lab = bk + 4 * kRows;               // [kRows]
  int *chg = lab + kRows;                  // [kRows]
  const int tid = threadIdx.x;
  for (int i = tid; i < K * F1; i += 256) acc[i] = 0.0;
  if (tid < K) {
    double s = 0.0;
    for (int f = 0; f < F; ++f) {
      const double c = centers[(size_t)tid * F + f];
      s += c * c;
    }
    cn[tid] = s;
  }
  const int G = 256 / F1, af = tid % F1, ag = tid / F1;
  const long nb = (long)blockIdx.x * rows_per_slice;
  long ne = nb + rows_per_slice;
  if (ne > N) ne = N;
  double inertia = 0.0;
  long long changed = 0;
  for (long row0 = nb; row0 < ne; row0 += kRows) {
    __syncthreads();
    load_tile(X, shift, row0, ne, F, ldx, xs, tid);
    __syncthreads();
    const int r = tid & 63, w = tid >> 6;
    {
      double best = INFINITY;
      int best_k = K;
      for (int k = w; k < K; k += 4) {
        const double *c = centers + (size_t)k * F;
        double dot = 0.0;
        for (int f = 0; f < F; ++f) dot += xs[r * ldx + f] * c[f];
        const double v = cn[k] - 2.0 * dot;
        if (v < best) {
          best = v;
          best_k = k;
        }
      }
      bv[w * kRows + r] = best;
      bk[w * kRows + r] = best_k;
    }
    __syncthreads();
    if (tid < kRows) {
      const long n = row0 + r;
      if (n < ne) {
        double vb = INFINITY;
        int kb = K;
        for (int g = 0; g < 4; ++g) {
          const double v = bv[g * kRows + r];
          const int k = bk[g * kRows + r];
          if (k < K && (kb == K || v < vb || (v == vb && k < kb))) {
            vb = v;
            kb = k;
          }
        }
        if (kb == K) kb = 0;                  // a row of NaNs: no value compared smaller
        const double *c = centers + (size_t)kb * F;
        double s = 0.0;
        for (int f = 0; f < F; ++f) {
          const double t = xs[r * ldx + f] - c[f];
          s += t * t;
        }
        chg[r] = labels_prev[n] != kb;
        labels[n] = kb;
        if (min_dist) min_dist[n] = s;
        md[r] = s;
        lab[r] = kb;
      } else {
        chg[r] = 0;
        md[r] = 0.0;
        lab[r] = -1;
      }
    }
    __syncthreads();
    if (tid == 0)
      for (int q = 0; q < kRows; ++q) {
        inertia += md[q];
        changed += chg[q];
      }
    if (ag < G)
      for (int q = 0; q < kRows; ++q) {
        const int k = lab[q];
        if (k >= 0 && k % G == ag) acc[k * F1 + af] += af < F ? xs[q * ldx + af] : 1.0;
      }
  }
  __syncthreads();
  double *dst = spart + (size_t)blockIdx.x * K * F1;
  for (int i = tid; i < K * F1; i += 256) dst[i] = acc[i];
  if (tid == 0) {
    ipart[blockIdx.x] = inertia;
    cpart[blockIdx.x] = changed;
  }
}

// One workgroup per cluster: sums and count over the slices in index order; the averaged centre where the count is positive (the
// old centre otherwise) and its squared shift, added in column order.
__global__ __launch_bounds__(256) void kmeans_lloyd_finalize(const double *__restrict__ spart, int S, int F, int K,
                                                             const double *__restrict__ centers, int update, double *__restrict__ sums,
                                                             double *__restrict__ counts, double *centers_out,
                                                             double *__restrict__ shift_k) {
  __shared__ double tot[kMaxF + 1];
  __shared__ double sq[kMaxF];
  const int k = blockIdx.x, f = threadIdx.x, F1 = F + 1;
  double a = 0.0;
  if (f < F1) {
    for (int s = 0; s < S; ++s) a += spart[((size_t)s * K + k) * F1 + f];
    tot[f] = a;
  }
  __syncthreads();
  if (f < F) {
    const double cnt = tot[F], old = centers[(size_t)k * F + f];
    const double nw = cnt > 0.0 ? a / cnt : old;
    sums[(size_t)k * F + f] = a;
    if (update) centers_out[(size_t)k * F + f] = nw;
    sq[f] = (nw - old) * (nw - old);
  }
  __syncthreads();
  if (f == 0) {
    counts[k] = tot[F];
    double s = 0.0;
    for (int q = 0; q < F; ++q) s += sq[q];
    shift_k[k] = update ? s : 0.0;
  }
}

// the statistics record: the shift added in k order, the inertia and the changed labels over the slices in index order
__global__ __launch_bounds__(64) void kmeans_stats_kernel(const double *__restrict__ ipart, const long long *__restrict__ cpart, int S,
                                                          const double *__restrict__ counts, const double *__restrict__ shift_k, int K,
                                                          KmeansStats *__restrict__ stats) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += shift_k[k];
    stats->shift = s;
  } else if (tid == 1) {
    double s = 0.0;
    for (int i = 0; i < S; ++i) s += ipart[i];
    stats->inertia = s;
  } else if (tid == 2) {
    long long c = 0;
    for (int i = 0; i < S; ++i) c += cpart[i];
    stats->changed = c;
  } else if (tid == 3) {
    long long e = 0;
    for (int k = 0; k < K; ++k) e += counts[k] == 0.0;
    stats->empty = e;
  }
}

size_t round256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

// The slice rule: one slice per 64-row tile up to 1024 slices, then whole tiles per slice; a function of N alone.
int kmeans_slices(long N) {
  long s = (N + kRows - 1) / kRows;
  if (s > kMaxSlices) s = kMaxSlices;
  return s < 1 ? 1 : (int)s;
}

static long kmeans_rows_per_slice(long N, int S) {
  const long tiles = (N + kRows - 1) / kRows;
  return (tiles + S - 1) / S * kRows;
}

// workspace layout: [seed partials: S 8] [Lloyd partial sums: S K (F + 1)] [partial inertia: S] [partial changed (int64): S]
// [squared shift per cluster: K], each region rounded up to 256 bytes
struct KmeansLayout {
  size_t p_off, s_off, i_off, c_off, k_off, total;
};
static KmeansLayout kmeans_layout(long N, int F, int K) {
  const size_t S = (size_t)kmeans_slices(N);
  KmeansLayout l;
  l.p_off = 0;
  l.s_off = l.p_off + round256(sizeof(double) * S * kMaxC);
  l.i_off = l.s_off + round256(sizeof(double) * S * K * (F + 1));
  l.c_off = l.i_off + round256(sizeof(double) * S);
  l.k_off = l.c_off + round256(sizeof(long long) * S);
  l.total = l.k_off + round256(sizeof(double) * K);
  return l;
}

size_t kmeans_workspace_bytes(long N, int F, int K) { return kmeans_layout(N, F, K).total; }
size_t kmeans_seed_workspace_bytes(long N) { return round256(sizeof(double) * (size_t)kmeans_slices(N) * kMaxC); }

int launch_kmeans_seed(hipStream_t st, const double *X, const double *shift, const int32_t *cand, const double *closest_in, long N,
                       int F, int C, double *d, double *pots, void *workspace) {
  const size_t lds = sizeof(double) * ((size_t)kRows * (F | 1) + (size_t)C * F + (size_t)C * kRows);
  // the largest shape (F = 128, C = 8) takes 76 KB: above the 64 KB a kernel gets unasked
  const size_t lds_max = sizeof(double) * ((size_t)kRows * (kMaxF | 1) + (size_t)kMaxC * kMaxF + (size_t)kMaxC * kRows);
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)kmeans_seed_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
  const int S = kmeans_slices(N);
  double *partial = (double *)workspace;
  hipLaunchKernelGGL(kmeans_seed_kernel, dim3((unsigned)S), dim3(256), lds, st, X, shift, cand, closest_in, N, F, C,
                     kmeans_rows_per_slice(N, S), d, partial);
  MLPG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(kmeans_pots_finalize, dim3(1), dim3(64), 0, st, (const double *)partial, S, C, pots);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountKmeansSeed);
  return 0;
}

static size_t lloyd_lds_bytes(int F, int K) {
  return sizeof(double) * ((size_t)kRows * (F | 1) + (size_t)K * (F + 1) + K + 5 * kRows) + sizeof(int) * 6 * kRows;
}

int launch_kmeans_lloyd(hipStream_t st, const double *X, const double *shift, const double *centers, const int32_t *labels_prev,
                        long N, int F, int K, int update, int32_t *labels, double *min_dist, double *sums, double *counts,
                        double *centers_out, void *stats, void *workspace) {
  const KmeansLayout l = kmeans_layout(N, F, K);
  const int S = kmeans_slices(N);
  double *spart = (double *)((char *)workspace + l.s_off);
  double *ipart = (double *)((char *)workspace + l.i_off);
  long long *cpart = (long long *)((char *)workspace + l.c_off);
  double *shift_k = (double *)((char *)workspace + l.k_off);
  // the largest shape (F = 128, K = 64) takes 134 KB of a CU's 160 KB
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)kmeans_lloyd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lloyd_lds_bytes(kMaxF, kMaxK)));
  hipLaunchKernelGGL(kmeans_lloyd_kernel, dim3((unsigned)S), dim3(256), lloyd_lds_bytes(F, K), st, X, shift, centers, labels_prev, N, F,
                     K, kmeans_rows_per_slice(N, S), labels, min_dist, spart, ipart, cpart);
  MLPG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(kmeans_lloyd_finalize, dim3((unsigned)K), dim3(256), 0, st, (const double *)spart, S, F, K, centers, update, sums,
                     counts, centers_out, shift_k);
  MLPG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(kmeans_stats_kernel, dim3(1), dim3(64), 0, st, (const double *)ipart, (const long long *)cpart, S,
                     (const double *)counts, (const double *)shift_k, K, (KmeansStats *)stats);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountKmeansLloyd);
  return 0;
}

}  // namespace mlpg

using namespace mlpg;

namespace {

// what the entries share: 0 go on, 1 nothing to do (N == 0), < 0 refused.  Nothing here touches the runtime.
int check_kmeans(const char *who, int device, int64_t N, int F, int K) {
  if (F < 1 || F > kMaxF) {
    set_error("%s: the number of features must be in [1, %d] (got %d)", who, kMaxF, F);
    return MLPG_HIP_EINVAL;
  }
  if (K < 1 || K > kMaxK) {
    set_error("%s: the number of clusters must be in [1, %d] (got %d)", who, kMaxK, K);
    return MLPG_HIP_EINVAL;
  }
  if (N < 0 || (N + kRows - 1) / kRows > 2147483647LL) {
    set_error("%s: bad number of rows (%lld)", who, (long long)N);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  return N == 0 ? 1 : 0;
}

int check_kmeans_workspace(const char *who, const void *workspace, size_t bytes, size_t need) {
  if (!workspace || bytes < need || ((uintptr_t)workspace & 7)) {
    set_error("%s: workspace of %zu bytes (8-byte aligned) needed, see mlpg_hip_kmeans_workspace_bytes", who, need);
    return MLPG_HIP_EINVAL;
  }
  return 0;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) size_t mlpg_hip_kmeans_workspace_bytes(int64_t N, int F, int K) {
  if (N < 0 || F < 1 || F > kMaxF || K < 1 || K > kMaxK || (N + kRows - 1) / kRows > 2147483647LL) return 0;
  return kmeans_workspace_bytes((long)N, F, K);
}

__attribute__((visibility("default"))) int mlpg_hip_kmeans_seed_step(int device, void *stream, const double *X, const double *shift,
                                                                     int64_t N, int F, const int32_t *candidates, int C,
                                                                     const double *closest_in, double *d, double *pots,
                                                                     void *workspace, size_t workspace_bytes) {
  const char *who = "kmeans_seed_step";
  if (C < 1 || C > kMaxC) {
    set_error("%s: the number of candidates must be in [1, %d] (got %d)", who, kMaxC, C);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_kmeans(who, device, N, F, 1)) return rc < 0 ? rc : 0;
  if (!X || !candidates || !d || !pots) {
    set_error("%s: NULL data pointer (X, candidates, d and pots are required)", who);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_kmeans_workspace(who, workspace, workspace_bytes, kmeans_seed_workspace_bytes((long)N))) return rc;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_kmeans_seed((hipStream_t)stream, X, shift, candidates, closest_in, (long)N, F, C, d, pots, workspace);
}

__attribute__((visibility("default"))) int mlpg_hip_kmeans_lloyd_step(int device, void *stream, const double *X, const double *shift,
                                                                      const double *centers, const int32_t *labels_prev, int64_t N,
                                                                      int F, int K, int update_centers, int32_t *labels,
                                                                      double *min_dist, double *sums, double *counts,
                                                                      double *centers_out, void *stats, void *workspace,
                                                                      size_t workspace_bytes) {
  const char *who = "kmeans_lloyd_step";
  if (int rc = check_kmeans(who, device, N, F, K)) return rc < 0 ? rc : 0;
  if (!X || !centers || !labels_prev || !labels || !sums || !counts || !stats || (update_centers && !centers_out)) {
    set_error("%s: NULL data pointer (X, centers, labels_prev, labels, sums, counts and stats are required, centers_out with "
              "update_centers)", who);
    return MLPG_HIP_EINVAL;
  }
  if (((uintptr_t)stats & 7)) {
    set_error("%s: the statistics record must be 8-byte aligned", who);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_kmeans_workspace(who, workspace, workspace_bytes, kmeans_workspace_bytes((long)N, F, K))) return rc;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_kmeans_lloyd((hipStream_t)stream, X, shift, centers, labels_prev, (long)N, F, K, update_centers ? 1 : 0, labels,
                             min_dist, sums, counts, centers_out, stats, workspace);
}

}  // extern "C"
