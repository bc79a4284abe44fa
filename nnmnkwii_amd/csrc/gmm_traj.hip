// K10: the statistics of trajectory GMM conversion over a padded batch (mlpg_hip_gmm_trajectory_stats; the reference's
// baseline/gmm.py:225-247): with the hard mixture label m of a live frame, mean = mu_y[m] + A[m] (x - mu_x[m]) and var = cvar[m],
// both in the padded layout mlpg_hip_forward reads.  Per frame that is one D x D matrix-vector product, 2 D^2 flops for 24 D bytes,
// so it runs on v_mfma_f64_16x16x4_f64 (lane maps: top of gmm_em.hip): frames are the rows, output dims the columns, K = D padded
// to a multiple of 4 with zero operands.
//
// One workgroup (4 waves) per MLPG_HIP_GMM_TRAJ_ROW_TILE = 64 rows of the flattened (B * Tmax) axis.  Thread r < 64 settles row r:
// its label, kBad for a live row whose label is outside [0, M), kPad for a row at or past its utterance's length (neither x nor the
// label of such a row is read).  x - mu_x[label] is staged in LDS (zeros for the other rows and for columns past D).  Wave w owns
// the 16-row MFMA block w of the tile and every 16-column tile of the output.  It walks the DISTINCT labels of its block, found by
// ballot over the 16 rows, in order of first appearance: per label and column tile it multiplies the block into the 4 x 16 operands
// of A[m], and a lane keeps a result only where the row's label is m.  The waves' work is equal whenever their blocks hold equally
// many labels, whatever D is; in speech a block holds one or two.  A row's sum over k runs in one fixed order whatever else is in
// its tile: the same bits for every tiling, batch shape and call.  No atomics.  The means go back into the rows' LDS image and leave
// as whole rows together with the variances (cvar[label] copied; 0 and 1 for padding rows; NaN for rows with a bad label).  Columns
// past D are never touched.  Worst case: 16 distinct labels in every block -- 16 times the flops of a tile with one label.  A[m]'s
// operands are read once per label, column tile and BLOCK (not per tile: up to four times the L2 reads when a tile holds one
// label); a split by column tiles with the operands shared by the four blocks was tried first and left the waves unequal (5 column
// tiles at D = 72) with a branch per block in the inner loop.
// Compiled with -ffp-contract=off.
#include <math.h>

#include "common.h"

namespace mlpg {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kTrajRows = MLPG_HIP_GMM_TRAJ_ROW_TILE;
constexpr int kTrajMaxD = 128, kTrajMaxM = 65536;
constexpr int kPad = -2, kBad = -1;
constexpr int kBatch = 8;            // k-steps whose operands of A[m] are loaded together
static_assert(kTrajRows == 64, "four waves, one 16-row MFMA block each");

__device__ inline v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(256) void gmm_traj_kernel(const double *__restrict__ x, long ld_x, const int32_t *__restrict__ lengths,
                                                       long frames, int Tmax, int D, const int32_t *__restrict__ labels,
                                                       const double *__restrict__ mu_x, const double *__restrict__ mu_y,
                                                       const double *__restrict__ A, const double *__restrict__ cvar, int M,
                                                       double *__restrict__ mean, long ld_mean, double *__restrict__ var, long ld_var) {
  extern __shared__ double lds[];
  __shared__ int rowlab[kTrajRows];
  const int K4 = (D + 3) & ~3;
  const int ldx = K4 + 1;             // odd row stride: the 16 rows of an A operand fall on different banks
  double *xs = lds;                   // [kTrajRows][ldx]: x - mu_x[label], later the means
  const int tid = threadIdx.x;
  const long n0 = (long)blockIdx.x * kTrajRows;

  if (tid < kTrajRows) {
    const long n = n0 + tid;
    int s = kPad;
    if (n < frames) {
      const long b = n / Tmax;
      const int t = (int)(n - b * Tmax);
      int len = Tmax;
      if (lengths) {
        len = lengths[b];
        len = len < 0 ? 0 : (len > Tmax ? Tmax : len);
      }
      if (t < len) {
        const int m = labels[n];
        s = (m >= 0 && m < M) ? m : kBad;
      }
    }
    rowlab[tid] = s;
  }
  __syncthreads();
  for (int i = tid; i < kTrajRows * ldx; i += 256) {
    const int r = i / ldx, c = i - r * ldx;
    const int m = rowlab[r];
    xs[i] = (m >= 0 && c < D) ? x[(size_t)(n0 + r) * ld_x + c] - mu_x[(size_t)m * D + c] : 0.0;
  }
  __syncthreads();

  // wave w owns rows 16 w .. 16 w + 15 (one MFMA row block) and all column tiles of them
  const int wave = tid >> 6, lane = tid & 63;
  const int r4 = lane >> 4, c16 = lane & 15;
  const int mine = rowlab[wave * 16 + c16];
  const double *xrow = xs + (wave * 16 + c16) * ldx;   // the A operand's row
  int rl[4];                          // the labels of the rows this lane's accumulator registers belong to: row 16 w + r4 + 4 g
  double res[kTrajMaxD / 16][4];      // [column tile][accumulator register]
#pragma unroll
  for (int g = 0; g < 4; ++g) rl[g] = rowlab[wave * 16 + r4 + 4 * g];
#pragma unroll
  for (int j = 0; j < kTrajMaxD / 16; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) res[j][g] = 0.0;

  unsigned todo = (unsigned)(__ballot(mine >= 0) & 0xffffull);   // lanes 0 .. 15: the block's rows
  while (todo) {
    const int m = __builtin_amdgcn_readfirstlane(rowlab[wave * 16 + __ffsll((long long)todo) - 1]);   // wave-uniform: A[m]'s base stays scalar
    todo &= ~(unsigned)(__ballot(mine == m) & 0xffffull);
    const double *Am = A + (size_t)m * D * D;
#pragma unroll
    for (int j = 0; j < kTrajMaxD / 16; ++j) {
      if (16 * j < D) {
        const int col = 16 * j + c16;
        const bool col_ok = col < D;
        const double *arow = Am + (size_t)(col_ok ? col : 0) * D;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        // kBatch k-steps at a time: their operands are loaded together (independent loads in flight: the loop is bound by the
        // latency of the L2 reads of A[m], not by the MFMA), then multiplied in k order; steps at or past K4 are skipped whole
        for (int k0 = 0; k0 < K4; k0 += 4 * kBatch) {
          double a[kBatch], b[kBatch];
#pragma unroll
          for (int u = 0; u < kBatch; ++u) {
            const int kk = k0 + 4 * u + r4;
            b[u] = (col_ok && kk < D) ? arow[kk] : 0.0;
            a[u] = k0 + 4 * u < K4 ? xrow[kk] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < kBatch; ++u)
            if (k0 + 4 * u < K4) acc = mfma_f64(a[u], b[u], acc);
        }
        const double bias = col_ok ? mu_y[(size_t)m * D + col] : 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (rl[g] == m) res[j][g] = bias + acc[g];
      }
    }
  }
  // the means go into the wave's own rows of xs, which no other wave reads as an operand
#pragma unroll
  for (int j = 0; j < kTrajMaxD / 16; ++j) {
    const int col = 16 * j + c16;
    if (col < D) {
#pragma unroll
      for (int g = 0; g < 4; ++g) xs[(wave * 16 + r4 + 4 * g) * ldx + col] = res[j][g];
    }
  }
  __syncthreads();
  const double nan = __builtin_nan("");
  for (int i = tid; i < kTrajRows * D; i += 256) {
    const int r = i / D, c = i - r * D;
    const long n = n0 + r;
    if (n < frames) {
      const int s = rowlab[r];
      mean[(size_t)n * ld_mean + c] = s >= 0 ? xs[r * ldx + c] : (s == kBad ? nan : 0.0);
      var[(size_t)n * ld_var + c] = s >= 0 ? cvar[(size_t)s * D + c] : (s == kBad ? nan : 1.0);
    }
  }
}

}  // namespace

int launch_gmm_traj(hipStream_t st, const double *x, long ld_x, const int32_t *lengths, int B, int Tmax, int D, const int32_t *labels,
                    const double *mu_x, const double *mu_y, const double *A, const double *cvar, int M, double *mean, long ld_mean,
                    double *var, long ld_var) {
  const long frames = (long)B * Tmax;
  const unsigned blocks = (unsigned)((frames + kTrajRows - 1) / kTrajRows);
  const size_t lds_max = sizeof(double) * (size_t)kTrajRows * (kTrajMaxD + 1);   // 66 KB at D = 128; 37 KB at D = 72
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)gmm_traj_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
  const size_t lds_bytes = sizeof(double) * (size_t)kTrajRows * (((D + 3) & ~3) + 1);
  hipLaunchKernelGGL(gmm_traj_kernel, dim3(blocks), dim3(256), lds_bytes, st, x, ld_x, lengths, frames, Tmax, D, labels, mu_x, mu_y, A,
                     cvar, M, mean, ld_mean, var, ld_var);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountGmmTraj);
  return 0;
}

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int mlpg_hip_gmm_trajectory_stats(int device, void *stream, const double *x, int64_t ld_x,
                                                                         const int32_t *lengths, int B, int Tmax, int D,
                                                                         const int32_t *labels, const double *mu_x, const double *mu_y,
                                                                         const double *A, const double *cvar, int M, double *mean,
                                                                         int64_t ld_mean, double *var, int64_t ld_var) {
  const char *who = "gmm_trajectory_stats";
  if (D < 1 || D > kTrajMaxD) {
    set_error("%s: the number of features must be in [1, %d] (got %d)", who, kTrajMaxD, D);
    return MLPG_HIP_EINVAL;
  }
  if (M < 1 || M > kTrajMaxM) {
    set_error("%s: the number of mixtures must be in [1, %d] (got %d)", who, kTrajMaxM, M);
    return MLPG_HIP_EINVAL;
  }
  if (B < 0 || Tmax < 0 || ((int64_t)B * Tmax + kTrajRows - 1) / kTrajRows > 16777215LL /* 2^24 - 1 workgroups of 256 threads: a grid is 32 bits of threads, a larger one runs truncated and reports nothing */) {
    set_error("%s: bad batch shape (B = %d, Tmax = %d)", who, B, Tmax);
    return MLPG_HIP_EINVAL;
  }
  if (ld_x < D || ld_mean < D || ld_var < D) {
    set_error("%s: row strides must be at least D = %d (got ld_x = %lld, ld_mean = %lld, ld_var = %lld)", who, D, (long long)ld_x,
              (long long)ld_mean, (long long)ld_var);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || Tmax == 0) return 0;
  if (!x || !labels || !mu_x || !mu_y || !A || !cvar || !mean || !var) {
    set_error("%s: NULL data pointer (x, labels, mu_x, mu_y, A, cvar, mean and var are required)", who);
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_gmm_traj((hipStream_t)stream, x, (long)ld_x, lengths, B, Tmax, D, labels, mu_x, mu_y, A, cvar, M, mean, (long)ld_mean,
                         var, (long)ld_var);
}

}  // extern "C"
