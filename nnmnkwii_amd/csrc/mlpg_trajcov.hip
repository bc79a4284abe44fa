// K19: the other half of MLPG's trajectory distribution N(c; cbar, R^-1) over a padded batch (include/nnmnkwii_trajectory.h):
// the band of S = R^-1 and log det R -- nnmk_traj_covariance -- and the trajectory likelihood with its gradients for the means
// and the variances -- nnmk_traj_nll.  tools/trajcov_model.py is the executable specification of everything below; DESIGN.md K19
// has the contract, the layout, the budget and the error bound.
//
// Per system (utterance b, static dim d) with T live frames, R = sum_w W_w^T diag(tau_w) W_w with tau as SysView::tau
// (assemble.h) gives it and R's columns as assemble_frame adds them up (the same products in the same order; window extents <= 1,
// so a column needs tau of the frames f - 1, f, f + 1 alone).
//
// traj_cov_kernel<TIN, Q>: one lane per system, the 64 lanes of a workgroup (one wavefront) on consecutive static dims of one
// utterance, so every row access is one contiguous run.
//   forward   t = 0 .. T - 1: column t of R, plus what the columns before it left (pend), is D_t and D_t l_{t+k,t}; log D_t is
//             added up; 1 / D_t and the Q multipliers go to row t of the caller's band planes.  The variances of a frame are
//             loaded kTcAhead + 1 frames before their reciprocals are taken (a register ring of raw rows), so the loads are in
//             flight under the dependent chain (pend -> pivot -> division -> pend) of the frames in between: at 256 x 60 the launch
//             is 256 wavefronts, one per compute unit, and nothing else hides a load.
//   backward  t = T - 1 .. 0: Takahashi's recurrence from the rows the forward sweep left (read kTcAhead rows ahead, too) and the
//             Q x Q block of S behind frame t, held in registers; row t is overwritten with S[t, t .. t + Q].
// A non-positive pivot ends the forward sweep of its lane: status = the frame (from 1), logdet and the rows below T NaN.
// No LDS, no cross-lane operation, no atomics, no workgroup waits for another; every offset is 64-bit.
//
// traj_nll_kernel<TIN>: a workgroup of four waves per (utterance, 64 static dims).  Wave v walks the frames
// [v ceil(T / 4), (v + 1) ceil(T / 4)) of its lanes' systems (a partition by the system's own T: the bits do not depend on Tmax),
// adding tau (W e)^2 and, for global variances, the variance gradients per window; the four partial sums meet in LDS and wave 0
// adds them in wave order.  traj_gvar_finish_kernel: one thread per column adds the utterances' sums in order.
// Compiled with -ffp-contract=off: the model rounds every product and sum separately.
#include <math.h>

#include <atomic>

#include "assemble.h"
#include "../../include/nnmnkwii_trajectory.h"

namespace mlpg {

namespace {

constexpr int kTcAhead = 4;                  // raw variance rows / factor rows in flight
constexpr unsigned kTcMaxGrid = 16777215u;   // 2^24 - 1 workgroups (of at most 256 threads: a grid is 32 bits of threads)
constexpr double kTcLog2Pi = 1.8378770664093453;

std::atomic<long long> g_traj_launches{0};

struct TcArgs {
  const void *mean, *var;
  const int32_t *lengths;
  int var_mode, B, Tmax, sd, ngrp;   // ngrp: groups of 64 static dims
  long ld_in;
  // covariance
  double *band;
  long ld_band;
  double *logdet;
  int32_t *status;
  int want_band;
  // likelihood
  const void *cbar, *target;
  long ld_cbar, ld_target;
  const double *band_in, *logdet_in;
  double *nll;
  void *grad_means, *grad_vars;
  double *partial;   // (B, D): the utterances' sums of the global-variance gradient
};

template <typename TIN>
struct TcRow {
  TIN v[kMaxWindows];
};

// SysView::tau (assemble.h) on a variance that has been loaded already
template <typename TIN>
__device__ __forceinline__ double tc_tau(int var_mode, int mw, int T, int w, int t, TIN raw) {
  if (w != 0 && (mw == 0 || t < mw || t >= T - mw)) return 0.0;
  if (var_mode == MLPG_HIP_VAR_UNIT) return 1.0;
  return recip_in_dtype<TIN>(raw);
}

__device__ __forceinline__ int tc_length(const int32_t *lengths, int b, int Tmax) {
  if (!lengths) return Tmax;
  const int n = lengths[b];
  return n < 0 ? 0 : (n > Tmax ? Tmax : n);
}

template <typename TIN, int Q>
__global__ __launch_bounds__(64) void traj_cov_kernel(TcArgs a, WinSet ws) {
  const int lane = threadIdx.x;
  const unsigned g = blockIdx.x;
  const int b = (int)(g / (unsigned)a.ngrp), d = (int)(g - (unsigned)b * (unsigned)a.ngrp) * 64 + lane;
  if (d >= a.sd) return;   // (no cross-lane operation and no barrier below)
  const int T = tc_length(a.lengths, b, a.Tmax);
  const int nw = ws.nw, mw = ws.mw, sd = a.sd;
  const bool frame = a.var_mode == MLPG_HIP_VAR_FRAME;
  const TIN *__restrict__ var = (const TIN *)a.var;
  if (frame) var += (size_t)b * a.Tmax * a.ld_in;
  TcRow<TIN> glob;
#pragma unroll
  for (int w = 0; w < kMaxWindows; ++w) glob.v[w] = (a.var_mode == MLPG_HIP_VAR_GLOBAL && w < nw) ? var[w * sd + d] : (TIN)1;
  const size_t plane = (size_t)a.B * a.Tmax * a.ld_band;
  double *bd = a.want_band ? a.band + (size_t)b * a.Tmax * a.ld_band + d : nullptr;

  // the raw variances of frame t (no row at or past T is read)
  auto fetch = [&](int t) {
    TcRow<TIN> r = glob;
    if (frame && t < T) {
#pragma unroll
      for (int w = 0; w < kMaxWindows; ++w)
        if (w < nw) r.v[w] = var[(size_t)t * a.ld_in + w * sd + d];
    }
    return r;
  };
  auto convert = [&](const TcRow<TIN> &r, int t, double(&o)[kMaxWindows]) {
#pragma unroll
    for (int w = 0; w < kMaxWindows; ++w) o[w] = (w < nw && t < T) ? tc_tau<TIN>(a.var_mode, mw, T, w, t, r.v[w]) : 0.0;
  };

  // ---- forward: assemble, eliminate, log D_t; 1 / D_t and the multipliers to row t
  double tm[kMaxWindows], t0[kMaxWindows], tp[kMaxWindows];   // tau of the frames f - 1, f, f + 1
  TcRow<TIN> ring[kTcAhead];                                  // ring[i]: the raw variances of frame f + 2 + i
#pragma unroll
  for (int w = 0; w < kMaxWindows; ++w) tm[w] = 0.0;
  convert(fetch(0), 0, t0);
  convert(fetch(1), 1, tp);
#pragma unroll
  for (int i = 0; i < kTcAhead; ++i) ring[i] = fetch(2 + i);
  double pend[Q + 1][Q + 1];   // pend[j][k]: what the columns so far take from R[f + j + k, f + j]
#pragma unroll
  for (int j = 0; j <= Q; ++j)
#pragma unroll
    for (int k = 0; k <= Q; ++k) pend[j][k] = 0.0;
  double ld = 0.0;
  int bad = 0;
  for (int f = 0; f < T; ++f) {
    double pk[Q + 1];
#pragma unroll
    for (int k = 0; k <= Q; ++k) pk[k] = 0.0;
#pragma unroll
    for (int w = 0; w < kMaxWindows; ++w) {
      if (w < nw) {
        const int l = ws.l[w], u = ws.u[w];
        const double *cw = ws.c + ws.off[w];
#pragma unroll
        for (int s = -1; s <= 1; ++s) {   // frame t = f + s, as assemble_frame walks t = f - u .. f + l
          if (s >= -u && s <= l && f + s >= 0 && f + s < T) {
            const double tau = s < 0 ? tm[w] : (s == 0 ? t0[w] : tp[w]);
            const double av = cw[l - s] * tau;
#pragma unroll
            for (int k = 0; k <= Q; ++k) {
              const int idx = l - s + k;
              if (idx <= l + u && f + k < T) pk[k] += av * cw[idx];
            }
          }
        }
      }
    }
    double col[Q + 1];
#pragma unroll
    for (int k = 0; k <= Q; ++k) col[k] = pk[k] + pend[0][k];
    if (col[0] <= 0.0) {
      bad = f + 1;
      break;
    }
    const double iv = 1.0 / col[0];
    ld += log(col[0]);
    double m[Q + 1];
    m[0] = iv;
#pragma unroll
    for (int k = 1; k <= Q; ++k) m[k] = col[k] * iv;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
#pragma unroll
      for (int k = 0; k <= Q; ++k) {
        double nv = pend[j + 1][k];
        if (k + j + 1 <= Q) nv -= m[j + 1] * col[k + j + 1];
        pend[j][k] = nv;
      }
    }
    if (bd) {
#pragma unroll
      for (int k = 0; k <= Q; ++k) bd[k * plane + (size_t)f * a.ld_band] = m[k];
    }
#pragma unroll
    for (int w = 0; w < kMaxWindows; ++w) {
      tm[w] = t0[w];
      t0[w] = tp[w];
    }
    convert(ring[0], f + 2, tp);
#pragma unroll
    for (int i = 0; i + 1 < kTcAhead; ++i) ring[i] = ring[i + 1];
    ring[kTcAhead - 1] = fetch(f + 2 + kTcAhead);
  }
  const size_t o = (size_t)b * sd + d;
  a.status[o] = bad;
  a.logdet[o] = bad ? (double)NAN : ld;
  if (!bd) return;
  for (int t = T; t < a.Tmax; ++t) {
#pragma unroll
    for (int k = 0; k <= Q; ++k) bd[k * plane + (size_t)t * a.ld_band] = 0.0;
  }
  if (bad) {
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int k = 0; k <= Q; ++k) bd[k * plane + (size_t)t * a.ld_band] = (double)NAN;
    }
    return;
  }

  // ---- backward: S[t, t .. t + Q] from row t of the factor and the block Z[i][j] = S[t + 1 + i, t + 1 + j]
  constexpr int QZ = Q > 0 ? Q : 1;
  double Z[QZ][QZ];
#pragma unroll
  for (int i = 0; i < QZ; ++i)
#pragma unroll
    for (int j = 0; j < QZ; ++j) Z[i][j] = 0.0;
  double fr[kTcAhead][Q + 1];   // fr[i]: row t - i of the factor
#pragma unroll
  for (int i = 0; i < kTcAhead; ++i)
#pragma unroll
    for (int k = 0; k <= Q; ++k) fr[i][k] = T - 1 - i >= 0 ? bd[k * plane + (size_t)(T - 1 - i) * a.ld_band] : 0.0;
  for (int t = T - 1; t >= 0; --t) {
    double m[Q + 1], s[Q + 1];
#pragma unroll
    for (int k = 0; k <= Q; ++k) m[k] = fr[0][k];
#pragma unroll
    for (int i = 0; i + 1 < kTcAhead; ++i)
#pragma unroll
      for (int k = 0; k <= Q; ++k) fr[i][k] = fr[i + 1][k];
#pragma unroll
    for (int k = 0; k <= Q; ++k) fr[kTcAhead - 1][k] = t - kTcAhead >= 0 ? bd[k * plane + (size_t)(t - kTcAhead) * a.ld_band] : 0.0;
    s[0] = m[0];
    if constexpr (Q > 0) {
#pragma unroll
      for (int k = 1; k <= Q; ++k) {
        double acc = m[1] * Z[0][k - 1];
#pragma unroll
        for (int j = 2; j <= Q; ++j) acc += m[j] * Z[j - 1][k - 1];
        s[k] = t + k < T ? -acc : 0.0;
      }
      double acc = m[1] * s[1];
#pragma unroll
      for (int j = 2; j <= Q; ++j) acc += m[j] * s[j];
      s[0] = m[0] - acc;
    }
#pragma unroll
    for (int k = 0; k <= Q; ++k) bd[k * plane + (size_t)t * a.ld_band] = s[k];
    if constexpr (Q > 0) {
#pragma unroll
      for (int i = QZ - 1; i >= 1; --i)
#pragma unroll
        for (int j = QZ - 1; j >= 1; --j) Z[i][j] = Z[i - 1][j - 1];
#pragma unroll
      for (int j = 1; j < QZ; ++j) Z[0][j] = Z[j][0] = s[j];
      Z[0][0] = s[0];
    }
  }
}

template <typename TIN>
__global__ __launch_bounds__(256) void traj_nll_kernel(TcArgs a, WinSet ws) {
  __shared__ double red[4][kMaxWindows + 1][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned g = blockIdx.x;
  const int b = (int)(g / (unsigned)a.ngrp), d = (int)(g - (unsigned)b * (unsigned)a.ngrp) * 64 + lane;
  const bool live = d < a.sd;
  const int T = tc_length(a.lengths, b, a.Tmax);
  const int nw = ws.nw, mw = ws.mw, sd = a.sd, Q = ws.q, D = nw * sd;
  const int per = (T + 3) / 4;
  const int f0 = wave * per < T ? wave * per : T, f1 = f0 + per < T ? f0 + per : T;
  const bool frame = a.var_mode == MLPG_HIP_VAR_FRAME;
  double quad = 0.0, gsum[kMaxWindows];
#pragma unroll
  for (int w = 0; w < kMaxWindows; ++w) gsum[w] = 0.0;
  if (live) {
    const TIN *__restrict__ mean = (const TIN *)a.mean + (size_t)b * a.Tmax * a.ld_in;
    const TIN *__restrict__ var = (const TIN *)a.var;
    if (frame) var += (size_t)b * a.Tmax * a.ld_in;
    const TIN *__restrict__ cb = (const TIN *)a.cbar + (size_t)b * a.Tmax * a.ld_cbar + d;
    const TIN *__restrict__ tg = (const TIN *)a.target + (size_t)b * a.Tmax * a.ld_target + d;
    TIN *gm = a.grad_means ? (TIN *)a.grad_means + (size_t)b * a.Tmax * D : nullptr;
    TIN *gv = (a.grad_vars && frame) ? (TIN *)a.grad_vars + (size_t)b * a.Tmax * D : nullptr;
    const bool want_gv = a.grad_vars != nullptr;
    const size_t plane = (size_t)a.B * a.Tmax * a.ld_band;
    const double *__restrict__ bd = want_gv ? a.band_in + (size_t)b * a.Tmax * a.ld_band + d : nullptr;
    for (int t = f0; t < f1; ++t) {
      // cbar and e = c - cbar of the frames t - 1, t, t + 1 (0 outside [0, T): never used)
      double cbv[3], ev[3];
#pragma unroll
      for (int s = -1; s <= 1; ++s) {
        const bool in = t + s >= 0 && t + s < T;
        cbv[s + 1] = in ? (double)cb[(size_t)(t + s) * a.ld_cbar] : 0.0;
        ev[s + 1] = in ? (double)tg[(size_t)(t + s) * a.ld_target] - cbv[s + 1] : 0.0;
      }
      // S[t + i, t + j], i <= j in {-1, 0, 1}: sb[i + 1][j - i] = plane j - i, row t + i
      double sb[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int row = t + i - 1;
          sb[i][k] = (want_gv && i + k < 3 && k <= Q && row >= 0 && row + k < T) ? bd[k * plane + (size_t)row * a.ld_band] : 0.0;
        }
#pragma unroll
      for (int w = 0; w < kMaxWindows; ++w) {
        if (w < nw) {
          const int l = ws.l[w], u = ws.u[w];
          const double *cw = ws.c + ws.off[w];
          const size_t col = (size_t)w * sd + d;
          double av = 0.0, gc = 0.0;
#pragma unroll
          for (int s = -1; s <= 1; ++s) {
            if (s >= -l && s <= u && t + s >= 0 && t + s < T) {
              av += cw[l + s] * ev[s + 1];
              gc += cw[l + s] * cbv[s + 1];
            }
          }
          const bool forced = w != 0 && (mw == 0 || t < mw || t >= T - mw);
          TIN raw = (TIN)1;
          if (!forced && a.var_mode != MLPG_HIP_VAR_UNIT) raw = frame ? var[(size_t)t * a.ld_in + col] : var[col];
          const double tau = tc_tau<TIN>(a.var_mode, mw, T, w, t, raw);
          const double aa = av * av;
          quad += tau * aa;
          if (gm) gm[(size_t)t * D + col] = (TIN)(-(tau * av));
          if (want_gv) {
            double gvar = 0.0;
            if (!forced) {
              double cov = 0.0;
#pragma unroll
              for (int i = -1; i <= 1; ++i)
#pragma unroll
                for (int j = -1; j <= 1; ++j) {
                  if (i >= -l && i <= u && j >= -l && j <= u && t + i >= 0 && t + i < T && t + j >= 0 && t + j < T) {
                    const int lo = i < j ? i : j, hi = i < j ? j : i;
                    cov += (cw[l + i] * cw[l + j]) * sb[lo + 1][hi - lo];
                  }
                }
              const double mu = (double)mean[(size_t)t * a.ld_in + col];
              const double gtau = (0.5 * aa - av * (mu - gc)) - 0.5 * cov;
              gvar = -((tau * tau) * gtau);
            }
            if (gv) gv[(size_t)t * D + col] = (TIN)gvar;
            gsum[w] += gvar;
          }
        }
      }
    }
    // rows at or past T: zeros (wave v takes T + v, T + v + 4, ...)
    for (int t = T + wave; t < a.Tmax; t += 4) {
      for (int w = 0; w < nw; ++w) {
        if (gm) gm[(size_t)t * D + (size_t)w * sd + d] = (TIN)0;
        if (gv) gv[(size_t)t * D + (size_t)w * sd + d] = (TIN)0;
      }
    }
  }
  red[wave][0][lane] = quad;
#pragma unroll
  for (int w = 0; w < kMaxWindows; ++w) red[wave][1 + w][lane] = gsum[w];
  __syncthreads();
  if (wave == 0 && live) {
    const double q = ((red[0][0][lane] + red[1][0][lane]) + red[2][0][lane]) + red[3][0][lane];
    const size_t o = (size_t)b * sd + d;
    a.nll[o] = (0.5 * q - 0.5 * a.logdet_in[o]) + (0.5 * (double)T) * kTcLog2Pi;
    if (a.partial) {
      for (int w = 0; w < nw; ++w)
        a.partial[(size_t)b * D + (size_t)w * sd + d] = ((red[0][1 + w][lane] + red[1][1 + w][lane]) + red[2][1 + w][lane]) + red[3][1 + w][lane];
    }
  }
}

// grad_vars[j] = sum_b partial[b, j], the utterances in order
template <typename TIN>
__global__ __launch_bounds__(256) void traj_gvar_finish_kernel(const double *__restrict__ partial, int B, int D, TIN *__restrict__ out) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= D) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += partial[(size_t)b * D + j];
  out[j] = (TIN)s;
}

int tc_refuse(const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  set_error(fmt, a, b, c, d);
  return MLPG_HIP_EINVAL;
}

bool tc_overlap(const void *p, size_t np, const void *q, size_t nq) {
  if (!p || !q || !np || !nq) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

// bytes from the first to behind the last element of `rows` rows of `width` elements with stride ld
size_t tc_span(int64_t rows, int64_t ld, int64_t width, size_t elem) {
  return rows > 0 && width > 0 ? (size_t)((rows - 1) * ld + width) * elem : 0;
}

// `rows` rows of stride ld (in elements of at most 8 bytes) end below 2^62 bytes: every offset the kernels and tc_span form fits
bool tc_stride_fits(int64_t planes, int B, int Tmax, int64_t ld) {
  const __int128 rows = (__int128)planes * B * Tmax;
  return (__int128)ld <= ((__int128)1 << 59) / (rows > 0 ? rows : 1);
}

int tc_refuse_stride(const char *name, int64_t ld) {
  set_error("trajectory: the row stride %s = %lld puts the batch's last row past 2^62 bytes", name, (long long)ld);
  return MLPG_HIP_EINVAL;
}

// what both entries ask of the batch, the variances and the windows; the window set on the way
int tc_check(int dtype, const void *variances, int var_mode, int64_t ld_in, int B, int Tmax, int D, int sd, int num_windows,
             const int32_t *wl, const int32_t *wu, const double *wc, WinSet *ws) {
  const char *who = "trajectory";
  if (int rc = check_dtype(who, dtype)) return rc;
  if (var_mode < 0 || var_mode > 2) return tc_refuse("trajectory: unknown var_mode %lld", var_mode);
  if (B < 0 || Tmax < 0 || D < 0 || sd < 0) return tc_refuse("trajectory: negative size (B = %lld, Tmax = %lld, D = %lld, sd = %lld)", B, Tmax, D, sd);
  if (num_windows < 1 || num_windows > kMaxWindows || !wl || !wu || !wc)
    return tc_refuse("trajectory: num_windows must be in [1, %lld] and the window tables non-NULL", kMaxWindows);
  if ((int64_t)num_windows * sd != (int64_t)D) return tc_refuse("trajectory: D = %lld is not num_windows * sd = %lld * %lld", D, num_windows, sd);
  for (int w = 0; w < num_windows; ++w)
    if (wl[w] < 0 || wu[w] < 0 || wl[w] > 1 || wu[w] > 1)
      return tc_refuse("trajectory: window %lld: extents (l = %lld, u = %lld) must be 0 or 1", w, wl[w], wu[w]);
  if (var_mode == MLPG_HIP_VAR_FRAME && ld_in < D) return tc_refuse("trajectory: the row stride ld_in = %lld is below D = %lld", ld_in, D);
  if (!tc_stride_fits(1, B, Tmax, ld_in > D ? ld_in : D)) return tc_refuse_stride("ld_in", ld_in);
  if ((int64_t)B * ((sd + 63) / 64) > (int64_t)kTcMaxGrid)
    return tc_refuse("trajectory: the batch is too large for one grid (B = %lld, sd = %lld)", B, sd);
  if (pack_windows(num_windows, wl, wu, wc, ws)) return tc_refuse("trajectory: bad window tables");
  return 0;
}

template <typename K>
int tc_launch(K kern, hipStream_t st, unsigned blocks, int threads, const TcArgs &a, const WinSet &ws) {
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, st, a, ws);
  MLPG_HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename TIN>
int launch_traj_cov(hipStream_t st, unsigned blocks, const TcArgs &a, const WinSet &ws) {
  if (ws.q == 0) return tc_launch(traj_cov_kernel<TIN, 0>, st, blocks, 64, a, ws);
  if (ws.q == 1) return tc_launch(traj_cov_kernel<TIN, 1>, st, blocks, 64, a, ws);
  return tc_launch(traj_cov_kernel<TIN, 2>, st, blocks, 64, a, ws);
}

template <typename TIN>
int launch_traj_nll(hipStream_t st, unsigned blocks, const TcArgs &a, const WinSet &ws, int D) {
  if (int rc = tc_launch(traj_nll_kernel<TIN>, st, blocks, 256, a, ws)) return rc;
  if (a.partial) {
    hipLaunchKernelGGL(traj_gvar_finish_kernel<TIN>, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, (const double *)a.partial, a.B, D,
                       (TIN *)a.grad_vars);
    MLPG_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int nnmk_traj_abi_version(void) { return NNMK_TRAJ_ABI_VERSION; }

__attribute__((visibility("default"))) long long nnmk_traj_launch_count(void) { return g_traj_launches.load(std::memory_order_relaxed); }

__attribute__((visibility("default"))) int64_t nnmk_traj_nll_workspace(int var_mode, int want_grad_vars, int B, int D) {
  if (var_mode < 0 || var_mode > 2 || B < 0 || D < 0) return -1;
  return var_mode == MLPG_HIP_VAR_GLOBAL && want_grad_vars ? (int64_t)8 * B * D : 0;
}

__attribute__((visibility("default"))) int nnmk_traj_covariance(int device, void *stream, int dtype, const void *variances, int var_mode,
                                                                int64_t ld_in, const int32_t *lengths, int B, int Tmax, int D, int sd,
                                                                int num_windows, const int32_t *win_l, const int32_t *win_u,
                                                                const double *win_coef, int want_band, double *band, int64_t ld_band,
                                                                double *logdet, int32_t *status) {
  const char *who = "trajectory";
  WinSet ws;
  if (int rc = tc_check(dtype, variances, var_mode, ld_in, B, Tmax, D, sd, num_windows, win_l, win_u, win_coef, &ws)) return rc;
  if (want_band && ld_band < sd) return tc_refuse("trajectory: the row stride ld_band = %lld is below sd = %lld", ld_band, sd);
  if (want_band && !tc_stride_fits(3 /* Q + 1 <= 3 planes */, B, Tmax, ld_band)) return tc_refuse_stride("ld_band", ld_band);
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || Tmax == 0 || sd == 0) return 0;
  if (var_mode != MLPG_HIP_VAR_UNIT && !variances) return tc_refuse("trajectory: NULL variances");
  if (!logdet || !status) return tc_refuse("trajectory: NULL logdet or status");
  if (want_band && !band) return tc_refuse("trajectory: NULL band (want_band = %lld)", want_band);
  const size_t esz = dtype == MLPG_HIP_F32 ? 4 : 8;
  if (want_band) {
    const size_t nband = tc_span((int64_t)(ws.q + 1) * B * Tmax, ld_band, sd, 8);
    const size_t nvar = var_mode == MLPG_HIP_VAR_FRAME ? tc_span((int64_t)B * Tmax, ld_in, D, esz) : (size_t)D * esz;
    if (tc_overlap(band, nband, variances, nvar) || tc_overlap(band, nband, lengths, (size_t)B * 4))
      return tc_refuse("trajectory: the band planes overlap an input (the factor is kept in them while the variances are read)");
    if (tc_overlap(band, nband, logdet, (size_t)B * sd * 8) || tc_overlap(band, nband, status, (size_t)B * sd * 4))
      return tc_refuse("trajectory: the band planes overlap logdet or status");
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  TcArgs a = {};
  a.var = variances;
  a.lengths = lengths;
  a.var_mode = var_mode;
  a.B = B;
  a.Tmax = Tmax;
  a.sd = sd;
  a.ngrp = (sd + 63) / 64;
  a.ld_in = (long)ld_in;
  a.band = band;
  a.ld_band = (long)ld_band;
  a.logdet = logdet;
  a.status = status;
  a.want_band = want_band != 0;
  const unsigned blocks = (unsigned)((int64_t)B * a.ngrp);
  const int rc = dtype == MLPG_HIP_F32 ? launch_traj_cov<float>((hipStream_t)stream, blocks, a, ws)
                                       : launch_traj_cov<double>((hipStream_t)stream, blocks, a, ws);
  if (rc == 0) g_traj_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

__attribute__((visibility("default"))) int nnmk_traj_nll(int device, void *stream, int dtype, const void *means, const void *variances,
                                                         int var_mode, int64_t ld_in, const int32_t *lengths, int B, int Tmax, int D,
                                                         int sd, int num_windows, const int32_t *win_l, const int32_t *win_u,
                                                         const double *win_coef, const void *cbar, int64_t ld_cbar, const void *target,
                                                         int64_t ld_target, const double *band, int64_t ld_band, const double *logdet,
                                                         double *nll, void *grad_means, void *grad_vars, void *workspace,
                                                         int64_t workspace_bytes) {
  const char *who = "trajectory";
  WinSet ws;
  if (int rc = tc_check(dtype, variances, var_mode, ld_in, B, Tmax, D, sd, num_windows, win_l, win_u, win_coef, &ws)) return rc;
  if (ld_in < D) return tc_refuse("trajectory: the row stride ld_in = %lld is below D = %lld", ld_in, D);
  if (ld_cbar < sd || ld_target < sd)
    return tc_refuse("trajectory: the row strides ld_cbar = %lld and ld_target = %lld must reach sd = %lld", ld_cbar, ld_target, sd);
  if (grad_vars && var_mode == MLPG_HIP_VAR_UNIT) return tc_refuse("trajectory: unit variances have no gradient (grad_vars must be NULL)");
  if (grad_vars && ld_band < sd) return tc_refuse("trajectory: the row stride ld_band = %lld is below sd = %lld", ld_band, sd);
  if (grad_vars && !tc_stride_fits(3 /* Q + 1 <= 3 planes */, B, Tmax, ld_band)) return tc_refuse_stride("ld_band", ld_band);
  if (!tc_stride_fits(1, B, Tmax, ld_cbar)) return tc_refuse_stride("ld_cbar", ld_cbar);
  if (!tc_stride_fits(1, B, Tmax, ld_target)) return tc_refuse_stride("ld_target", ld_target);
  const int64_t need = nnmk_traj_nll_workspace(var_mode, grad_vars != nullptr, B, D);
  if (workspace_bytes < need || (need > 0 && (!workspace || ((uintptr_t)workspace & 7))))
    return tc_refuse("trajectory: the workspace must be %lld bytes, 8-byte aligned (got %lld)", need, workspace_bytes);
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || Tmax == 0 || sd == 0) return 0;
  if (var_mode != MLPG_HIP_VAR_UNIT && !variances) return tc_refuse("trajectory: NULL variances");
  if (!means || !cbar || !target || !logdet || !nll) return tc_refuse("trajectory: NULL means, cbar, target, logdet or nll");
  if (grad_vars && !band) return tc_refuse("trajectory: the variance gradient needs the band (band is NULL)");
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  TcArgs a = {};
  a.mean = means;
  a.var = variances;
  a.lengths = lengths;
  a.var_mode = var_mode;
  a.B = B;
  a.Tmax = Tmax;
  a.sd = sd;
  a.ngrp = (sd + 63) / 64;
  a.ld_in = (long)ld_in;
  a.cbar = cbar;
  a.target = target;
  a.ld_cbar = (long)ld_cbar;
  a.ld_target = (long)ld_target;
  a.band_in = band;
  a.ld_band = (long)ld_band;
  a.logdet_in = logdet;
  a.nll = nll;
  a.grad_means = grad_means;
  a.grad_vars = grad_vars;
  a.partial = need > 0 ? (double *)workspace : nullptr;
  const unsigned blocks = (unsigned)((int64_t)B * a.ngrp);
  const int rc = dtype == MLPG_HIP_F32 ? launch_traj_nll<float>((hipStream_t)stream, blocks, a, ws, D)
                                       : launch_traj_nll<double>((hipStream_t)stream, blocks, a, ws, D);
  if (rc == 0) g_traj_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

}  // extern "C"
