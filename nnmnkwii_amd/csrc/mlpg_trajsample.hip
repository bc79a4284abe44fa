// K20: draws from MLPG's trajectory distribution N(c; cbar, R^-1) over a padded batch and the inverse map that whitens a
// trajectory under it (include/nnmnkwii_sample.h).  tools/trajsample_model.py is the executable specification of everything below;
// DESIGN.md K20 has the contract, the layout, the group size and the error bound.
//
// With R = L D L^T (banded, unit L): a draw is c = cbar + L^-T D^-1/2 z, the inverse map z = D^1/2 L^T (c - cbar).
//
// draw_factor_kernel<TIN, Q>: the forward sweep of traj_cov_kernel (mlpg_trajcov.hip), RESTATED here statement for statement --
// the same products and sums in the same order, so the rows are bit for bit those that kernel leaves before its backward sweep
// overwrites them.  (It is not shared through a header: tests/test_trajcov_host_cpu.py builds mlpg_trajcov.hip from a fixed list
// of files and plants its defects in that file's own text.)  One lane per system, the 64 lanes of a workgroup (one wavefront) on
// consecutive static dims of one utterance; the raw variances ride a register ring kTcAhead + 1 frames ahead of their use.
//
// draw_sample_kernel<TIN, Q>: the same lanes.  Back-substitution t = T - 1 .. 0; a lane carries the kDrawGroup draws of a group
// side by side -- independent chains that share the factor row and its square root -- and takes the groups one after another.
// The factor row, the group's noise and the mean of frame t are loaded kTcAhead frames before they are used.
//
// draw_whiten_kernel<TIN>: four waves per (utterance, 64 static dims); wave v takes the frames [v ceil(T / 4), (v + 1) ceil(T / 4))
// of its lanes' systems.  No chain along time: a frame's result depends on that frame's inputs alone.
// No LDS, no cross-lane operation, no barrier, no atomics, no workgroup waits for another; every offset is 64-bit.
// Compiled with -ffp-contract=off: the model rounds every product and sum separately.
#include <math.h>

#include <atomic>

#include "assemble.h"
#include "../../include/nnmnkwii_sample.h"

namespace mlpg {

namespace {

constexpr int kTcAhead = 4;                  // rows in flight (as mlpg_trajcov.hip)
constexpr int kDrawGroup = 4;                // draws a lane carries side by side (the resource table)
constexpr unsigned kDrMaxGrid = 16777215u;   // 2^24 - 1 workgroups (of at most 256 threads: a grid is 32 bits of threads)

std::atomic<long long> g_draw_launches{0};

struct DrArgs {
  const int32_t *lengths;
  int B, Tmax, sd, ngrp;   // ngrp: groups of 64 static dims
  // factor
  const void *var;
  int var_mode;
  long ld_in;
  double *fac;
  double *logdet;
  int32_t *status;
  // sample, whiten
  const double *fac_in;
  long ld_fac;
  const int32_t *status_in;
  int Q, K;
  const void *src, *mean;   // src: the noise (sample) or x (whiten)
  void *dst;
  long ld_src, ld_mean, ld_dst;
};

template <typename TIN>
struct DrVarRow {
  TIN v[kMaxWindows];
};

// SysView::tau (assemble.h) on a variance that has been loaded already
template <typename TIN>
__device__ __forceinline__ double dr_tau(int var_mode, int mw, int T, int w, int t, TIN raw) {
  if (w != 0 && (mw == 0 || t < mw || t >= T - mw)) return 0.0;
  if (var_mode == MLPG_HIP_VAR_UNIT) return 1.0;
  return recip_in_dtype<TIN>(raw);
}

__device__ __forceinline__ int dr_length(const int32_t *lengths, int b, int Tmax) {
  if (!lengths) return Tmax;
  const int n = lengths[b];
  return n < 0 ? 0 : (n > Tmax ? Tmax : n);
}

template <typename TIN, int Q>
__global__ __launch_bounds__(64) void draw_factor_kernel(DrArgs a, WinSet ws) {
  const int lane = threadIdx.x;
  const unsigned g = blockIdx.x;
  const int b = (int)(g / (unsigned)a.ngrp), d = (int)(g - (unsigned)b * (unsigned)a.ngrp) * 64 + lane;
  if (d >= a.sd) return;   // (no cross-lane operation and no barrier below)
  const int T = dr_length(a.lengths, b, a.Tmax);
  const int nw = ws.nw, mw = ws.mw, sd = a.sd;
  const bool frame = a.var_mode == MLPG_HIP_VAR_FRAME;
  const TIN *__restrict__ var = (const TIN *)a.var;
  if (frame) var += (size_t)b * a.Tmax * a.ld_in;
  DrVarRow<TIN> glob;
#pragma unroll
  for (int w = 0; w < kMaxWindows; ++w) glob.v[w] = (a.var_mode == MLPG_HIP_VAR_GLOBAL && w < nw) ? var[w * sd + d] : (TIN)1;
  const size_t plane = (size_t)a.B * a.Tmax * a.ld_fac;
  double *fd = a.fac + (size_t)b * a.Tmax * a.ld_fac + d;

  // the raw variances of frame t (no row at or past T is read)
  auto fetch = [&](int t) {
    DrVarRow<TIN> r = glob;
    if (frame && t < T) {
#pragma unroll
      for (int w = 0; w < kMaxWindows; ++w)
        if (w < nw) r.v[w] = var[(size_t)t * a.ld_in + w * sd + d];
    }
    return r;
  };
  auto convert = [&](const DrVarRow<TIN> &r, int t, double(&o)[kMaxWindows]) {
#pragma unroll
    for (int w = 0; w < kMaxWindows; ++w) o[w] = (w < nw && t < T) ? dr_tau<TIN>(a.var_mode, mw, T, w, t, r.v[w]) : 0.0;
  };

  double tm[kMaxWindows], t0[kMaxWindows], tp[kMaxWindows];   // tau of the frames f - 1, f, f + 1
  DrVarRow<TIN> ring[kTcAhead];                               // ring[i]: the raw variances of frame f + 2 + i
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
#pragma unroll
    for (int k = 0; k <= Q; ++k) fd[k * plane + (size_t)f * a.ld_fac] = m[k];
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
  for (int t = T; t < a.Tmax; ++t) {
#pragma unroll
    for (int k = 0; k <= Q; ++k) fd[k * plane + (size_t)t * a.ld_fac] = 0.0;
  }
  if (bad) {
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int k = 0; k <= Q; ++k) fd[k * plane + (size_t)t * a.ld_fac] = (double)NAN;
    }
  }
}

// what back-substitution needs of frame t: the factor row, the group's noise and the mean
template <typename TIN, int Q>
struct DrRow {
  double f[Q + 1];
  TIN z[kDrawGroup];
  TIN m;
};

template <typename TIN, int Q>
__global__ __launch_bounds__(64) void draw_sample_kernel(DrArgs a) {
  const int lane = threadIdx.x;
  const unsigned g = blockIdx.x;
  const int b = (int)(g / (unsigned)a.ngrp), d = (int)(g - (unsigned)b * (unsigned)a.ngrp) * 64 + lane;
  if (d >= a.sd) return;   // (no cross-lane operation and no barrier below)
  const int T = dr_length(a.lengths, b, a.Tmax);
  const bool bad = a.status_in[(size_t)b * a.sd + d] != 0;
  const size_t plane = (size_t)a.B * a.Tmax * a.ld_fac;
  const size_t dsrc = (size_t)a.B * a.Tmax * a.ld_src, ddst = (size_t)a.B * a.Tmax * a.ld_dst;   // draw strides
  const double *__restrict__ fd = a.fac_in + (size_t)b * a.Tmax * a.ld_fac + d;
  const TIN *__restrict__ mn = a.mean ? (const TIN *)a.mean + (size_t)b * a.Tmax * a.ld_mean + d : nullptr;
  for (int k0 = 0; k0 < a.K; k0 += kDrawGroup) {
    const int n = a.K - k0 < kDrawGroup ? a.K - k0 : kDrawGroup;   // the last group may be short: its other slots stay idle
    const TIN *__restrict__ nz = (const TIN *)a.src + (size_t)k0 * dsrc + (size_t)b * a.Tmax * a.ld_src + d;
    TIN *out = (TIN *)a.dst + (size_t)k0 * ddst + (size_t)b * a.Tmax * a.ld_dst + d;
    for (int t = T; t < a.Tmax; ++t) {
#pragma unroll
      for (int i = 0; i < kDrawGroup; ++i)
        if (i < n) out[i * ddst + (size_t)t * a.ld_dst] = (TIN)0;
    }
    if (bad) {
      for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int i = 0; i < kDrawGroup; ++i)
          if (i < n) out[i * ddst + (size_t)t * a.ld_dst] = (TIN)NAN;
      }
      continue;
    }
    auto fetch = [&](int t) {
      DrRow<TIN, Q> r;
#pragma unroll
      for (int k = 0; k <= Q; ++k) r.f[k] = t >= 0 ? fd[k * plane + (size_t)t * a.ld_fac] : 0.0;
#pragma unroll
      for (int i = 0; i < kDrawGroup; ++i) r.z[i] = (t >= 0 && i < n) ? nz[i * dsrc + (size_t)t * a.ld_src] : (TIN)0;
      r.m = (t >= 0 && mn) ? mn[(size_t)t * a.ld_mean] : (TIN)0;
      return r;
    };
    DrRow<TIN, Q> ring[kTcAhead];   // ring[i]: frame t - i
#pragma unroll
    for (int i = 0; i < kTcAhead; ++i) ring[i] = fetch(T - 1 - i);
    double x1[kDrawGroup], x2[kDrawGroup];   // x of the frames t + 1, t + 2
#pragma unroll
    for (int i = 0; i < kDrawGroup; ++i) x1[i] = x2[i] = 0.0;
    for (int t = T - 1; t >= 0; --t) {
      const DrRow<TIN, Q> r = ring[0];
#pragma unroll
      for (int i = 0; i + 1 < kTcAhead; ++i) ring[i] = ring[i + 1];
      ring[kTcAhead - 1] = fetch(t - kTcAhead);
      const double sq = sqrt(r.f[0]);
#pragma unroll
      for (int i = 0; i < kDrawGroup; ++i) {
        double x = (double)r.z[i] * sq;
        if constexpr (Q >= 1) {
          if (t + 1 < T) x -= r.f[1] * x1[i];
        }
        if constexpr (Q >= 2) {
          if (t + 2 < T) x -= r.f[2] * x2[i];
        }
        if (i < n) out[i * ddst + (size_t)t * a.ld_dst] = (TIN)(mn ? (double)r.m + x : x);
        x2[i] = x1[i];
        x1[i] = x;
      }
    }
  }
}

template <typename TIN>
__global__ __launch_bounds__(256) void draw_whiten_kernel(DrArgs a) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned g = blockIdx.x;
  const int b = (int)(g / (unsigned)a.ngrp), d = (int)(g - (unsigned)b * (unsigned)a.ngrp) * 64 + lane;
  if (d >= a.sd) return;   // (no cross-lane operation and no barrier below)
  const int T = dr_length(a.lengths, b, a.Tmax), Q = a.Q;
  const int per = (T + 3) / 4;
  const int f0 = wave * per < T ? wave * per : T, f1 = f0 + per < T ? f0 + per : T;
  const bool bad = a.status_in[(size_t)b * a.sd + d] != 0;
  const size_t plane = (size_t)a.B * a.Tmax * a.ld_fac;
  const size_t dsrc = (size_t)a.B * a.Tmax * a.ld_src, ddst = (size_t)a.B * a.Tmax * a.ld_dst;
  const double *__restrict__ fd = a.fac_in + (size_t)b * a.Tmax * a.ld_fac + d;
  const TIN *__restrict__ mn = a.mean ? (const TIN *)a.mean + (size_t)b * a.Tmax * a.ld_mean + d : nullptr;
  const TIN *__restrict__ xs = (const TIN *)a.src + (size_t)b * a.Tmax * a.ld_src + d;
  TIN *out = (TIN *)a.dst + (size_t)b * a.Tmax * a.ld_dst + d;
  for (int t = f0; t < f1; ++t) {
    if (bad) {
      for (int k = 0; k < a.K; ++k) out[k * ddst + (size_t)t * a.ld_dst] = (TIN)NAN;
      continue;
    }
    const bool in1 = Q >= 1 && t + 1 < T, in2 = Q >= 2 && t + 2 < T;
    const double sq = sqrt(fd[(size_t)t * a.ld_fac]);
    const double m1 = in1 ? fd[plane + (size_t)t * a.ld_fac] : 0.0, m2 = in2 ? fd[2 * plane + (size_t)t * a.ld_fac] : 0.0;
    double mu[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) mu[s] = (mn && t + s < T) ? (double)mn[(size_t)(t + s) * a.ld_mean] : 0.0;
    for (int k = 0; k < a.K; ++k) {
      const TIN *xk = xs + k * dsrc;
      double acc = (double)xk[(size_t)t * a.ld_src];
      if (mn) acc -= mu[0];
      if (in1) {
        double e = (double)xk[(size_t)(t + 1) * a.ld_src];
        if (mn) e -= mu[1];
        acc += m1 * e;
      }
      if (in2) {
        double e = (double)xk[(size_t)(t + 2) * a.ld_src];
        if (mn) e -= mu[2];
        acc += m2 * e;
      }
      out[k * ddst + (size_t)t * a.ld_dst] = (TIN)(acc / sq);
    }
  }
  // rows at or past T: zeros (wave v takes T + v, T + v + 4, ...)
  for (int t = T + wave; t < a.Tmax; t += 4)
    for (int k = 0; k < a.K; ++k) out[k * ddst + (size_t)t * a.ld_dst] = (TIN)0;
}

int dr_refuse(const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  set_error(fmt, a, b, c, d);
  return MLPG_HIP_EINVAL;
}

bool dr_overlap(const void *p, size_t np, const void *q, size_t nq) {
  if (!p || !q || !np || !nq) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

// bytes from the first to behind the last element of `rows` rows of `width` elements with stride ld
size_t dr_span(int64_t rows, int64_t ld, int64_t width, size_t elem) {
  return rows > 0 && width > 0 ? (size_t)((rows - 1) * ld + width) * elem : 0;
}

// `planes * B * Tmax` rows of stride ld (in elements of at most 8 bytes) end below 2^62 bytes: every offset formed here fits
bool dr_stride_fits(int64_t planes, int B, int Tmax, int64_t ld) {
  const __int128 rows = (__int128)planes * B * Tmax;
  return (__int128)ld <= ((__int128)1 << 59) / (rows > 0 ? rows : 1);
}

int dr_refuse_stride(const char *name, int64_t ld) {
  set_error("sample: the row stride %s = %lld puts the last row past 2^62 bytes", name, (long long)ld);
  return MLPG_HIP_EINVAL;
}

int dr_check_grid(int B, int sd) {
  if ((int64_t)B * ((sd + 63) / 64) > (int64_t)kDrMaxGrid) return dr_refuse("sample: the batch is too large for one grid (B = %lld, sd = %lld)", B, sd);
  return 0;
}

// what nnmk_draw_sample and nnmk_draw_whiten ask of their arguments; *empty: nothing to launch
int dr_check_draws(int device, int dtype, const double *factor, int64_t ld_fac, const int32_t *status, int B, int Tmax, int sd, int Q, int K,
                   const void *src, int64_t ld_src, const void *mean, int64_t ld_mean, void *dst, int64_t ld_dst, const char *src_name,
                   bool dst_apart_from_src, bool *empty) {
  const char *who = "sample";
  *empty = true;
  if (int rc = check_dtype(who, dtype)) return rc;
  if (B < 0 || Tmax < 0 || sd < 0) return dr_refuse("sample: negative size (B = %lld, Tmax = %lld, sd = %lld)", B, Tmax, sd);
  if (K < 0) return dr_refuse("sample: negative number of draws K = %lld", K);
  if (Q < 0 || Q > 2) return dr_refuse("sample: the half-bandwidth Q = %lld must be in [0, 2] (window extents of at most 1)", Q);
  if (ld_fac < sd || ld_src < sd || ld_dst < sd || (mean && ld_mean < sd))
    return dr_refuse("sample: a row stride (ld_fac = %lld, the input's %lld, ld_mean = %lld, the output's %lld) is below sd", ld_fac, ld_src, ld_mean, ld_dst);
  if (!dr_stride_fits(Q + 1, B, Tmax, ld_fac)) return dr_refuse_stride("ld_fac", ld_fac);
  if (!dr_stride_fits(K, B, Tmax, ld_src)) return dr_refuse_stride(src_name, ld_src);
  if (mean && !dr_stride_fits(1, B, Tmax, ld_mean)) return dr_refuse_stride("ld_mean", ld_mean);
  if (!dr_stride_fits(K, B, Tmax, ld_dst)) return dr_refuse_stride("of the output", ld_dst);
  if (int rc = dr_check_grid(B, sd)) return rc;
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || Tmax == 0 || sd == 0 || K == 0) return 0;
  if (!factor || !status || !src || !dst) return dr_refuse("sample: NULL factor, status, input or output");
  const size_t esz = dtype == MLPG_HIP_F32 ? 4 : 8;
  const size_t nfac = dr_span((int64_t)(Q + 1) * B * Tmax, ld_fac, sd, 8), ndst = dr_span((int64_t)K * B * Tmax, ld_dst, sd, esz);
  if (dr_overlap(dst, ndst, factor, nfac)) return dr_refuse("sample: the output overlaps the factor planes");
  if (dst_apart_from_src && dr_overlap(dst, ndst, src, dr_span((int64_t)K * B * Tmax, ld_src, sd, esz)))
    return dr_refuse("sample: the output overlaps x (a frame's z needs the x of the two frames behind it)");
  *empty = false;
  return 0;
}

DrArgs dr_draw_args(const double *factor, int64_t ld_fac, const int32_t *status, const int32_t *lengths, int B, int Tmax, int sd, int Q, int K,
                    const void *src, int64_t ld_src, const void *mean, int64_t ld_mean, void *dst, int64_t ld_dst) {
  DrArgs a = {};
  a.lengths = lengths;
  a.B = B;
  a.Tmax = Tmax;
  a.sd = sd;
  a.ngrp = (sd + 63) / 64;
  a.fac_in = factor;
  a.ld_fac = (long)ld_fac;
  a.status_in = status;
  a.Q = Q;
  a.K = K;
  a.src = src;
  a.mean = mean;
  a.dst = dst;
  a.ld_src = (long)ld_src;
  a.ld_mean = (long)ld_mean;
  a.ld_dst = (long)ld_dst;
  return a;
}

template <typename K, typename... Args>
int dr_launch(K kern, hipStream_t st, unsigned blocks, int threads, Args... args) {
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, st, args...);
  MLPG_HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename TIN>
int launch_draw_factor(hipStream_t st, unsigned blocks, const DrArgs &a, const WinSet &ws) {
  if (ws.q == 0) return dr_launch(draw_factor_kernel<TIN, 0>, st, blocks, 64, a, ws);
  if (ws.q == 1) return dr_launch(draw_factor_kernel<TIN, 1>, st, blocks, 64, a, ws);
  return dr_launch(draw_factor_kernel<TIN, 2>, st, blocks, 64, a, ws);
}

template <typename TIN>
int launch_draw_sample(hipStream_t st, unsigned blocks, const DrArgs &a) {
  if (a.Q == 0) return dr_launch(draw_sample_kernel<TIN, 0>, st, blocks, 64, a);
  if (a.Q == 1) return dr_launch(draw_sample_kernel<TIN, 1>, st, blocks, 64, a);
  return dr_launch(draw_sample_kernel<TIN, 2>, st, blocks, 64, a);
}

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int nnmk_draw_abi_version(void) { return NNMK_DRAW_ABI_VERSION; }

__attribute__((visibility("default"))) int nnmk_draw_group(void) { return kDrawGroup; }

__attribute__((visibility("default"))) long long nnmk_draw_launch_count(void) { return g_draw_launches.load(std::memory_order_relaxed); }

__attribute__((visibility("default"))) int nnmk_draw_factor(int device, void *stream, int dtype, const void *variances, int var_mode,
                                                            int64_t ld_in, const int32_t *lengths, int B, int Tmax, int D, int sd,
                                                            int num_windows, const int32_t *win_l, const int32_t *win_u,
                                                            const double *win_coef, double *factor, int64_t ld_fac, double *logdet,
                                                            int32_t *status) {
  const char *who = "sample";
  WinSet ws;
  if (int rc = check_dtype(who, dtype)) return rc;
  if (var_mode < 0 || var_mode > 2) return dr_refuse("sample: unknown var_mode %lld", var_mode);
  if (B < 0 || Tmax < 0 || D < 0 || sd < 0) return dr_refuse("sample: negative size (B = %lld, Tmax = %lld, D = %lld, sd = %lld)", B, Tmax, D, sd);
  if (num_windows < 1 || num_windows > kMaxWindows || !win_l || !win_u || !win_coef)
    return dr_refuse("sample: num_windows must be in [1, %lld] and the window tables non-NULL", kMaxWindows);
  if ((int64_t)num_windows * sd != (int64_t)D) return dr_refuse("sample: D = %lld is not num_windows * sd = %lld * %lld", D, num_windows, sd);
  for (int w = 0; w < num_windows; ++w)
    if (win_l[w] < 0 || win_u[w] < 0 || win_l[w] > 1 || win_u[w] > 1)
      return dr_refuse("sample: window %lld: extents (l = %lld, u = %lld) must be 0 or 1", w, win_l[w], win_u[w]);
  if (var_mode == MLPG_HIP_VAR_FRAME && ld_in < D) return dr_refuse("sample: the row stride ld_in = %lld is below D = %lld", ld_in, D);
  if (!dr_stride_fits(1, B, Tmax, ld_in > D ? ld_in : D)) return dr_refuse_stride("ld_in", ld_in);
  if (int rc = dr_check_grid(B, sd)) return rc;
  if (pack_windows(num_windows, win_l, win_u, win_coef, &ws)) return dr_refuse("sample: bad window tables");
  if (ld_fac < sd) return dr_refuse("sample: the row stride ld_fac = %lld is below sd = %lld", ld_fac, sd);
  if (!dr_stride_fits(3 /* Q + 1 <= 3 planes */, B, Tmax, ld_fac)) return dr_refuse_stride("ld_fac", ld_fac);
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || Tmax == 0 || sd == 0) return 0;
  if (var_mode != MLPG_HIP_VAR_UNIT && !variances) return dr_refuse("sample: NULL variances");
  if (!factor || !logdet || !status) return dr_refuse("sample: NULL factor, logdet or status");
  const size_t esz = dtype == MLPG_HIP_F32 ? 4 : 8;
  const size_t nfac = dr_span((int64_t)(ws.q + 1) * B * Tmax, ld_fac, sd, 8);
  const size_t nvar = var_mode == MLPG_HIP_VAR_FRAME ? dr_span((int64_t)B * Tmax, ld_in, D, esz) : (size_t)D * esz;
  if (dr_overlap(factor, nfac, variances, nvar) || dr_overlap(factor, nfac, lengths, (size_t)B * 4))
    return dr_refuse("sample: the factor planes overlap an input");
  if (dr_overlap(factor, nfac, logdet, (size_t)B * sd * 8) || dr_overlap(factor, nfac, status, (size_t)B * sd * 4))
    return dr_refuse("sample: the factor planes overlap logdet or status");
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  DrArgs a = {};
  a.lengths = lengths;
  a.B = B;
  a.Tmax = Tmax;
  a.sd = sd;
  a.ngrp = (sd + 63) / 64;
  a.var = variances;
  a.var_mode = var_mode;
  a.ld_in = (long)ld_in;
  a.fac = factor;
  a.ld_fac = (long)ld_fac;
  a.logdet = logdet;
  a.status = status;
  const unsigned blocks = (unsigned)((int64_t)B * a.ngrp);
  const int rc = dtype == MLPG_HIP_F32 ? launch_draw_factor<float>((hipStream_t)stream, blocks, a, ws)
                                       : launch_draw_factor<double>((hipStream_t)stream, blocks, a, ws);
  if (rc == 0) g_draw_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

__attribute__((visibility("default"))) int nnmk_draw_sample(int device, void *stream, int dtype, const double *factor, int64_t ld_fac,
                                                            const int32_t *status, const int32_t *lengths, int B, int Tmax, int sd, int Q,
                                                            int K, const void *noise, int64_t ld_noise, const void *mean, int64_t ld_mean,
                                                            void *out, int64_t ld_out) {
  bool empty;
  if (int rc = dr_check_draws(device, dtype, factor, ld_fac, status, B, Tmax, sd, Q, K, noise, ld_noise, mean, ld_mean, out, ld_out, "ld_noise",
                              false, &empty))
    return rc;
  if (empty) return 0;
  DeviceGuard g("sample", device);
  if (g.rc) return g.rc;
  const DrArgs a = dr_draw_args(factor, ld_fac, status, lengths, B, Tmax, sd, Q, K, noise, ld_noise, mean, ld_mean, out, ld_out);
  const unsigned blocks = (unsigned)((int64_t)B * a.ngrp);
  const int rc = dtype == MLPG_HIP_F32 ? launch_draw_sample<float>((hipStream_t)stream, blocks, a)
                                       : launch_draw_sample<double>((hipStream_t)stream, blocks, a);
  if (rc == 0) g_draw_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

__attribute__((visibility("default"))) int nnmk_draw_whiten(int device, void *stream, int dtype, const double *factor, int64_t ld_fac,
                                                            const int32_t *status, const int32_t *lengths, int B, int Tmax, int sd, int Q,
                                                            int K, const void *x, int64_t ld_x, const void *mean, int64_t ld_mean, void *z,
                                                            int64_t ld_z) {
  bool empty;
  if (int rc = dr_check_draws(device, dtype, factor, ld_fac, status, B, Tmax, sd, Q, K, x, ld_x, mean, ld_mean, z, ld_z, "ld_x", true, &empty))
    return rc;
  if (empty) return 0;
  DeviceGuard g("sample", device);
  if (g.rc) return g.rc;
  const DrArgs a = dr_draw_args(factor, ld_fac, status, lengths, B, Tmax, sd, Q, K, x, ld_x, mean, ld_mean, z, ld_z);
  const unsigned blocks = (unsigned)((int64_t)B * a.ngrp);
  const int rc = dtype == MLPG_HIP_F32 ? dr_launch(draw_whiten_kernel<float>, (hipStream_t)stream, blocks, 256, a)
                                       : dr_launch(draw_whiten_kernel<double>, (hipStream_t)stream, blocks, 256, a);
  if (rc == 0) g_draw_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

}  // extern "C"
