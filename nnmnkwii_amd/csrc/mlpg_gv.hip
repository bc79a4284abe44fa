// K11: parameter generation with the likelihood of the trajectory's GV (the variance over time of each static dimension of one
// utterance; Toda, Black, Tokuda 2007, section IV) -- mlpg_hip_gv_ascent -- and the GV of a padded batch -- mlpg_hip_gv.
// tools/gvmlpg_model.py is the specification; DESIGN.md K11 has the contract and the measurements.
//
// Per system (utterance b, static dim d) with T live frames, P = sum_w W_w^T diag(tau_w) W_w (pentadiagonal: window extents <= 1),
// r = sum_w W_w^T diag(tau_w) mu_w, both assembled by assemble.h exactly as the natural-order forward kernel does:
//   L(y) = omega (-1/2 y^T P y + y^T r) - 1/2 p_v (v(y) - mu_v)^2,   omega = omega_scale / (2 T)
//   g(y) = omega (r - P y) - (2 / T) p_v (v(y) - mu_v) (y - m(y)),    y <- y + alpha g(y), n_iter times.
//
// ONE launch for all systems and all iterations: one 64-lane workgroup (one wavefront) per system.  Lane p owns the chunk of
// M = max(2, ceil(T / 64)) consecutive frames [p M, p M + M); its y, the three band columns of P and r live in LDS at
// [i * 64 + p] (conflict-free; 5 * 64 * M doubles: 38 KB at 900 frames, 80 KB at the 2048 the kernel reaches.  Registers would
// take the chunk length as a template parameter and 320 VGPRs at 2048 frames; one body with a runtime M in LDS serves every
// length).  After the assembly a lane touches its own LDS column only, so the iterations
// need no barrier: the two-frame halo of y comes from the neighbouring lanes by cross-lane moves at the top of every sweep, the
// halo of P once.  m and v are summed sequentially inside a chunk and then by one xor butterfly over the 64 lanes (every lane
// ends with the same bits).  Frames at or past T hold zeros, are never updated and are masked out of v.  No traffic between
// workgroups, no atomics: a system's bits depend on its own inputs alone.
// Compiled with -ffp-contract=off: the model rounds every product and sum separately.
#include <math.h>

#include "assemble.h"

namespace mlpg {

namespace {

constexpr int kGvMaxFrames = 2048;   // 64 lanes x 32 frames; 5 arrays of 2048 doubles = 80 KB of LDS
constexpr int kGvMaxIter = 100000;

struct GvArgs {
  const void *y_in;
  void *y_out;
  const double *gv_mean, *gv_prec;
  double omega_scale, step;
  int n_iter, init;
  double *report;
  int32_t *status;
};

__device__ __forceinline__ double wave_sum(double s) {
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return s;
}
__device__ __forceinline__ double wave_max(double s) {
  for (int m = 32; m >= 1; m >>= 1) s = __builtin_fmax(s, __shfl_xor(s, m));
  return s;
}

// One system's LDS image and the halo of P; chunk-local frame i of this lane is at [i * 64 + lane].
struct GvSys {
  double *Y, *Pd, *P1, *P2, *R;
  int M, T, lane;
  double ca, cb, cc;   // P[f0, f0 - 2], P[f0, f0 - 1], P[f0 + 1, f0 - 1] with f0 the chunk's first frame (0 on lane 0)

  __device__ __forceinline__ bool live(int i) const { return lane * M + i < T; }

  // One sweep over the chunk: f(i, y_t, (P y)_t, r_t, sum_j |P_tj|) for i = 0 .. M - 1.  f may write Y[i * 64 + lane]: the
  // neighbours' halo was fetched before the first call and the chunk's own later frames have not been written yet.
  template <typename F>
  __device__ __forceinline__ void sweep(F &&f) const {
    double ym2 = __shfl_up(Y[(M - 2) * 64 + lane], 1), ym1 = __shfl_up(Y[(M - 1) * 64 + lane], 1);
    double yp1 = __shfl_down(Y[lane], 1), yp2 = __shfl_down(Y[64 + lane], 1);
    if (lane == 0) ym2 = ym1 = 0.0;
    if (lane == 63) yp1 = yp2 = 0.0;
    double q2a = ca, q1 = cb, q2b = cc;   // P2 of frame t - 2, P1 of t - 1, P2 of t - 1
    double cur = Y[lane], nx1 = Y[64 + lane];
    for (int i = 0; i < M; ++i) {
      const double nx2 = i + 2 < M ? Y[(i + 2) * 64 + lane] : (i + 2 == M ? yp1 : yp2);
      const double pd = Pd[i * 64 + lane], p1 = P1[i * 64 + lane], p2 = P2[i * 64 + lane];
      double acc = pd * cur;
      acc += p1 * nx1;
      acc += p2 * nx2;
      acc += q1 * ym1;
      acc += q2a * ym2;
      const double rowsum = __builtin_fabs(pd) + __builtin_fabs(p1) + __builtin_fabs(p2) + __builtin_fabs(q1) + __builtin_fabs(q2a);
      f(i, cur, acc, R[i * 64 + lane], rowsum);
      ym2 = ym1;
      ym1 = cur;
      cur = nx1;
      nx1 = nx2;
      q2a = q2b;
      q2b = p2;
      q1 = p1;
    }
  }

  // m = (1/T) sum y, v = (1/T) sum (y - m)^2: two passes, chunk-sequential, then the butterfly
  __device__ __forceinline__ void mean_var(double &m, double &v) const {
    double s = 0.0;
    for (int i = 0; i < M; ++i) s += Y[i * 64 + lane];   // frames past T hold 0
    m = wave_sum(s) / (double)T;
    double q = 0.0;
    for (int i = 0; i < M; ++i)
      if (live(i)) {
        const double e = Y[i * 64 + lane] - m;
        q += e * e;
      }
    v = wave_sum(q) / (double)T;
  }

  // L(y) with v = v(y) given; G = max_t sum_j |P_tj| on the way
  __device__ __forceinline__ double objective(double omega, double pv, double muv, double v, double &G) const {
    double q = 0.0, g = 0.0;
    sweep([&](int i, double y, double py, double r, double rowsum) {
      if (live(i)) {
        q += y * (r - 0.5 * py);
        g = __builtin_fmax(g, rowsum);
      }
    });
    G = wave_max(g);
    const double dv = v - muv;
    return omega * wave_sum(q) - 0.5 * pv * (dv * dv);
  }
};

template <typename TIN>
__global__ __launch_bounds__(64) void gv_ascent_kernel(Problem p, WinSet ws, GvArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)p.sd), d = (int)(blockIdx.x - (unsigned)b * (unsigned)p.sd);
  int T = p.Tmax;
  if (p.lengths) {
    T = p.lengths[b];
    T = T < 0 ? 0 : (T > p.Tmax ? p.Tmax : T);
  }
  const TIN *yi = (const TIN *)a.y_in + (size_t)b * p.Tmax * p.sd + d;
  TIN *yo = (TIN *)a.y_out + (size_t)b * p.Tmax * p.sd + d;
  for (int t = T + lane; t < p.Tmax; t += 64) yo[(size_t)t * p.sd] = (TIN)0;   // pad frames (never read, also in place)
  double *rep = a.report + (size_t)blockIdx.x * 4;
  if (T == 0) {
    if (lane == 0) {
      rep[0] = rep[1] = rep[2] = rep[3] = 0.0;
      a.status[blockIdx.x] = 0;
    }
    return;
  }

  GvSys s;
  s.M = (T + 63) / 64 < 2 ? 2 : (T + 63) / 64;
  s.T = T;
  s.lane = lane;
  const int n = 64 * s.M;
  s.Y = lds;
  s.Pd = lds + n;
  s.P1 = lds + 2 * n;
  s.P2 = lds + 3 * n;
  s.R = lds + 4 * n;
  // assembly with consecutive lanes on consecutive frames; frame f lands in the chunk layout at [(f % M) * 64 + f / M]
  const SysView<TIN, false> view = make_view<TIN, false>(p, ws, b, d, T);
  for (int i = 0; i < s.M; ++i) {
    const int f = i * 64 + lane;
    double pk[3] = {0.0, 0.0, 0.0}, rhs = 0.0, y0 = 0.0;
    if (f < T) {
      assemble_frame<2, TIN, false>(view, ws, f, pk, rhs);
      y0 = (double)yi[(size_t)f * p.sd];
    }
    const int at = (f % s.M) * 64 + f / s.M;
    s.Y[at] = y0;
    s.Pd[at] = pk[0];
    s.P1[at] = pk[1];
    s.P2[at] = pk[2];
    s.R[at] = rhs;
  }
  __syncthreads();
  s.ca = __shfl_up(s.P2[(s.M - 2) * 64 + lane], 1);
  s.cb = __shfl_up(s.P1[(s.M - 1) * 64 + lane], 1);
  s.cc = __shfl_up(s.P2[(s.M - 1) * 64 + lane], 1);
  if (lane == 0) s.ca = s.cb = s.cc = 0.0;

  const double Td = (double)T;
  const double omega = a.omega_scale / (2.0 * Td);
  const double muv = a.gv_mean[d], pv = a.gv_prec[d];
  double m, v;
  s.mean_var(m, v);
  const double v0 = v;
  if (a.init == 1 && v0 > 0.0 && muv > 0.0) {   // the scaled start: the GV of the start is mu_v
    const double sc = sqrt(muv / v0);
    for (int i = 0; i < s.M; ++i)
      if (s.live(i)) s.Y[i * 64 + lane] = m + sc * (s.Y[i * 64 + lane] - m);
    s.mean_var(m, v);
  }
  double G;
  const double L0 = s.objective(omega, pv, muv, v, G);
  double alpha = a.step;
  if (!(alpha > 0.0)) {
    const double dv = __builtin_fabs(v - muv);
    alpha = 1.0 / (omega * G + 2.0 / Td * pv * (dv + 2.0 * __builtin_fmax(v, muv)));
  }
  for (int it = 0; it < a.n_iter; ++it) {
    const double c = 2.0 / Td * pv * (v - muv);
    double sum = 0.0;
    s.sweep([&](int i, double y, double py, double r, double) {
      if (s.live(i)) {
        const double g = omega * (r - py) - c * (y - m);
        const double yn = y + alpha * g;
        s.Y[i * 64 + lane] = yn;
        sum += yn;
      }
    });
    m = wave_sum(sum) / Td;
    double q = 0.0;
    for (int i = 0; i < s.M; ++i)
      if (s.live(i)) {
        const double e = s.Y[i * 64 + lane] - m;
        q += e * e;
      }
    v = wave_sum(q) / Td;
  }
  const double L1 = a.n_iter > 0 ? s.objective(omega, pv, muv, v, G) : L0;
  if (lane == 0) {
    rep[0] = L0;
    rep[1] = L1;
    rep[2] = v0;
    rep[3] = v;
    int st = 0;
    const double big = __builtin_fmax(__builtin_fabs(L0), __builtin_fabs(L1));
    if (!(big < INFINITY) || !(__builtin_fabs(v) < INFINITY)) st = 1;   // NaN compares false
    else if (L1 < L0 - 0x1p-40 * big) st = 2;
    a.status[blockIdx.x] = st;
  }
  __syncthreads();
  for (int i = 0; i < s.M; ++i) {
    const int f = i * 64 + lane;
    if (f < T) yo[(size_t)f * p.sd] = (TIN)s.Y[(f % s.M) * 64 + f / s.M];
  }
}

// GV of every (b, d) of a padded batch: one thread per system, two sequential passes over the live frames
template <typename TIN>
__global__ __launch_bounds__(256) void gv_kernel(const TIN *__restrict__ x, long ld_x, const int32_t *__restrict__ lengths, int B,
                                                 int Tmax, int D, double *__restrict__ out) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= (long)B * D) return;
  const int b = (int)(k / D), d = (int)(k - (long)b * D);
  int T = Tmax;
  if (lengths) {
    T = lengths[b];
    T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
  }
  double v = 0.0;
  if (T > 0) {
    const TIN *col = x + (size_t)b * Tmax * ld_x + d;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += (double)col[(size_t)t * ld_x];
    const double m = s / (double)T;
    double q = 0.0;
    for (int t = 0; t < T; ++t) {
      const double e = (double)col[(size_t)t * ld_x] - m;
      q += e * e;
    }
    v = q / (double)T;
  }
  out[k] = v;
}

template <typename TIN>
int launch_gv_ascent_t(hipStream_t st, const Problem &p, const WinSet &ws, const GvArgs &a) {
  const int Mmax = (p.Tmax + 63) / 64 < 2 ? 2 : (p.Tmax + 63) / 64;
  const size_t lds_bytes = sizeof(double) * 5 * 64 * (size_t)Mmax;
  MLPG_HIP_CHECK(hipFuncSetAttribute((const void *)gv_ascent_kernel<TIN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(sizeof(double) * 5 * kGvMaxFrames)));
  hipLaunchKernelGGL(gv_ascent_kernel<TIN>, dim3((unsigned)(p.B * p.sd)), dim3(64), lds_bytes, st, p, ws, a);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountGvAscent);
  return 0;
}

}  // namespace

}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int mlpg_hip_gv_max_frames(void) { return kGvMaxFrames; }

__attribute__((visibility("default"))) int mlpg_hip_gv_ascent(int device, void *stream, int dtype, const void *mean, const void *var,
                                                              int var_mode, const int32_t *lengths, int B, int Tmax, int D,
                                                              int num_windows, const int32_t *win_l_h, const int32_t *win_u_h,
                                                              const double *win_coef_h, const void *y_in, void *y_out,
                                                              const double *gv_mean, const double *gv_prec, double omega_scale,
                                                              int n_iter, double step, int init, double *report, int32_t *status) {
  const char *who = "gv_ascent";
  if (B < 0 || Tmax < 0 || D < 0 || (int64_t)B * D > 67108863LL /* 2^26 - 1 workgroups of 64 threads (D >= sd): a grid is 32 bits of threads */) {
    set_error("%s: bad batch shape (B = %d, Tmax = %d, D = %d)", who, B, Tmax, D);
    return MLPG_HIP_EINVAL;
  }
  if (num_windows < 1 || num_windows > kMaxWindows || !win_l_h || !win_u_h || !win_coef_h) {
    set_error("%s: num_windows must be in [1, %d] and the window tables non-NULL", who, kMaxWindows);
    return MLPG_HIP_EINVAL;
  }
  if (D % num_windows != 0) {
    set_error("%s: D = %d is not a multiple of num_windows = %d", who, D, num_windows);
    return MLPG_HIP_EINVAL;
  }
  for (int w = 0; w < num_windows; ++w)
    if (win_l_h[w] < 0 || win_u_h[w] < 0 || win_l_h[w] > 1 || win_u_h[w] > 1) {
      set_error("%s: window %d: extents (l = %d, u = %d) must be 0 or 1", who, w, win_l_h[w], win_u_h[w]);
      return MLPG_HIP_EINVAL;
    }
  if (int rc = check_dtype(who, dtype)) return rc;
  if (int rc = check_var(who, var_mode, var)) return rc;
  if (n_iter < 0 || n_iter > kGvMaxIter) {
    set_error("%s: n_iter must be in [0, %d] (got %d)", who, kGvMaxIter, n_iter);
    return MLPG_HIP_EINVAL;
  }
  if (init != 0 && init != 1) {
    set_error("%s: init must be 0 (the given trajectory) or 1 (scaled to the mean gv), got %d", who, init);
    return MLPG_HIP_EINVAL;
  }
  if (!(omega_scale > 0.0) || !(omega_scale < INFINITY) || step != step || !(step < INFINITY)) {
    set_error("%s: omega_scale must be positive and finite, step finite (a step <= 0 asks for the derived one)", who);
    return MLPG_HIP_EINVAL;
  }
  if (Tmax > kGvMaxFrames) {
    set_error("%s: takes at most %d frames per utterance (Tmax = %d)", who, kGvMaxFrames, Tmax);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || Tmax == 0 || D == 0) return 0;
  if (!mean || !y_in || !y_out || !gv_mean || !gv_prec || !report || !status) {
    set_error("%s: NULL data pointer (mean, y_in, y_out, gv_mean, gv_prec, report and status are required)", who);
    return MLPG_HIP_EINVAL;
  }
  WinSet ws;
  if (int rc = pack_windows(num_windows, win_l_h, win_u_h, win_coef_h, &ws)) return rc;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  const Problem p = dense_problem(mean, var, nullptr, lengths, y_out, status, false, var_mode, B, Tmax, D, D / num_windows);
  const GvArgs a = {y_in, y_out, gv_mean, gv_prec, omega_scale, step, n_iter, init, report, status};
  return dtype == MLPG_HIP_F32 ? launch_gv_ascent_t<float>((hipStream_t)stream, p, ws, a)
                               : launch_gv_ascent_t<double>((hipStream_t)stream, p, ws, a);
}

__attribute__((visibility("default"))) int mlpg_hip_gv(int device, void *stream, int dtype, const void *x, int64_t ld_x,
                                                       const int32_t *lengths, int B, int Tmax, int D, double *out) {
  const char *who = "gv";
  if (B < 0 || Tmax < 0 || D < 0 || (int64_t)B * D > 16777215LL * 256 /* 2^24 - 1 workgroups of 256 threads: a grid is 32 bits of threads, a larger one runs truncated and reports nothing */) {
    set_error("%s: bad batch shape (B = %d, Tmax = %d, D = %d)", who, B, Tmax, D);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_dtype(who, dtype)) return rc;
  if (ld_x < D) {
    set_error("%s: the row stride must be at least D = %d (got %lld)", who, D, (long long)ld_x);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || D == 0) return 0;
  if (!out || (Tmax > 0 && !x)) {
    set_error("%s: NULL data pointer (x and out are required)", who);
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  const unsigned blocks = (unsigned)(((int64_t)B * D + 255) / 256);
  if (dtype == MLPG_HIP_F32)
    hipLaunchKernelGGL(gv_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float *)x, (long)ld_x, lengths, B, Tmax,
                       D, out);
  else
    hipLaunchKernelGGL(gv_kernel<double>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const double *)x, (long)ld_x, lengths, B,
                       Tmax, D, out);
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountGv);
  return 0;
}

}  // extern "C"
