// Gradient of MLPG w.r.t. the variances (mlpg_hip_backward_var): the epilogue that runs behind the backward solve.
//
// For system (b, d) of length L, with tau_w = 1 / var (input dtype, edge-masked), y the trajectory and z = P^-1 g the
// solve mlpg_hip_backward already performs (grad_mean[t, w*sd+d] = tau_w[t] (W_w z)[t]):
//   grad_var[t, w*sd+d] = -tau_w[t]^2 (W_w z)[t] (mu_w[t] - (W_w y)[t]) = -grad_mean[t, w*sd+d] tau_w[t] (mu_w[t] - (W_w y)[t])
// One thread per (b, t, d) handles every window (var_grad_element, vargrad_element.h: the body this kernel shares with the
// stream-table epilogue): it reads the y stencil y[t - lmax .. t + umax] once (truncated at 0 and L, so the padding of y is never
// read), then per window grad_mean, mean and -- only where the edge mask leaves the precision alive -- var.  Adjacent lanes are
// adjacent (t, d) of the flattened (B, Tmax, sd) index, as in delta_kernel: rows are read
// contiguously and narrow streams (sd = 1, 5) still fill the wavefront.  float64 arithmetic throughout.
#include "common.h"
#include "vargrad_element.h"

namespace mlpg {
namespace {

template <typename T, bool GLOBAL>
__global__ void __launch_bounds__(256) var_grad_kernel(const T *__restrict__ grad_mean, const T *__restrict__ var,
                                                       const T *__restrict__ mean, const T *__restrict__ y,
                                                       const int32_t *__restrict__ lengths, const int32_t *__restrict__ status,
                                                       int B, int Tmax, int sd, WinSet ws, T *__restrict__ grad_var) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * Tmax * sd;
  if (e >= total) return;
  const int d = (int)(e % sd);
  const long bt = e / sd;
  const int t = (int)(bt % Tmax), b = (int)(bt / Tmax);
  int len = lengths ? lengths[b] : Tmax;
  len = len < 0 ? 0 : (len > Tmax ? Tmax : len);
  const size_t D = (size_t)ws.nw * sd;
  const size_t row = (size_t)bt * D + d;  // element (b, t, d) of window 0
  T *gv = grad_var + row;
  if (t >= len || status[(size_t)b * sd + d] != 0) {
    for (int w = 0; w < ws.nw; ++w) gv[(size_t)w * sd] = (T)0;
    return;
  }
  var_grad_element<T>(grad_mean, var, mean, y + (size_t)b * Tmax * sd + d, row, GLOBAL ? (size_t)d : row, (size_t)sd, (size_t)sd, t, len, ws,
                      grad_var);
}

template <typename T, bool GLOBAL>
void launch_t(hipStream_t st, unsigned grid, const void *grad_mean, const void *var, const void *mean, const void *y,
              const int32_t *lengths, const int32_t *status, int B, int Tmax, int sd, const WinSet &w, void *grad_var) {
  hipLaunchKernelGGL((var_grad_kernel<T, GLOBAL>), dim3(grid), dim3(256), 0, st, (const T *)grad_mean, (const T *)var,
                     (const T *)mean, (const T *)y, lengths, status, B, Tmax, sd, w, (T *)grad_var);
}

}  // namespace

int launch_var_grad(hipStream_t st, int dtype, const void *grad_mean, const void *var, int var_mode, const void *mean,
                    const void *y, const int32_t *lengths, const int32_t *status, int B, int Tmax, int sd, const WinSet &w,
                    void *grad_var) {
  const long total = (long)B * Tmax * sd;
  if (total == 0) return 0;
  const long blocks = (total + 255) / 256;
  if (blocks > 16777215L /* 2^24 - 1 workgroups of 256 threads: a grid is 32 bits of threads, a larger one runs truncated and reports nothing */) {
    set_error("backward_var: batch too large");
    return MLPG_HIP_EINVAL;
  }
  const unsigned grid = (unsigned)blocks;
  const bool global = var_mode == MLPG_HIP_VAR_GLOBAL;
  if (dtype == MLPG_HIP_F32) {
    if (global) launch_t<float, true>(st, grid, grad_mean, var, mean, y, lengths, status, B, Tmax, sd, w, grad_var);
    else launch_t<float, false>(st, grid, grad_mean, var, mean, y, lengths, status, B, Tmax, sd, w, grad_var);
  } else {
    if (global) launch_t<double, true>(st, grid, grad_mean, var, mean, y, lengths, status, B, Tmax, sd, w, grad_var);
    else launch_t<double, false>(st, grid, grad_mean, var, mean, y, lengths, status, B, Tmax, sd, w, grad_var);
  }
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountVarGrad);
  return 0;
}

}  // namespace mlpg
