// The variance gradient of ONE live element (b, t, d), every window of it: the body shared by var_grad_kernel (mlpg_vargrad.hip,
// dense rows) and streams_bwd_kernel (mlpg_streams_bwd.hip, column slices of wider rows).  The tests require the two kernels to agree
// bit for bit, so the formula, the zero rule of the edge mask and the order of reads exist here and nowhere else.
//
// For system (b, d) of length len, with tau_w = 1 / var (input dtype, edge-masked), y the trajectory and grad_mean the result of the
// backward solve:
//   grad_var[t, w*sd + d] = -grad_mean[t, w*sd + d] tau_w[t] (mu_w[t] - (W_w y)[t]),   float64 arithmetic.
// The caller has already dealt with the rows past the length and with failed systems (zeros), and maps threads to elements.
#pragma once
#include "common.h"

namespace mlpg {

// row:   index of element (b, t, window 0, d) in grad_mean, mean and grad_var; window w is wstride elements further on.
// vrow:  the same for var -- `row` for per-frame variances, the dim's column for global ones (the global-variance base).
// yb:    y at (b, frame 0, d); ldy: its row stride.
template <typename T>
__device__ __forceinline__ void var_grad_element(const T *__restrict__ grad_mean, const T *__restrict__ var, const T *__restrict__ mean,
                                                 const T *__restrict__ yb, size_t row, size_t vrow, size_t wstride, size_t ldy, int t,
                                                 int len, const WinSet &ws, T *__restrict__ grad_var) {
  // the y stencil, shared by every window; taps outside [0, len) are the truncation of W_w (and never read)
  int lmax = 0, umax = 0;
  for (int w = 0; w < ws.nw; ++w) {
    lmax = ws.l[w] > lmax ? ws.l[w] : lmax;
    umax = ws.u[w] > umax ? ws.u[w] : umax;
  }
  double ys[2 * kMaxExtent + 1];
#pragma unroll
  for (int k = -kMaxExtent; k <= kMaxExtent; ++k) {
    const int tt = t + k;
    ys[k + kMaxExtent] = (k >= -lmax && k <= umax && tt >= 0 && tt < len) ? (double)yb[(size_t)tt * ldy] : 0.0;
  }
  const T one = (T)1;
  for (int w = 0; w < ws.nw; ++w) {
    // the edge mask and the [-0:] rule BEFORE the variance is read: a masked entry may hold 0, a negative value or NaN
    const bool masked = w >= 1 && (ws.mw == 0 || t < ws.mw || t >= len - ws.mw);
    const size_t c = (size_t)w * wstride;
    double g = 0.0;
    if (!masked) {
      const double tau = (double)(one / var[vrow + c]);
      const double *cw = ws.c + ws.off[w];
      const int l = ws.l[w], u = ws.u[w];
      double wy = 0.0;
#pragma unroll
      for (int k = -kMaxExtent; k <= kMaxExtent; ++k)
        if (k >= -l && k <= u) wy += cw[l + k] * ys[k + kMaxExtent];
      const double r = (double)mean[row + c] - wy;
      g = -(double)grad_mean[row + c] * tau * r;
    }
    grad_var[row + c] = (T)g;
  }
}

}  // namespace mlpg
