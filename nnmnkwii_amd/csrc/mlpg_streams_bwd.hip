// Epilogue of mlpg_hip_backward_streams: the variance gradient of every stream of a multi-stream batch, in place, and the
// backward pass of its pass-through streams.
//
// The parent arrays are (B, Tmax, ld_in) [mean, var, grad_mean, grad_var] and (B, Tmax, ld_out) [y, grad_out]; a ColTable
// passed BY VALUE (kernarg segment, as WinSet is) lists the member streams of one launch: their static dims side by side on
// a merged index j in [0, total), member m owning j in [begin[m], begin[m] + sd[m]).  One thread per (b, t, j), j fastest:
//  * dynamic members (all of one window list): var_grad_element (vargrad_element.h), the very body of var_grad_kernel
//    (mlpg_vargrad.hip), on strided rows --
//      grad_var[t, in_col + w*sd + d] = -grad_mean[..] tau_w[t] (mu_w[t] - (W_w y)[t]),  float64 arithmetic,
//    0 at and past the length, 0 in every column of a system whose status is non-zero, 0 where the edge mask removes the
//    precision, the mask test BEFORE the variance is read;
//  * pass-through members (no windows): grad_mean = grad_out on live rows and 0 on padding, grad_var = 0, status = 0.
// Thread-to-column mapping: with j fastest, the lanes of a wavefront that belong to one member read, per window, sd
// consecutive elements of a row (mgc at config 5: 60 float64 = 480 contiguous bytes out of a 1584-byte row, three such runs per
// row and array) and the y stencil as the same runs of the (narrower) output rows; the members of a Merlin row (60 + 1 + 5
// dims) share a wavefront, so the 1- and 5-dim streams cost no wavefronts of their own.  The other mapping -- one thread per
// input column -- would make every run a whole row, but evaluates the y stencil once per window instead of once per dim (three
// times the stencil loads and three times the threads).  Either way every row is requested once per array; whether the kernel then
// runs at the rate of HBM is a matter of measurement.
#include "common.h"
#include "vargrad_element.h"

namespace mlpg {
namespace {

template <typename T, int MODE>  // MODE: MLPG_HIP_VAR_FRAME, MLPG_HIP_VAR_GLOBAL, or kPass
__global__ void __launch_bounds__(256) streams_bwd_kernel(const T *__restrict__ grad_out, const T *__restrict__ var,
                                                          const T *__restrict__ mean, const T *__restrict__ y,
                                                          const int32_t *__restrict__ lengths, int32_t *__restrict__ status,
                                                          int B, int Tmax, long ld_in, long ld_out, int ld_status, ColTable ct,
                                                          WinSet ws, T *__restrict__ grad_mean, T *__restrict__ grad_var) {
  constexpr bool PASS = MODE == kStreamsBwdPass;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * Tmax * ct.total;
  if (e >= total) return;
  const int j = (int)(e % ct.total);
  const long bt = e / ct.total;
  const int t = (int)(bt % Tmax), b = (int)(bt / Tmax);
  // the member that owns j: the last one with begin <= j (begin[] ascends; at most 64 entries)
  int lo = 0, hi = ct.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ct.begin[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  const int d = j - ct.begin[lo], sd = ct.sd[lo];
  const int sc = ct.stat_col[lo] + d;
  int len = lengths ? lengths[b] : Tmax;
  len = len < 0 ? 0 : (len > Tmax ? Tmax : len);
  const size_t row = (size_t)bt * ld_in + ct.in_col[lo] + d;  // element (b, t, window 0, d) of the (B, Tmax, ld_in) arrays
  const size_t orow = (size_t)ct.out_col[lo] + d;             // the dim's column of the (B, Tmax, ld_out) arrays
  if (PASS) {
    grad_mean[row] = t < len ? grad_out[(size_t)bt * ld_out + orow] : (T)0;
    if (grad_var) grad_var[row] = (T)0;
    if (t == 0 && status) status[(size_t)b * ld_status + sc] = 0;  // pass-through streams cannot fail
    return;
  }
  T *gv = grad_var + row;
  if (t >= len || status[(size_t)b * ld_status + sc] != 0) {
    for (int w = 0; w < ws.nw; ++w) gv[(size_t)w * sd] = (T)0;
    return;
  }
  var_grad_element<T>(grad_mean, var, mean, y + (size_t)b * Tmax * ld_out + orow, row,
                      MODE == MLPG_HIP_VAR_GLOBAL ? (size_t)ct.in_col[lo] + d : row, (size_t)sd, (size_t)ld_out, t, len, ws, grad_var);
}

template <typename T, int MODE>
void launch_t(hipStream_t st, unsigned grid, const void *grad_out, const void *var, const void *mean, const void *y,
              const int32_t *lengths, int32_t *status, int B, int Tmax, long ld_in, long ld_out, int ld_status,
              const ColTable &ct, const WinSet &ws, void *grad_mean, void *grad_var) {
  hipLaunchKernelGGL((streams_bwd_kernel<T, MODE>), dim3(grid), dim3(256), 0, st, (const T *)grad_out, (const T *)var,
                     (const T *)mean, (const T *)y, lengths, status, B, Tmax, ld_in, ld_out, ld_status, ct, ws, (T *)grad_mean,
                     (T *)grad_var);
}

}  // namespace

bool streams_bwd_fits(int B, int Tmax, int total) {
  return ((long)B * Tmax * total + 255) / 256 <= 16777215L;  // 2^24 - 1 workgroups of 256 threads: a grid is 32 bits of threads, a larger one runs truncated and reports nothing
}

int launch_streams_bwd(hipStream_t st, int dtype, int mode, const void *grad_out, const void *var, const void *mean,
                       const void *y, const int32_t *lengths, int32_t *status, int B, int Tmax, long ld_in, long ld_out,
                       int ld_status, const ColTable &ct, const WinSet &ws, void *grad_mean, void *grad_var) {
  const long total = (long)B * Tmax * ct.total;
  if (total == 0) return 0;
  if (!streams_bwd_fits(B, Tmax, ct.total)) {
    set_error("backward_streams: batch too large");
    return MLPG_HIP_EINVAL;
  }
  const unsigned grid = (unsigned)((total + 255) / 256);
#define MLPG_SB_LAUNCH(T, MODE) \
  launch_t<T, MODE>(st, grid, grad_out, var, mean, y, lengths, status, B, Tmax, ld_in, ld_out, ld_status, ct, ws, grad_mean, grad_var)
  if (dtype == MLPG_HIP_F32) {
    if (mode == kStreamsBwdPass) MLPG_SB_LAUNCH(float, kStreamsBwdPass);
    else if (mode == MLPG_HIP_VAR_GLOBAL) MLPG_SB_LAUNCH(float, MLPG_HIP_VAR_GLOBAL);
    else MLPG_SB_LAUNCH(float, MLPG_HIP_VAR_FRAME);
  } else {
    if (mode == kStreamsBwdPass) MLPG_SB_LAUNCH(double, kStreamsBwdPass);
    else if (mode == MLPG_HIP_VAR_GLOBAL) MLPG_SB_LAUNCH(double, MLPG_HIP_VAR_GLOBAL);
    else MLPG_SB_LAUNCH(double, MLPG_HIP_VAR_FRAME);
  }
#undef MLPG_SB_LAUNCH
  MLPG_HIP_CHECK(hipGetLastError());
  note_launch(kCountStreamsBwd);
  return 0;
}

}  // namespace mlpg
