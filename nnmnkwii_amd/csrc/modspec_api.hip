// C-ABI entry points of the modulation spectrum over padded minibatches (declared in include/mlpg_hip.h): mlpg_hip_modspec_batch,
// _batch_backward, _loss_form, _loss_workspace_bytes, _loss_step.  The reference takes one (T, D) array per call
// (autograd/_impl/modspec.py:9-72, preprocessing/modspec.py:6-53); these take (B, Tmax, D) float32 / float64 with an optional
// int32 lengths[B].  Every argument is checked before a device is selected or anything is launched.
#include <math.h>

#include "common.h"

using namespace mlpg;

namespace {

// what the three launching entries share: 0 go on, 1 an empty batch (return 0), < 0 refused
int check_batch(const char *who, int device, int dtype, int B, int Tmax, int D, int n) {
  if (int rc = check_dtype(who, dtype)) return rc;
  if (B < 0 || Tmax < 0 || D < 0) {
    set_error("%s: negative size (B=%d, Tmax=%d, D=%d)", who, B, Tmax, D);
    return MLPG_HIP_EINVAL;
  }
  if (n < 2) {
    set_error("%s: the DFT length must be at least 2 (got %d)", who, n);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  if (B == 0 || D == 0) return 1;
  if ((double)B * (double)((D + 1) / 2) > 2147483647.0) {
    set_error("%s: B * ceil(D / 2) = %d * %d workgroups are more than one launch takes", who, B, (D + 1) / 2);
    return MLPG_HIP_EINVAL;
  }
  return 0;
}

bool fft_route(int n) { return modspec_fft_takes(n) && !modspec_direct(); }

int check_direct_batch(const char *who, int B, int n) {
  if (B <= 65535) return 0;
  set_error("%s: more than 65535 sequences per call with DFT length %d, which takes the direct transform", who, n);
  return MLPG_HIP_EINVAL;
}

size_t loss_workspace_bytes(int B, int D) {
  const size_t bytes = sizeof(double) * (size_t)B * (size_t)((D + 1) / 2);
  return (bytes + 255) / 256 * 256 + 256;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int mlpg_hip_modspec_batch(int device, void *stream, int dtype, const void *x,
                                                                  const int32_t *lengths, int B, int Tmax, int D, int n, int ortho,
                                                                  void *ms) {
  const char *who = "modspec_batch";
  if (int rc = check_batch(who, device, dtype, B, Tmax, D, n)) return rc < 0 ? rc : 0;
  if ((!x && Tmax > 0) || !ms) {
    set_error("%s: NULL data pointer (x and ms are required)", who);
    return MLPG_HIP_EINVAL;
  }
  const bool fft = fft_route(n);
  if (!fft)
    if (int rc = check_direct_batch(who, B, n)) return rc;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  if (fft)
    return launch_modspec_batch((hipStream_t)stream, 0, dtype, x, nullptr, lengths, ms, B, Tmax, D, n, ortho, 0, 0.0, 1.0, nullptr,
                                nullptr);
  return launch_modspec_dft_batch((hipStream_t)stream, device, 0, dtype, x, nullptr, lengths, ms, B, Tmax, D, n, ortho);
}

__attribute__((visibility("default"))) int mlpg_hip_modspec_batch_backward(int device, void *stream, int dtype, const void *x,
                                                                           const void *grad_ms, const int32_t *lengths, int B,
                                                                           int Tmax, int D, int n, int ortho, void *grad_x) {
  const char *who = "modspec_batch_backward";
  if (int rc = check_batch(who, device, dtype, B, Tmax, D, n)) return rc < 0 ? rc : 0;
  if (Tmax == 0) return 0;  // no row of grad_x to write
  if (!x || !grad_ms || !grad_x) {
    set_error("%s: NULL data pointer (x, grad_ms and grad_x are required)", who);
    return MLPG_HIP_EINVAL;
  }
  const bool fft = fft_route(n);
  if (!fft)
    if (int rc = check_direct_batch(who, B, n)) return rc;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  if (fft)
    return launch_modspec_batch((hipStream_t)stream, 1, dtype, x, grad_ms, lengths, grad_x, B, Tmax, D, n, ortho, 0, 0.0, 1.0,
                                nullptr, nullptr);
  return launch_modspec_dft_batch((hipStream_t)stream, device, 1, dtype, x, grad_ms, lengths, grad_x, B, Tmax, D, n, ortho);
}

__attribute__((visibility("default"))) int mlpg_hip_modspec_loss_form(int n) { return fft_route(n) ? 1 : 0; }

__attribute__((visibility("default"))) size_t mlpg_hip_modspec_loss_workspace_bytes(int B, int D) {
  if (B < 0 || D < 0) return 0;
  return loss_workspace_bytes(B, D);
}

__attribute__((visibility("default"))) int mlpg_hip_modspec_loss_step(int device, void *stream, int dtype, const void *x,
                                                                      const void *target_ms, const int32_t *lengths, int B,
                                                                      int Tmax, int D, int n, int ortho, int log_domain, double eps,
                                                                      double n_elems, void *grad_x, double *loss, void *workspace,
                                                                      size_t workspace_bytes) {
  const char *who = "modspec_loss_step";
  const int rc0 = check_batch(who, device, dtype, B, Tmax, D, n);
  if (rc0 < 0) return rc0;
  if (!(eps >= 0.0) || !isfinite(eps)) {
    set_error("%s: eps must be finite and not negative (got %g)", who, eps);
    return MLPG_HIP_EINVAL;
  }
  if (!(n_elems > 0.0) || !isfinite(n_elems)) {
    set_error("%s: n_elems must be a positive finite number (got %g)", who, n_elems);
    return MLPG_HIP_EINVAL;
  }
  if (rc0 == 1) return 0;
  if (!fft_route(n)) {
    set_error("%s: the fused step takes a power of two in [2, 4096] on the FFT route (n=%d, mlpg_hip_modspec_loss_form answers 0): "
              "compose mlpg_hip_modspec_batch and mlpg_hip_modspec_batch_backward", who, n);
    return MLPG_HIP_EINVAL;
  }
  if ((!x && Tmax > 0) || !target_ms || (!grad_x && Tmax > 0) || !loss) {
    set_error("%s: NULL data pointer (x, target_ms, grad_x and loss are required)", who);
    return MLPG_HIP_EINVAL;
  }
  if (!workspace || workspace_bytes < loss_workspace_bytes(B, D) || ((uintptr_t)workspace & 7)) {
    set_error("%s: workspace of %zu bytes (8-byte aligned) needed, see mlpg_hip_modspec_loss_workspace_bytes", who,
              loss_workspace_bytes(B, D));
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_modspec_batch((hipStream_t)stream, 2, dtype, x, target_ms, lengths, grad_x, B, Tmax, D, n, ortho, log_domain != 0, eps,
                              n_elems, (double *)workspace, loss);
}

}  // extern "C"
