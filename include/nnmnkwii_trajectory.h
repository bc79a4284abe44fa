/* The other half of MLPG's trajectory distribution N(c; cbar, R^-1) over padded batches: the band of the covariance R^-1, log det R,
 * and the trajectory likelihood with its gradients -- an extension header of libmlpg_hip.so with its own prefix and version.
 * include/mlpg_hip.h, its ABI version, its export list, the kinds of mlpg_hip_launch_count and the other extension headers are
 * not touched by it; errors are read with mlpg_hip_last_error().  Plain C99.  DESIGN.md K19; csrc/mlpg_trajcov.hip;
 * tools/trajcov_model.py is the executable specification.
 *
 * The dtype codes (MLPG_HIP_F32 | MLPG_HIP_F64) and the variance modes (MLPG_HIP_VAR_FRAME | _GLOBAL | _UNIT) are those of
 * mlpg_hip.h; the three window tables (host memory: extents l[], u[] and the packed coefficients) are passed as the mlpg_hip_*
 * device entries take them. */
#ifndef NNMNKWII_TRAJECTORY_H
#define NNMNKWII_TRAJECTORY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNMK_TRAJ_ABI_VERSION 1

/* One system is (utterance b, static dim d) with T = lengths[b] live frames (clamped to [0, Tmax]; lengths NULL: Tmax each).
 *   tau_w[t]  the reciprocal of the variance in the input dtype, 0 on the first and last mw frames of every window but the
 *             first (mw: the largest window extent), 1 for unit variances: what every MLPG kernel of the library uses.
 *   R         sum_w W_w^T diag(tau_w) W_w, T x T, half-bandwidth Q = max_w (l_w + u_w): the matrix the forward kernels solve with.
 *   S         R^-1; the BAND is S_k[t] = S[t, t + k], k = 0 .. Q, zero where t + k >= T.  S_0 is the posterior variance.
 *   logdet    log det R = sum_t log D_t of R = L D L^T.
 * Window extents of at most 1 (Q <= 2).
 *
 * variances: device (B, Tmax, D) with row stride ld_in >= D in elements (utterance stride Tmax * ld_in), or (D), or NULL, by
 * var_mode; D = num_windows * sd, window-major columns.  A (D) or NULL variance is read in place: nothing is broadcast.
 * The band is PLANAR: device float64 (Q + 1, B, Tmax, sd), plane k's rows with stride ld_band >= sd in elements (utterance
 * stride Tmax * ld_band, plane stride B * Tmax * ld_band).  logdet: device float64 (B, sd), status: device int32 (B, sd), dense.
 *
 * Every launch goes on the caller's `stream`; no entry synchronises, allocates or puts work on another stream.  All return 0,
 * or -1 with the text "trajectory: ..." (nothing was launched, the runtime was not touched, the counter did not move), or -2
 * (runtime error).  Refused with -1: an unknown dtype or var_mode, a negative size, D != num_windows * sd, bad window tables,
 * a window extent above 1, a row stride below the width or so large that the batch's last row lies past 2^62 bytes, a batch
 * too large for one grid (B * ceil(sd / 64) above 2^24 - 1 workgroups), NULL for an array that has elements, and -- by
 * nnmk_traj_covariance, which keeps the factor in them while it reads -- band planes whose bytes overlap the variances, the
 * lengths, logdet or status.
 * B = 0, Tmax = 0 and sd = 0 return 0 and launch nothing (their other arguments are still checked).  All offsets are 64-bit. */

/* 1 */
int nnmk_traj_abi_version(void);

/* Factor, log-determinant and selected inverse: one launch.  One lane per system, the lanes of a wavefront on consecutive static
 * dims of one utterance.  The forward sweep assembles column t of R, eliminates it (banded L D L^T), adds log D_t and keeps
 * 1 / D_t and the column's Q multipliers in row t of the band planes; the backward sweep t = T - 1 .. 0 is Takahashi's recurrence
 *     S[t, t + k] = - sum_{j = 1 .. Q} l_{t+j, t} S[t + j, t + k]          S[t, t] = 1 / D_t - sum_j l_{t+j, t} S[t + j, t]
 * which overwrites row t after reading it: no workspace, and T is bounded by the buffer alone.  Rows at or past T of every plane
 * get zeros.  want_band = 0: the forward sweep only -- logdet and status are written, band may be NULL.
 * status[b, d]: 0, or the 1-based frame of the first non-positive pivot; that system's logdet and its band rows below T are NaN
 * then, and no other system is disturbed.  No atomics, no workgroup waits for another; a system's bits depend on its own inputs
 * alone. */
int nnmk_traj_covariance(int device, void *stream, int dtype, const void *variances, int var_mode, int64_t ld_in,
                         const int32_t *lengths, int B, int Tmax, int D, int sd, int num_windows, const int32_t *win_l,
                         const int32_t *win_u, const double *win_coef, int want_band, double *band, int64_t ld_band,
                         double *logdet, int32_t *status);

/* The negative log-likelihood of the target trajectories and its gradients.  means: device (B, Tmax, D), row stride ld_in (the
 * variances' too); cbar: the trajectory the forward pass gave for (means, variances), device (B, Tmax, sd) of `dtype`, row
 * stride ld_cbar >= sd; target: the natural trajectory c, the same layout with ld_target; band, logdet: what
 * nnmk_traj_covariance wrote for the same variances, windows and lengths.  With e = c - cbar:
 *     nll[b, d] = 1/2 sum_w sum_t tau_w[t] (W_w e)_t^2 - 1/2 logdet[b, d] + T / 2 log 2 pi              (device float64 (B, sd))
 *     grad_means[b, t, w sd + d] = - tau_w[t] (W_w e)_t                                     (device (B, Tmax, D) of `dtype`, dense)
 *     d nll / d tau_w[t] = 1/2 a^2 - a (mu_w[t] - (W_w cbar)_t) - 1/2 (W_w S W_w^T)_tt,   a = (W_w e)_t
 *     grad_vars = - tau^2 d nll / d tau, exactly 0 where tau is forced to 0: (B, Tmax, D) dense for per-frame variances, summed
 *     over b and t to (D) for global ones (both of `dtype`), NULL for unit ones.
 * grad_means and grad_vars may each be NULL (not wanted); band may be NULL unless grad_vars is wanted.  Rows at or past T get zeros.
 * Every sum over t is deterministic: each lane adds its dim's frames over a fixed four-way partition of [0, T), and the four
 * partial sums meet in LDS in a fixed order; the sum over b of the global-variance gradient is a second launch (one thread per
 * column, utterances in order) over `workspace` (device, at least nnmk_traj_nll_workspace(...) bytes, 8-byte aligned; may be
 * NULL when that is 0).  No atomics: the same bits on every call.  One launch, two with a global-variance gradient. */
int nnmk_traj_nll(int device, void *stream, int dtype, const void *means, const void *variances, int var_mode, int64_t ld_in,
                  const int32_t *lengths, int B, int Tmax, int D, int sd, int num_windows, const int32_t *win_l,
                  const int32_t *win_u, const double *win_coef, const void *cbar, int64_t ld_cbar, const void *target,
                  int64_t ld_target, const double *band, int64_t ld_band, const double *logdet, double *nll, void *grad_means,
                  void *grad_vars, void *workspace, int64_t workspace_bytes);

/* bytes of workspace nnmk_traj_nll needs: 8 B D for a global-variance gradient (want_grad_vars != 0), else 0; -1 for a bad
 * var_mode or a negative size (host code) */
int64_t nnmk_traj_nll_workspace(int var_mode, int want_grad_vars, int B, int D);

/* calls of nnmk_traj_covariance and nnmk_traj_nll that launched, since the library was loaded (a test aid) */
long long nnmk_traj_launch_count(void);

#ifdef __cplusplus
}
#endif

#endif
