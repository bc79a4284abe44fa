/* Draws from MLPG's trajectory distribution N(c; cbar, R^-1) over padded batches, and the inverse map that whitens a trajectory
 * under it -- an extension header of libmlpg_hip.so with its own prefix and version.  include/mlpg_hip.h, its ABI version, its
 * export list, the kinds of mlpg_hip_launch_count and the other extension headers are not touched by it; errors are read with
 * mlpg_hip_last_error().  Plain C99.  DESIGN.md K20; csrc/mlpg_trajsample.hip; tools/trajsample_model.py is the executable
 * specification.
 *
 * The dtype codes, the variance modes, the window tables, the clamping of `lengths` to [0, Tmax] and the meaning of R, tau, Q
 * and one "system" (utterance b, static dim d) are those of nnmnkwii_trajectory.h. */
#ifndef NNMNKWII_SAMPLE_H
#define NNMNKWII_SAMPLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNMK_DRAW_ABI_VERSION 1

/* R = L D L^T (L unit lower triangular of half-bandwidth Q, D diagonal).  A draw is c = cbar + L^-T D^-1/2 z with z white; the
 * inverse map is z = D^1/2 L^T (c - cbar), and 1/2 |z|^2 is the quadratic term of nnmk_traj_nll.
 *
 * The FACTOR is planar like the band of nnmk_traj_covariance: device float64 (Q + 1, B, Tmax, sd), plane k's rows with stride
 * ld_fac >= sd in elements (utterance stride Tmax * ld_fac, plane stride B * Tmax * ld_fac).  Plane 0 row t holds 1 / D_t, plane k
 * row t holds l_{t+k,t}; rows at or past T are zero.  The values are bit for bit what nnmk_traj_covariance's forward sweep
 * leaves.  status: device int32 (B, sd), logdet: device float64 (B, sd), dense.
 *
 * Every launch goes on the caller's `stream`; no entry synchronises, allocates or puts work on another stream; no atomics, no
 * workgroup waits for another; all offsets are 64-bit.  All return 0, or -1 with the text "sample: ..." (nothing was launched,
 * the runtime was not touched, the counter did not move), or -2 (runtime error).  Refused with -1: an unknown dtype or var_mode,
 * a negative size, D != num_windows * sd, bad window tables, a window extent above 1, Q outside [0, 2], a row stride below the
 * width or so large that the last row lies past 2^62 bytes, a batch too large for one grid (B * ceil(sd / 64) above 2^24 - 1
 * workgroups), NULL for an array that has elements, factor planes that overlap the inputs, logdet or status of nnmk_draw_factor,
 * and an output of nnmk_draw_sample / nnmk_draw_whiten that overlaps the factor (nnmk_draw_whiten: or its x).
 * B = 0, Tmax = 0, sd = 0 and K = 0 return 0 and launch nothing (their other arguments are still checked). */

/* 1 */
int nnmk_draw_abi_version(void);

/* The forward sweep of nnmk_traj_covariance alone: one launch, one lane per system.  logdet and status as that entry writes them.
 * status[b, d]: 0, or the 1-based frame of the first non-positive pivot; that system's logdet and its factor rows below T are NaN
 * then, and no other system is disturbed. */
int nnmk_draw_factor(int device, void *stream, int dtype, const void *variances, int var_mode, int64_t ld_in,
                     const int32_t *lengths, int B, int Tmax, int D, int sd, int num_windows, const int32_t *win_l,
                     const int32_t *win_u, const double *win_coef, double *factor, int64_t ld_fac, double *logdet,
                     int32_t *status);

/* K draws per system by back-substitution.  noise, out: device (K, B, Tmax, sd) of `dtype`, row strides ld_noise, ld_out >= sd,
 * draw stride B * Tmax * ld; mean: device (B, Tmax, sd) of `dtype`, row stride ld_mean, or NULL (zero-mean draws).  For
 * t = T - 1 .. 0:
 *     x_t = z_t * sqrt(fac_0[t]) - fac_1[t] * x_{t+1} - fac_2[t] * x_{t+2}     (terms with t + j >= T absent, subtracted in order)
 *     out_t = mean_t + x_t
 * in float64, rounded once to `dtype`.  Rows at or past T of out are zero; rows at or past T of noise and mean are never loaded.
 * A system with status != 0 gets NaN in its rows below T.  One launch: one lane per system, kDrawGroup draws side by side in a
 * lane, the groups one after another.  A draw's bits depend neither on K nor on its place in a group. */
int nnmk_draw_sample(int device, void *stream, int dtype, const double *factor, int64_t ld_fac, const int32_t *status,
                     const int32_t *lengths, int B, int Tmax, int sd, int Q, int K, const void *noise, int64_t ld_noise,
                     const void *mean, int64_t ld_mean, void *out, int64_t ld_out);

/* The inverse map, with the shapes, the zero rows and the NaN rule of nnmk_draw_sample (x, z: (K, B, Tmax, sd)).  With e = x - mean:
 *     z_t = (e_t + fac_1[t] * e_{t+1} + fac_2[t] * e_{t+2}) / sqrt(fac_0[t])     (terms with t + j >= T absent, added in order)
 * One launch, four waves per (utterance, 64 static dims) over a partition of the system's own [0, T): a frame's result depends
 * on that frame's inputs alone, so the bits do not depend on the partition. */
int nnmk_draw_whiten(int device, void *stream, int dtype, const double *factor, int64_t ld_fac, const int32_t *status,
                     const int32_t *lengths, int B, int Tmax, int sd, int Q, int K, const void *x, int64_t ld_x,
                     const void *mean, int64_t ld_mean, void *z, int64_t ld_z);

/* the number of draws a lane of nnmk_draw_sample carries side by side (a compile-time constant of the library) */
int nnmk_draw_group(void);

/* calls of nnmk_draw_factor, nnmk_draw_sample and nnmk_draw_whiten that launched, since the library was loaded (a test aid) */
long long nnmk_draw_launch_count(void);

#ifdef __cplusplus
}
#endif

#endif
