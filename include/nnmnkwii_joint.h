/* Joint feature rows on the device: the deltas of one or two padded batches side by side, the zero frames and the padding
 * removed, the kept rows written densely (the reference's delta_features + concatenate + remove_zeros_frames) -- an extension
 * header of libmlpg_hip.so with its own prefix and version.  include/mlpg_hip.h, its ABI version, its export list, the kinds of
 * mlpg_hip_launch_count and the other extension headers are not touched by it; errors are read with mlpg_hip_last_error().
 * Plain C99.  DESIGN.md K17; csrc/joint_rows.hip; tools/joint_model.py is the executable specification. */
#ifndef NNMNKWII_JOINT_H
#define NNMNKWII_JOINT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNMK_JOINT_ABI_VERSION 1
/* dtypes, independently for x, y and out */
#define NNMK_JOINT_F32 0
#define NNMK_JOINT_F64 1
/* keep rules */
#define NNMK_JOINT_NONZERO 0   /* keep the row iff s > eps, s the float64 sum of |row[j]| over the rounded output values */
#define NNMK_JOINT_LIVE 1      /* keep iff t < max(len_x[b], len_y[b]); no frame is read for the decision */
/* frames of one utterance per workgroup; one 64-bit keep mask per tile (at most 64) */
#define NNMK_JOINT_TILE 64
#define NNMK_JOINT_MAX_WINDOWS 8
#define NNMK_JOINT_MAX_EXTENT 8   /* the largest l or u of a window */

/* 1 */
int nnmk_joint_abi_version(void);

/* Bytes of device workspace nnmk_joint_count / _write need for a batch: 16 for every tile of NNMK_JOINT_TILE frames of every
 * utterance (the tile's keep mask and its first output row), B * ceil(Tmax / TILE) tiles.  -1 for a negative size. */
int64_t nnmk_joint_workspace_bytes(int B, int Tmax);

/* The row of frame t of utterance b, of width W = (Dx + Dy) * nw, nw = max(num_windows, 1):
 *   row[w * Dx + d] = sum_{k = -l_w .. u_w} coef_w[l_w + k] * x[b, t + k, d]
 * in float64, from 0.0, k ascending, one rounded multiplication and one rounded addition per tap; taps outside
 * [0, len_x[b]) are skipped (x counts as 0 there); the whole x block is 0 for t >= len_x[b]; the value is rounded once to
 * dtype_out.  num_windows == 0: row[d] = x[b, t, d] converted (no arithmetic: -0.0 stays).  The y block follows at column
 * Dx * nw, built the same way from y and len_y; Dy == 0: there is no y (y and len_y are not looked at).  No element at or past a
 * source's length is read.
 *
 * x, y: device (B, Tmax, Dx | Dy) of dtype_x | dtype_y with row strides ld_x >= Dx, ld_y >= Dy in elements (utterance stride
 * Tmax * ld); len_x, len_y: device int32 (B), clamped to [0, Tmax], NULL: Tmax each.  win_l, win_u, win_coef: HOST arrays as
 * in mlpg_hip_delta_features (window w has l_w + u_w + 1 coefficients, one after another), l, u <= NNMK_JOINT_MAX_EXTENT.
 *
 * Keep rule NONZERO: s sums |row[j]| of the rounded values in float64 in one fixed order -- lane i of 64 takes j = i, i + 64, ...
 * ascending from 0.0, then for m = 32, 16, .. 1 every lane adds the sum of lane i ^ m -- and the row is kept iff s > eps (a NaN
 * sum drops it).  Rows with t >= max(len_x[b], len_y[b]) are dropped without being read.  LIVE: kept iff t < that maximum.
 *
 * nnmk_joint_count: two launches on `stream` (tiles beyond one grid go in slices; no atomics, no workgroup waits for another):
 * the keep masks of all tiles, then one workgroup's exclusive scan of their counts.  workspace then holds what _write needs, and
 * offsets, device int64 (B + 1), the first output row of every utterance and offsets[B] = N, the number of kept rows.
 *
 * nnmk_joint_write: one launch with the same sources, windows and workspace: kept row number r (in (b, t) order) goes to
 * out[r * ld_out + 0 .. W) of dtype_out -- the dtype_out given to _count -- for r < cap.  No byte outside the W columns of the
 * first min(N, cap) rows of out is written.  out must not overlap a source.  All offsets are 64-bit.  The same bits on every call.
 *
 * Both return 0, or -1 with the text "joint: ..." (nothing was launched, the runtime was not touched, no counter moved), or -2
 * (runtime error).  Refused with -1: an unknown dtype or keep mode, a negative size, a row stride below its width, num_windows > 8,
 * an l or u outside [0, 8], eps < 0 or NaN, NULL for an array that has elements, a workspace smaller than
 * nnmk_joint_workspace_bytes or not aligned to 8 bytes, cap < 0.  B * Tmax * W == 0 launches nothing, sets offsets to zeros if
 * B > 0, and returns 0. */
int nnmk_joint_count(int device, void *stream, int dtype_x, const void *x, int64_t ld_x, const int32_t *len_x, int Dx, int dtype_y,
                     const void *y, int64_t ld_y, const int32_t *len_y, int Dy, int B, int Tmax, int num_windows, const int32_t *win_l,
                     const int32_t *win_u, const double *win_coef, int keep, double eps, int dtype_out, void *workspace,
                     int64_t workspace_bytes, int64_t *offsets);

int nnmk_joint_write(int device, void *stream, int dtype_x, const void *x, int64_t ld_x, const int32_t *len_x, int Dx, int dtype_y,
                     const void *y, int64_t ld_y, const int32_t *len_y, int Dy, int B, int Tmax, int num_windows, const int32_t *win_l,
                     const int32_t *win_u, const double *win_coef, const void *workspace, int64_t workspace_bytes, int dtype_out,
                     void *out, int64_t ld_out, int64_t cap);

/* calls of nnmk_joint_count and nnmk_joint_write that launched, since the library was loaded (a test aid) */
long long nnmk_joint_launch_count(void);

#ifdef __cplusplus
}
#endif

#endif
