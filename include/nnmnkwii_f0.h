/* Continuous F0 on the device: the unvoiced gaps of F0 / log-F0 tracks filled (the reference's preprocessing.interp1d) and the
 * voiced / unvoiced flag, over padded batches -- an extension header of libmlpg_hip.so with its own prefix and version.
 * include/mlpg_hip.h, its ABI version, its export list, the kinds of mlpg_hip_launch_count, include/nnmnkwii_metrics.h and
 * include/nnmnkwii_frontend.h are not touched by it; errors are read with mlpg_hip_last_error().  Plain C99.
 * DESIGN.md K15; csrc/f0_interp.hip; tools/f0_model.py is the executable specification. */
#ifndef NNMNKWII_F0_H
#define NNMNKWII_F0_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNMK_F0_ABI_VERSION 1
/* dtypes, independently for x, y and vuv */
#define NNMK_F0_F32 0
#define NNMK_F0_F64 1
/* kinds.  A fillable frame t (value <= 0) lies between the knots p < t < q with values a and b (below). */
#define NNMK_F0_SLINEAR 0      /* a + (b - a) * ((t - p) / (q - p)): float64, four rounded operations, no contraction */
#define NNMK_F0_LINEAR 1       /* the same */
#define NNMK_F0_PREVIOUS 2     /* a */
#define NNMK_F0_ZERO 3         /* a */
#define NNMK_F0_NEXT 4         /* b */
#define NNMK_F0_NEAREST 5      /* a if 2 (t - p) <= q - p, else b */
#define NNMK_F0_NEAREST_UP 6   /* a if 2 (t - p) < q - p, else b */
/* frames per step of a workgroup's walk along its column; the kernel's LDS use (a tile of float64 and a few words) does not
 * depend on Tmax, and no length is refused */
#define NNMK_F0_TILE 256

/* 1 */
int nnmk_f0_abi_version(void);

/* One launch on `stream` over the padded batch (a batch of more than 2^24 - 1 (utterance, column) pairs goes in slices of that
 * many).  x: device (B, Tmax, C) of dtype_x with row stride ld_x >= C in elements (utterance stride Tmax * ld_x); lengths: device
 * int32 (B), clamped to [0, Tmax], or NULL (Tmax each); y, vuv: device (B, Tmax, C) of dtype_y / dtype_vuv with row strides
 * ld_y, ld_vuv >= C; either may be NULL (not wanted), not both.  Every column of every utterance on its own, over its L live
 * frames: a frame is voiced (x > 0), fillable (x <= 0) or neither (NaN).  Without a voiced frame, or with L < 2, y = x.
 * Otherwise frame 0 takes the first voiced value and frame L-1 the last, whatever they held; the knots are the voiced frames and
 * these two; a fillable frame between two knots gets the value of `kind`, computed in float64 from values read in dtype_x and
 * rounded once to dtype_y; every other frame is converted.  vuv = 1 where the original x > 0, else 0.  Rows at or past L of y
 * and vuv get zeros; no frame of x there is read.  No byte outside the C columns of the B * Tmax rows of y and vuv is written.
 * All offsets are 64-bit.
 *
 * y may be x itself (the same pointer, dtype and stride): a frame is read before it is written, and the look-ahead reads only
 * frames the walk has not reached.  Any other overlap between x, y and vuv is the caller's error.
 *
 * Returns 0, or -1 with the text "f0: ..." (nothing was launched, the runtime was not touched), or -2 (runtime error).  Refused
 * with -1: an unknown dtype or kind, a negative size, a row stride below C, NULL for an array that has elements, y and vuv
 * both NULL.  B * Tmax * C == 0 launches nothing and returns 0. */
int nnmk_f0_interp(int device, void *stream, int dtype_x, const void *x, int64_t ld_x, const int32_t *lengths, int B, int Tmax, int C,
                   int kind, int dtype_y, void *y, int64_t ld_y, int dtype_vuv, void *vuv, int64_t ld_vuv);

/* calls of nnmk_f0_interp that launched, since the library was loaded (a test aid) */
long long nnmk_f0_launch_count(void);

#ifdef __cplusplus
}
#endif

#endif
