/* Phone-level linguistic features expanded to frames on the device (the duration-dependent part of the reference's
 * frontend.merlin.linguistic_features(..., add_frame_features=True, subphone_features=...)) -- an extension header of
 * libmlpg_hip.so with its own prefix and version.  include/mlpg_hip.h, its ABI version, its export list, the kinds of
 * mlpg_hip_launch_count and include/nnmnkwii_metrics.h are not touched by it; errors are read with mlpg_hip_last_error().
 * Plain C99.  DESIGN.md K14; csrc/frame_expand.hip; tools/frontend_model.py is the executable specification. */
#ifndef NNMNKWII_FRONTEND_H
#define NNMNKWII_FRONTEND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNMK_FRONTEND_ABI_VERSION 1
/* dtypes: the phone matrix and the output take F32 | F64, the durations any of the four */
#define NNMK_FRONTEND_F32 0
#define NNMK_FRONTEND_F64 1
#define NNMK_FRONTEND_I32 2
#define NNMK_FRONTEND_I64 3
/* sub-phone kinds and the columns F they add behind the Dl phone-level ones (nnmk_frontend_feature_size).  A frame is frame i
 * (from 0) of state s (from 1) of fn frames; its phone has S states and pd frames, `base` of them in front of state s;
 * j = base + i.  Every quotient is one float64 division of two integers. */
#define NNMK_FRONTEND_NONE 0            /* 0 columns */
#define NNMK_FRONTEND_FULL 1            /* 9: (i+1)/fn, (fn-i)/fn, fn, s, S+1-s, pd, fn/pd, (pd-i-base)/pd, (base+i+1)/pd */
#define NNMK_FRONTEND_MINIMAL_FRAME 2   /* 2: (i+1)/fn, s */
#define NNMK_FRONTEND_STATE_ONLY 3      /* 1: s */
#define NNMK_FRONTEND_FRAME_ONLY 4      /* 1: (j+1)/pd */
#define NNMK_FRONTEND_UNIFORM_STATE 5   /* 2: (j+1)/pd, max(1, rint((j+1)/pd * 5)) */
#define NNMK_FRONTEND_COARSE_CODING 6   /* 4: (float)cc[0][300+q], (float)cc[1][200+q], (float)cc[2][100+q], pd; q = (int)((200/pd) * j) */
#define NNMK_FRONTEND_MINIMAL_PHONEME 7 /* 3: (j+1)/pd, (pd-j)/pd, pd */
#define NNMK_FRONTEND_MAX_S 8
#define NNMK_FRONTEND_CC_POINTS 600     /* the coarse-coding table is double (3, 600) */
/* frames of ONE utterance per workgroup, counted from the utterance's frame 0 */
#define NNMK_FRONTEND_BLOCK_ROWS 64
/* Nmax * S may not exceed this.  A workgroup of nnmk_frontend_expand keeps the running frame count behind every state of its
 * utterance in LDS, one int32 each, to find the states of its frames by binary search: 32 KB at the cap, which with the 5 KB of
 * its rows' sub-phone columns lets four workgroups share a compute unit's 160 KB.  (A Merlin utterance has a few hundred
 * states.) */
#define NNMK_FRONTEND_MAX_STATES 8192

/* Durations in frames, for both entries below: a floating-point duration is rounded to the nearest integer, halves to even; an
 * integer one is taken as it is; then whatever is not greater than min_frames (NaN included) becomes min_frames, and whatever
 * exceeds 2^31 - 1 counts as 2^31 - 1.  num_phones: device int32 (B), clamped to [0, Nmax], or NULL (Nmax each); no duration
 * and no phone row at or past an utterance's num_phones is read.
 *
 * Both return 0, or -1 with the text "frontend: ..." (nothing was launched, the runtime was not touched), or -2 (runtime
 * error).  Refused with -1: an unknown dtype or kind, a negative size or min_frames, S outside 1 .. NNMK_FRONTEND_MAX_S,
 * Nmax * S above NNMK_FRONTEND_MAX_STATES, a row stride below the width, a batch too large for one grid, NULL for an array that
 * has elements, the coarse-coding kind without its table, scale_ without min_ or the reverse. */

/* 1 */
int nnmk_frontend_abi_version(void);

/* F of a kind (0, 9, 2, 1, 1, 2, 4, 3 for kinds 0 .. 7), -1 for anything else */
int nnmk_frontend_feature_size(int kind);

/* counts[b] (device int64 (B)) = the frames of utterance b: the sum of its states' durations in frames.  durations: device
 * (B, Nmax, S), dense, of dtype_dur.  One launch on `stream`. */
int nnmk_frontend_frame_counts(int device, void *stream, int dtype_dur, const void *durations, const int32_t *num_phones, int B,
                               int Nmax, int S, int min_frames, int64_t *counts);

/* One launch on `stream` over the padded batch.  phone: device (B, Nmax, Dl) of dtype_phone with row stride ld_phone >= Dl in
 * elements (utterance stride Nmax * ld_phone); durations as above; cc: device double (3, 600), read by the coarse-coding kind
 * alone (NULL otherwise); scale_, min_: device double (Dl + F) each or both NULL -- a value v of column c becomes
 * v * scale_[c] + min_[c], the product and the sum each rounded.  out: device (B, Tmax, Dl + F) of dtype_out with row stride
 * ld_out >= Dl + F (utterance stride Tmax * ld_out; uninitialised memory is fine).  With T_b the frames of utterance b:
 * rows t < min(T_b, Tmax) get the phone's row followed by the sub-phone columns, computed in float64 and rounded once to
 * dtype_out; rows from there to Tmax get zeros; lengths_out[b] (device int32 (B)) = min(T_b, Tmax).  No column at or past
 * Dl + F and no byte outside out's B * Tmax rows is written.  All offsets are 64-bit. */
int nnmk_frontend_expand(int device, void *stream, int dtype_phone, const void *phone, int64_t ld_phone, int dtype_dur,
                         const void *durations, const int32_t *num_phones, int B, int Nmax, int S, int Dl, int min_frames, int kind,
                         const double *cc, const double *scale_, const double *min_, int dtype_out, void *out, int64_t ld_out,
                         int Tmax, int32_t *lengths_out);

/* calls of nnmk_frontend_expand that launched, since the library was loaded (a test aid) */
long long nnmk_frontend_launch_count(void);

#ifdef __cplusplus
}
#endif

#endif
