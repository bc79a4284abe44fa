/* Silence frames dropped on the device: the reference's
 *     idx = labels.silence_frame_indices(regex); X = np.delete(X, idx, axis=0); Y = np.delete(Y, idx, axis=0)
 * over padded batches, as a stream compaction whose keep mask is constant over each phone -- an extension header of
 * libmlpg_hip.so with its own prefix and version.  include/mlpg_hip.h, its ABI version, its export list, the kinds of
 * mlpg_hip_launch_count and the other extension headers are not touched by it; errors are read with mlpg_hip_last_error().
 * Plain C99.  DESIGN.md K18; csrc/frame_keep.hip; tools/silence_model.py is the executable specification.
 *
 * The dtype codes, the sub-phone kinds, NNMK_FRONTEND_MAX_S and NNMK_FRONTEND_MAX_STATES are those of nnmnkwii_frontend.h. */
#ifndef NNMNKWII_SILENCE_H
#define NNMNKWII_SILENCE_H

#include <stdint.h>

#include "nnmnkwii_frontend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNMK_SIL_ABI_VERSION 1
/* OUTPUT rows of ONE utterance per workgroup, counted from the utterance's first kept row */
#define NNMK_SIL_BLOCK_ROWS 64

/* Common to the three entries.  durations: device (B, Nmax, S), dense, of dtype_dur (any of the four codes), turned into frames
 * as nnmnkwii_frontend.h says (rint, then min_frames, then the cap at 2^31 - 1); num_phones: device int32 (B), clamped to
 * [0, Nmax], or NULL (Nmax each); silence: device (B, Nmax), dense, one byte per phone, non-zero: every frame of the phone is
 * silent.  No duration, phone row or flag at or past an utterance's num_phones is read.  S in 1 .. NNMK_FRONTEND_MAX_S and
 * Nmax * S <= NNMK_FRONTEND_MAX_STATES.  T_b: the frames of utterance b; K_b: those among them whose phone is not flagged.
 *
 * A workgroup of nnmk_sil_expand / nnmk_sil_gather (four waves, NNMK_SIL_BLOCK_ROWS output rows) redoes the int64 scan over its
 * utterance's states and keeps TWO running counts behind every state in dynamic LDS, one int32 each, saturated at 2^31 - 1: the
 * frames, and the kept frames.  An output row finds its state by binary search on the kept counts -- a flagged state and a state
 * of 0 frames add nothing to them and are never found -- and its source frame is the frame count in front of that state plus the
 * offset inside it.  No scan over frames, no atomics, no workgroup waits for another.  LDS: 8 bytes per state plus 0.3 KB (gather)
 * or 4.9 KB (expand): about 3 KB for the few hundred states of a Merlin utterance; 64 KB + that at the cap of 8192 states, which
 * leaves two workgroups per compute unit (160 KB).  Neither case has been measured.
 *
 * All return 0, or -1 with the text "silence: ..." (nothing was launched, the runtime was not touched, the counter did not
 * move), or -2 (runtime error).  Refused with -1: an unknown dtype or kind, a negative size or min_frames, S or Nmax * S out of
 * range, a row stride below the width, a batch too large for one grid (2^24 - 1 workgroups: B for the counts, B * ceil(Tcap / 64)
 * for the other two), NULL for an array that has elements, the coarse-coding kind without its table, scale_ without min_ or the
 * reverse, out == src, a source of Tmax = 2^31 - 1 rows.  All offsets are 64-bit. */

/* 1 */
int nnmk_sil_abi_version(void);

/* counts (device int64 (B, 2)): counts[b][0] = K_b, counts[b][1] = T_b.  One workgroup per utterance, one launch on `stream`. */
int nnmk_sil_frame_counts(int device, void *stream, int dtype_dur, const void *durations, const int32_t *num_phones,
                          const uint8_t *silence, int B, int Nmax, int S, int min_frames, int64_t *counts);

/* nnmk_frontend_expand with the silent frames left out: row r < min(K_b, Tcap) of out (B, Tcap, Dl + F) is the row
 * nnmk_frontend_expand writes for the r-th non-silent frame of utterance b -- the sub-phone columns from the frame's place in the
 * ORIGINAL phone (i, fn, base and pd are not changed by the removal), the same optional scale_ / min_ map, one rounding to
 * dtype_out.  Rows from there to Tcap get zeros; lengths_out[b] (device int32 (B)) = min(K_b, Tcap).  Silent frames are never
 * materialised.  phone, cc, scale_, min_, out, ld_phone, ld_out: as in nnmk_frontend_expand.  No column at or past Dl + F and no
 * byte outside out's B * Tcap rows is written.  One launch on `stream`. */
int nnmk_sil_expand(int device, void *stream, int dtype_phone, const void *phone, int64_t ld_phone, int dtype_dur,
                    const void *durations, const int32_t *num_phones, const uint8_t *silence, int B, int Nmax, int S, int Dl,
                    int min_frames, int kind, const double *cc, const double *scale_, const double *min_, int dtype_out, void *out,
                    int64_t ld_out, int Tcap, int32_t *lengths_out);

/* The same removal for any frame-level matrix.  src: device (B, Tmax, D) of dtype_src (F32 | F64) with row stride ld_src >= D in
 * elements (utterance stride Tmax * ld_src); len_src: device int32 (B), clamped to [0, Tmax], or NULL (Tmax each).  Frame
 * t < len_src[b] is dropped iff t < T_b and its phone is flagged; frames at or past T_b are kept (np.delete keeps them); silent
 * frames at or past len_src[b] do not exist.  The kept rows go, in order, to the first rows of out (B, Tcap, D) of dtype_out
 * (F32 | F64; converted, rounded once; row stride ld_out >= D, utterance stride Tcap * ld_out); the rows behind them get zeros;
 * lengths_out[b] = min(their number, Tcap).  No row of src at or past its length is read, no byte outside out's D columns is
 * written.  out == src is refused (rows move across workgroups); any other overlap is the caller's error.  One launch. */
int nnmk_sil_gather(int device, void *stream, int dtype_dur, const void *durations, const int32_t *num_phones, const uint8_t *silence,
                    int B, int Nmax, int S, int min_frames, int dtype_src, const void *src, int64_t ld_src, const int32_t *len_src,
                    int Tmax, int D, int dtype_out, void *out, int64_t ld_out, int Tcap, int32_t *lengths_out);

/* calls of the three entries above that launched, since the library was loaded (a test aid) */
long long nnmk_sil_launch_count(void);

#ifdef __cplusplus
}
#endif

#endif
