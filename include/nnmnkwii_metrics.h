/* Objective metrics over padded batches on the device (nnmnkwii.metrics: melcd, mean_squared_error, lf0_mean_squared_error,
 * vuv_error) -- an extension header of libmlpg_hip.so with its own prefix and version.  include/mlpg_hip.h, its ABI version, its
 * export list and the kinds of mlpg_hip_launch_count are not touched by it; errors are read with mlpg_hip_last_error().
 * Plain C99.  DESIGN.md K13; csrc/frame_metrics.hip; tools/metrics_model.py is the executable specification. */
#ifndef NNMNKWII_METRICS_H
#define NNMNKWII_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNMK_METRICS_ABI_VERSION 1
#define NNMK_METRICS_F32 0
#define NNMK_METRICS_F64 1
#define NNMK_METRICS_MAX_TERMS 8
/* frames of ONE utterance per workgroup, counted from the utterance's frame 0 */
#define NNMK_METRICS_BLOCK_ROWS 256
/* bytes of one frame the terms may span: the columns from the first to the last one any term names, of x (rounded up to 8 bytes)
 * plus of y (rounded up to 8 bytes).  A wave stages them in LDS: four waves' worth and the workgroup's own 384 bytes fit 64 KB. */
#define NNMK_METRICS_MAX_ROW_BYTES 16000

/* kinds of a term: what is summed over the live frames of an utterance, and what is counted */
#define NNMK_METRICS_FRAME_L2 0        /* sqrt(sum_d (x[t, x_col + d] - y[t, y_col + d])^2); live frames */
#define NNMK_METRICS_SQUARED 1         /* sum_d (x - y)^2; live frames * width */
#define NNMK_METRICS_VOICED_SQUARED 2  /* width 1: z^2 on the frames both sides call voiced, z = x - y or exp(x) - exp(y); those frames */
#define NNMK_METRICS_MISMATCH 3        /* elements with x != y, or (x > threshold) != (y > threshold); live frames * width */
#define NNMK_METRICS_FLAG_EXP 1        /* VOICED_SQUARED: z = exp(x) - exp(y) */

/* Columns count from the pointers x and y.  Voiced (VOICED_SQUARED): x[t, x_mask_col] + y[t, y_mask_col] >= 2 if threshold is NaN,
 * else x[t, x_mask_col] > threshold && y[t, y_mask_col] > threshold.  MISMATCH: threshold NaN means x != y.  The other kinds do
 * not look at threshold and the mask columns.  All arithmetic is float64. */
typedef struct nnmk_metrics_term {
  int32_t kind;
  int32_t x_col, y_col, width;
  int32_t x_mask_col, y_mask_col;
  int32_t flags;
  double threshold;
} nnmk_metrics_term;

/* 1 */
int nnmk_metrics_abi_version(void);

/* Bytes of workspace nnmk_metrics_batch needs: 16 * nterms per workgroup, B * ceil(Tmax / NNMK_METRICS_BLOCK_ROWS) workgroups.
 * -1: a negative size, or the count does not fit. */
int64_t nnmk_metrics_workspace(int B, int Tmax, int nterms);

/* Evaluates terms[0 .. nterms - 1] (host memory, read before the call returns) over x and y: padded (B, Tmax, .) device arrays of
 * dtype_x / dtype_y (NNMK_METRICS_F32 | _F64) with row strides ld_x, ld_y in elements and utterance strides Tmax * ld.  lengths:
 * device int32 (B), clamped to [0, Tmax], or NULL (every frame live); frames past an utterance's length are never read.
 * totals: device double (nterms, 2), the pairs (sum, count) over the batch; per_utt: device double (B, nterms, 2) or NULL.
 * workspace: device memory, 8-byte aligned, at least nnmk_metrics_workspace(B, Tmax, nterms) bytes.  Two launches on `stream`
 * (one if B * Tmax == 0: the totals are then zeros), no atomics: the same bits on every call.  An utterance's per_utt values
 * depend on its own live frames and the term alone.
 * Returns 0, or -1 with the text "metrics: ..." (nothing was launched, the runtime was not touched), or -2 (runtime error). */
int nnmk_metrics_batch(int device, void *stream, int dtype_x, const void *x, int64_t ld_x, int dtype_y, const void *y, int64_t ld_y,
                       const int32_t *lengths, int B, int Tmax, const nnmk_metrics_term *terms, int nterms, double *per_utt,
                       double *totals, void *workspace, int64_t workspace_bytes);

/* calls of nnmk_metrics_batch that launched, since the library was loaded (a test aid) */
long long nnmk_metrics_launch_count(void);

#ifdef __cplusplus
}
#endif

#endif
