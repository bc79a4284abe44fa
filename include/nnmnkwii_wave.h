/* The waveform side of the reference's preprocessing on the device, over padded batches of waveforms: pre-emphasis, mu-law
 * companding and quantisation in one launch ("encode"), and expansion and de-emphasis in one launch ("decode") -- the
 * reference's mulaw, inv_mulaw, mulaw_quantize, inv_mulaw_quantize, preemphasis and inv_preemphasis
 * (preprocessing/generic.py:56-226).  An extension header of libmlpg_hip.so with its own prefix and version.
 * include/mlpg_hip.h, its ABI version, its export list, the kinds of mlpg_hip_launch_count and the other extension headers are
 * not touched by it; errors are read with mlpg_hip_last_error().  Plain C99.
 * DESIGN.md K16; csrc/wave_codec.hip; tools/wave_model.py is the executable specification. */
#ifndef NNMNKWII_WAVE_H
#define NNMNKWII_WAVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNMK_WAVE_ABI_VERSION 1
/* dtypes: waveforms and companded values are F32 or F64, classes U8, I16, I32 or I64 */
#define NNMK_WAVE_F32 0
#define NNMK_WAVE_F64 1
#define NNMK_WAVE_U8 2
#define NNMK_WAVE_I16 3
#define NNMK_WAVE_I32 4
#define NNMK_WAVE_I64 5
/* the mu-law stage of encode (what y holds) and of decode (what x holds) */
#define NNMK_WAVE_PLAIN 0      /* none: a waveform */
#define NNMK_WAVE_MULAW 1      /* companded floats in [-1, 1] */
#define NNMK_WAVE_QUANTIZE 2   /* classes in [0, mu] */
/* samples per step of a decode workgroup's walk (256 threads, 4 consecutive samples each), and per encode workgroup */
#define NNMK_WAVE_TILE 1024
/* a decode table of at most this many entries (mu + 1) is looked up from LDS, a longer one from memory */
#define NNMK_WAVE_TABLE_LDS 4096

/* 1 */
int nnmk_wave_abi_version(void);

/* Common to both launches.  x: device (B, Lmax) of dtype_x with utterance stride ld_x >= Lmax in elements; y: device (B, Lmax)
 * of dtype_y with utterance stride ld_y >= Lmax; lengths: device int32 (B), clamped to [0, Lmax], or NULL (Lmax each).  Samples
 * of x at or past lengths[b] are never read; there y gets 0 (float outputs) or the class of silence, mu / 2 (class outputs).
 * No byte outside the Lmax samples of the B rows of y is written.  All offsets are 64-bit; a batch over the grid's limit goes
 * in slices.  mu is an integer >= 1.  Non-finite samples give NaN (float outputs); as a class a NaN gives 0.
 *
 * Both return 0, or -1 with the text "wave: ..." (nothing was launched, the runtime was not touched), or -2 (runtime error).
 * B * Lmax == 0 launches nothing and returns 0 after the checks. */

/* encode: waveform -> [pre-emphasis] -> [mu-law] -> [quantise], elementwise with one neighbour, one launch.
 *   emphasis != 0: p[0] = x[0] + 0, p[n] = fl(x[n] + fl(fl(-coef) x[n-1])) computed in dtype_x with coef rounded to it first
 *     (bit for bit scipy.signal.lfilter([1, -coef], [1], x), whose state starts at +0.0); emphasis == 0: p = x.
 *   stage PLAIN: y = p converted to dtype_y.
 *   stage MULAW: y = sign(p) log1p(mu |p|) / log1p(mu) in float64 on p as read, rounded once to dtype_y (F32 / F64).
 *   stage QUANTIZE: v = (mulaw + 1) / 2 * mu in float64, the class is v truncated toward zero; no clamp: |p| > 1 leaves
 *     [0, mu] as in the reference.  p = -1, +1, +-0 give 0, mu and mu / 2 exactly (both logarithms come from the device's own
 *     log1p).  dtype_y is a class dtype (U8 is refused for mu > 255) and the value is narrowed to it.
 * dtype_x is F32 or F64 (integer waveforms are refused: the reference truncates coef to an integer there).
 * Without pre-emphasis y may be x itself when the element sizes match; with it equal pointers are refused (a neighbouring
 * workgroup would race on the boundary sample).  Any other overlap is the caller's error. */
int nnmk_wave_encode(int device, void *stream, int dtype_x, const void *x, int64_t ld_x, const int32_t *lengths, int B, int Lmax,
                     int emphasis, double coef, int stage, int mu, int dtype_y, void *y, int64_t ld_y);

/* decode: classes or companded floats -> [expand] -> [de-emphasis] -> waveform, one launch.
 *   stage QUANTIZE: x holds classes (U8 / I16 / I32 / I64); the value is table[class], table a device float32 array of mu + 1
 *     entries (the Python layer fills it with the reference's literal expression: the kernel holds no transcendental here).
 *     Classes outside [0, mu] are the caller's error and are clamped to the table's ends.
 *   stage MULAW: x holds floats; the value is sign(x) (1 / mu) ((1 + mu)^|x| - 1) in float64 on x as read.
 *   stage PLAIN: x holds floats; the value is x.  table is looked at for QUANTIZE only.
 *   emphasis != 0: y[n] = value[n] + coef y[n-1] as a scan in float64 (coef as given: the caller rounds it to the dtype the
 *     reference would filter in), rounded once to dtype_y (F32 / F64) on store.  It does not reproduce the bits of the reference's
 *     sequential recurrence in dtype_x; tools/wave_model.py carries the bound.  |coef| < 1 is not required without segments.
 *   segment: 0 chooses automatically, a value >= Lmax walks each utterance with one workgroup, any other value must be a
 *     positive multiple of NNMK_WAVE_TILE that passes nnmk_wave_plan (else -1).  Looked at with de-emphasis only.
 * With de-emphasis equal pointers are refused (a segment's warm-up reads what its neighbour writes); without it y may be x when
 * the element sizes match. */
int nnmk_wave_decode(int device, void *stream, int dtype_x, const void *x, int64_t ld_x, const int32_t *lengths, int B, int Lmax,
                     int stage, int mu, const float *table, int emphasis, double coef, int64_t segment, int dtype_y, void *y,
                     int64_t ld_y);

/* How decode with de-emphasis splits an utterance of Lmax samples among workgroups: a pure host function, so the bits of a
 * result depend on (Lmax, coef, segment) alone, never on the device or the call.  *W: the warm-up, the smallest positive multiple
 * of NNMK_WAVE_TILE with |coef|^W <= 2^-80 (found by repeated multiplication of |coef|^NNMK_WAVE_TILE, itself ten squarings;
 * -1: |coef| >= 1, NaN, or beyond 2^30 samples).  *S: the samples per segment, *nseg their count.  Segment j > 0 starts from a
 * zero state W samples before its first sample, j S.  segment == 0: the built-in choice, taken when Lmax > S and
 * 0 < W <= S / 4 (a warm-up of at most a quarter of the work), else *S = Lmax, *nseg = 1.  segment >= Lmax: no split.  An
 * explicit segment below Lmax that is no positive multiple of the tile, or for which the decay fails (no W, or W > S: the
 * warm-up would start in front of the segment before), returns -1 with the text "wave: ...".  Any of S, W, nseg may be NULL. */
int nnmk_wave_plan(int64_t Lmax, double coef, int64_t segment, int64_t *S, int64_t *W, int64_t *nseg);

/* calls of nnmk_wave_encode and nnmk_wave_decode that launched, since the library was loaded (a test aid) */
long long nnmk_wave_launch_count(void);

#ifdef __cplusplus
}
#endif

#endif
