/*
 * include/mlpg_hip.h -- C ABI of libmlpg_hip.so (MI355X / gfx950).
 *
 * The reference (r9y9/nnmnkwii) has no FFI for this path: its native code is a
 * set of Cython extension modules imported by name.  This header is therefore
 * the boundary *we* introduce beneath the reference's Python signatures; each
 * entry point names the reference routine(s) it replaces (paths relative to
 * /root/reference/nnmnkwii/).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - All data pointers are DEVICE pointers on `device`, row-major, densely
 *    packed.  Pointers suffixed _h are HOST pointers (tiny window tables).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 *    only enqueue work; they never synchronise.  `status`/`path_len` are filled
 *    on the stream: read them after synchronising it.
 *  - dtype codes: MLPG_HIP_F32 = 0, MLPG_HIP_F64 = 1.
 *  - Return value: 0 on success, negative MLPG_HIP_E* on argument/runtime
 *    errors (text via mlpg_hip_last_error()).  Numerical failures (a leading
 *    minor that is not positive definite) are reported per system in `status`,
 *    never as a return code.
 *  - Windows are the reference's `(l, u, coeff)` triples packed as win_l_h[nw],
 *    win_u_h[nw], win_coef_h[sum(l+u+1)] (float64), window 0 first
 *    (paramgen/_mlpg.py:13-50).  Feature columns are window-major: column
 *    w*static_dim + d (paramgen/_mlpg.py:187-188).
 *  - Batches are the reference's zero-padded (B, Tmax, D) arrays
 *    (util/__init__.py:44-66, datasets/__init__.py:152-218); `lengths` (device
 *    int32[B], or NULL for "all Tmax") gives the valid frames per utterance.
 *    Output frames >= lengths[b] are zero-filled.
 *  - Re-entrant per (device, stream); internal scratch is cached per device
 *    and released by mlpg_hip_shutdown().  No OpenMP, no global mutable state
 *    besides that cache and the last-error string (thread-local).
 *  - Scratch and HIP graphs.  The scratch of a (device, stream) only grows: a
 *    call that needs more than its slot holds synchronises the stream, frees
 *    the slot and allocates a larger one.  None of that can happen while the
 *    stream is being captured, so an entry that uses scratch -- the solve
 *    routes of mlpg_hip_forward / _backward / _backward_var / _streams,
 *    mlpg_hip_fastdtw and the dtw_level calls, the direct and chirp-z routes
 *    of the modspec calls -- is "capturable once that scratch exists": run
 *    one call of the largest shape on the stream, then capture.  A captured
 *    graph holds the slot's address.  AFTER A CAPTURE, NO LARGER CALL ON THAT
 *    STREAM WHILE THE GRAPH LIVES: it would free the slot the graph's kernels
 *    still write to.  Calls of the same or a smaller shape, replays and calls
 *    on other streams are fine.
 */
#ifndef MLPG_HIP_H_
#define MLPG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLPG_HIP_F32 0
#define MLPG_HIP_F64 1

#define MLPG_HIP_EINVAL (-1)   /* bad argument (shape, dtype, window table)   */
#define MLPG_HIP_ERUNTIME (-2) /* HIP runtime error (launch, malloc, device)  */
#define MLPG_HIP_ENOMEM (-3)   /* scratch allocation failed                   */

/* Batch sizes.  Return code 0 means the WHOLE batch was done.  One kernel launch takes fewer than 2^32 threads; an entry whose
 * kernel has a workgroup per batch item (the modulation-spectrum entries, mlpg_hip_trim_lengths, _gather_path, _fastdtw, the
 * wave-per-system kernel of mlpg_hip_forward / _backward) walks a larger batch in several launches and still counts as one call.
 * What cannot be cut refuses with MLPG_HIP_EINVAL, nothing written and no counter moved, in a text that names the limit:
 * mlpg_hip_unit_mse_step in its one-launch form beyond 2^24 - 1 workgroups (8 per block of 8 utterances and group of 4 static
 * dims), MLPG_HIP_ALGO_FIR / _CHUNK / _GENERIC by name beyond their grids (AUTO takes another kernel), mlpg_hip_delta_features,
 * mlpg_hip_gmm_convert and the copy of one pass-through stream in mlpg_hip_forward_streams beyond 2^32 - 256 elements,
 * mlpg_hip_gmm_estep and its siblings beyond 2^30 - 64 rows, mlpg_hip_column_stats beyond 2^26 - 4 columns. */

/* variance modes */
#define MLPG_HIP_VAR_FRAME 0   /* var is (B, Tmax, D)                         */
#define MLPG_HIP_VAR_GLOBAL 1  /* var is (D,), tiled over frames (_mlpg.py:169-170) */
#define MLPG_HIP_VAR_UNIT 2    /* var == NULL: unit variances (_mlpg.py:297-373) */

/* kernel selection for the forward/backward solves */
#define MLPG_HIP_ALGO_AUTO 0    /* strip kernel for wide streams, wave-per-system for narrow, else generic */
#define MLPG_HIP_ALGO_GENERIC 1 /* thread-per-system, factor in HBM scratch       */
#define MLPG_HIP_ALGO_WAVE 2    /* wave-per-system, factor in registers           */
#define MLPG_HIP_ALGO_STRIP 3   /* lane-per-static-dim, wavefront per 16-frame chunk, any T.  A stream of 1 .. 32 static dims (forward,
                                   three windows): the lanes of a wavefront run over
                                   64 / dims consecutive utterances x the dims instead (the transposed form, round 5) */
#define MLPG_HIP_ALGO_PIPE 4    /* retired in ABI 11 (the software-pipelined strip kernel of round 3; its sources left the tree in
                                   round 6 and are in the git history under tools/experimental/pipe): selects the strip kernel */
#define MLPG_HIP_ALGO_CONST 5   /* global (D,) / unit variances: the matrix of a static dim is the same for every
                                   utterance (_mlpg.py:169-170 tiles the variances) -- factorised once per launch, the
                                   solves are constant-coefficient recurrences, lane-per-static-dim, any T */
#define MLPG_HIP_ALGO_CHUNK 6   /* window extents up to 2 (5-tap windows: P has half-bandwidth 4), forward and backward: chunks of 16 + 4 frames
                                   eliminated twice around a block-tridiagonal solve over their separators; no workgroup waits
                                   for another; lane-per-static-dim, any T */
#define MLPG_HIP_ALGO_FIR 7     /* unit variances on float32 tensors (autograd.unit_variance_mlpg, autograd/_impl/mlpg.py:108-172: the
                                   reference multiplies by a dense float32 R): P^-1 is Toeplitz away from the ends and decays by
                                   about a bit per frame -- a 49-tap FIR filter plus 24 table rows per end, every 32-frame tile
                                   independent; the decay is checked per window set, else MLPG_HIP_EINVAL (AUTO: another kernel) */

int mlpg_hip_abi_version(void);
const char *mlpg_hip_last_error(void);
/* Test aid, not part of the reference's interface: launches per MLPG kernel family since the library was loaded --
 * 0 natural-order, 1 wave-per-system, 2 strip, 3 strip with several streams merged, 4 constant-coefficient, 5 fused, 6 chunked, 7 FIR,
 * 8 constant-coefficient with several streams merged, 9 strip in its transposed form (narrow streams: the lanes over several
 * utterances); and, counting CALLS rather than launches, 10 host-memory calls that took the short path with their inputs copied to the
 * device, 11 with the kernel reading the pinned staging buffer itself (see mlpg_hip_forward_host); 100 + d: chunks the chunked
 * host-memory calls (mlpg_hip_forward_host_multi / mlpg_hip_fastdtw_host_multi) have enqueued on device d; 13 launches of the
 * variance-gradient kernel of mlpg_hip_backward_var; 15 launches of the stream-table epilogue of mlpg_hip_backward_streams; 17
 * launches of the typed in-LDS FFT kernel of mlpg_hip_modspec_batch / mlpg_hip_modspec_batch_backward, 18 transforms those two
 * calls sent through the direct transform, 19 launches of the fused loss kernel of mlpg_hip_modspec_loss_step; 20 CALLS of
 * mlpg_hip_modspec / _inv_modspec / _modspec_smoothing / _modspec_backward that the chirp-z kernel served (one per call); 31
 * launches of the kernel of mlpg_hip_modspec_filter; 33 launches of the kernel of mlpg_hip_gmm_trajectory_stats; 35
 * launches of the kernel of mlpg_hip_gv_ascent (one per call, whatever n_iter is), 37 of the kernel of mlpg_hip_gv; 39 CALLS of
 * mlpg_hip_column_stats that launched, 41 launches of the kernel of mlpg_hip_column_affine; -1 for any other `kind` (12, 14, 16,
 * 30, 32, 34, 36, 38, 40 and 42 included).
 * (Tests use it to assert WHICH kernel / route a call took.) */
long long mlpg_hip_launch_count(int kind);
int mlpg_hip_device_count(void);
/* Frees the per-device scratch caches. */
void mlpg_hip_shutdown(void);

/*
 * One training step of unit-variance MLPG under a mean-squared-error loss, fused: what the reference's
 * perf/autograd_mlpg_perf.py:56-86 loop does per batch with autograd.unit_variance_mlpg (autograd/_impl/mlpg.py:70-172:
 * dense R @ means forward, R^T @ grad backward) around torch.nn.MSELoss --
 *     y = MLPG(mean) with unit variances;  loss = sum_{live frames} (y - target)^2 / n_elems;
 *     grad_mean = d loss / d mean
 * in ONE kernel launch (wave-per-system scheme: both solves of a system share the launch, the trajectory stays in
 * registers between them).  mean (B, Tmax, D), target (B, Tmax, D/nw), grad_mean (B, Tmax, D) of `dtype`; y_out
 * (B, Tmax, D/nw) or NULL; loss: one float64 on the device; n_elems: the divisor of the mean (B * Tmax * D/nw for
 * nn.MSELoss over a padded batch).  Window extents <= 1, Tmax <= 1024.  The loss is summed in a fixed order
 * (bitwise repeatable).  status as for mlpg_hip_forward (may be NULL); a system whose status is non-zero gets 0 in its y and
 * grad_mean columns and adds nothing to the loss.
 * workspace: caller-owned device memory, 128-byte aligned, >= mlpg_hip_unit_mse_workspace_bytes(B, D, nw) bytes,
 * zeroed ONCE by the caller before its first use (the kernel leaves its arrival counter zero); one workspace per stream
 * that may run the call concurrently.  The call allocates nothing and is capturable into a HIP graph.
 * Float32 batches without lengths, Tmax >= 96, 1-3 windows of extent <= 2 the first of which is a single tap, given a workspace of
 * mlpg_hip_unit_mse_workspace_bytes_t(B, Tmax, D, nw) bytes: the step runs in the FIR form (MLPG_HIP_ALGO_FIR) as TWO launches --
 * forward + loss terms + d loss / d y into the workspace, then backward + the loss sum (fixed order, bitwise repeatable) -- with no
 * limit on Tmax; the first call for a window set builds the tap table (synchronous, not capturable: warm up before capturing).
 * With the smaller workspace of mlpg_hip_unit_mse_workspace_bytes the call behaves as before.
 */
int mlpg_hip_unit_mse_step(int device, void *stream, int dtype, const void *mean, const void *target,
                           const int32_t *lengths, int B, int Tmax, int D, int num_windows,
                           const int32_t *win_l_h, const int32_t *win_u_h, const double *win_coef_h,
                           double n_elems, void *y_out, void *grad_mean, double *loss, int32_t *status,
                           void *workspace, size_t workspace_bytes);
size_t mlpg_hip_unit_mse_workspace_bytes(int B, int D, int num_windows);
size_t mlpg_hip_unit_mse_workspace_bytes_t(int B, int Tmax, int D, int num_windows);
/*
 * Which form mlpg_hip_unit_mse_step takes for this problem when it is given the workspace of mlpg_hip_unit_mse_workspace_bytes_t:
 * 2 the FIR form, 1 the one-launch kernel, 0 neither (the step would return MLPG_HIP_EINVAL: the caller runs forward, loss and
 * backward as separate calls); negative: an error code.  The step decides with the same function.  The FIR form's conditions include
 * a property of the window set's NUMBERS (its inverse must decay to 2^-26 within 24 frames -- false for, e.g., dynamic windows scaled
 * by 4 or a static weight of 0.3), so the shape alone does not tell; the first query for a window set on a device builds the tap
 * table (synchronous).  While `stream` is being captured a table that does not exist yet cannot be built: the answer is then 1 or
 * 0, and may become 2 later (ABI 13).
 */
int mlpg_hip_unit_mse_form(int device, void *stream, int dtype, int has_lengths, int B, int Tmax, int D, int num_windows,
                           const int32_t *win_l_h, const int32_t *win_u_h, const double *win_coef_h);

/*
 * Measurement aid, not part of the reference's interface: a plain streaming copy of nbytes (a multiple of 16; both
 * pointers 16-byte aligned device memory), 16 bytes per lane and access.  bench.py times it in the same run as the
 * MLPG kernels to report the HBM rate a copy kernel reaches on the box ("fraction of both nominal and
 * measured-copy peak").
 */
int mlpg_hip_stream_copy(int device, void *stream, const void *src, void *dst, size_t nbytes);

/*
 * MLPG forward, batched.  Replaces paramgen.mlpg (paramgen/_mlpg.py:92-199)
 * and everything beneath it: build_win_mats (:13-50), build_poe (:53-89),
 * _bandmat/tensor.pyx dot_mv_plus_equals (:20-64) / dot_mm_plus_equals
 * (:82-174) and _bandmat/linalg.pyx solveh (:290-304) = _cholesky_banded
 * (:36-104) + _solve_triangular_banded (:106-176) x2.
 *
 *   out[b, :, d] = (sum_w W_w^T diag(tau_w) W_w)^-1 sum_w W_w^T (tau_w * mu_w)
 *   tau_w = 1/var evaluated in the INPUT dtype (:188), zeroed on the first/last
 *   max(max(l,u)) frames for w >= 1 (:177,191-193); all later arithmetic float64.
 *
 *   mean : (B, Tmax, D) dtype      var : per var_mode      out : (B, Tmax, D/nw) dtype
 *   status : int32 (B * D/nw): 0, or k = "k-th leading minor not positive
 *            definite" (linalg.pyx:79-82); may be NULL.
 */
int mlpg_hip_forward(int device, void *stream, int dtype, int algo,
                     const void *mean, const void *var, int var_mode,
                     const int32_t *lengths, int B, int Tmax, int D,
                     int num_windows, const int32_t *win_l_h,
                     const int32_t *win_u_h, const double *win_coef_h,
                     void *out, int32_t *status);

/*
 * The same call on HOST memory (numpy in, numpy out; no framework tensor in between): what a user of the
 * reference writes as a Python loop of paramgen.mlpg over a padded batch (util/__init__.py:44-66).  Synchronous.
 * The batch is cut into utterance chunks that alternate between two internal HIP streams, so that the host ->
 * device copy of one chunk, the kernels of another and the device -> host copy of a third overlap; pageable
 * memory is staged through pinned buffers by a few copy threads, memory from mlpg_hip_host_alloc (or any pinned /
 * registered host memory) is transferred in place.  All pointers are HOST pointers; shapes, dtypes, windows,
 * var_mode and status as for mlpg_hip_forward (lengths_h may be NULL).
 * A SMALL call -- at most 64 MB of input (MLPG_HIP_HOST_SMALL_MB) on one device: the literal per-utterance
 * paramgen.mlpg(mean_frames (T, D), variance_frames, windows) of the reference (_mlpg.py:92), 9.6 KB at T = 100 x 2 static
 * dims, 2.9 MB at T = 1000 x 60, and batches of a few utterances -- takes a short path instead: one stream, one cached pinned
 * staging buffer, no chunk plan and no thread; the arrays are staged and sent one behind the other (up to 48 KB the kernel reads
 * the pinned buffer itself), the kernel writes trajectory and verdicts straight into pinned host memory, and the host polls a
 * sequence number written behind them (round 6; mlpg_hip_launch_count(10 / 11) counts these calls).  An array of at least 1.2 MB
 * (MLPG_HIP_HOST_DIRECT_KB) that the library has been handed before (same address and size, one of its last 16), and any array of
 * at least 4 MB (MLPG_HIP_HOST_DIRECT_ALWAYS_KB), is not staged: the runtime copies it straight from -- the result: to -- the
 * caller's pageable memory at the pinned rate (mapping pages the device has never seen costs more than staging them, up to a few MB).
 * While the device works the calling thread touches the result array's pages (a store of 0 per page: the array must not overlap
 * the inputs), so that a fresh array's page faults are not taken one by one in the copy out (MLPG_HIP_HOST_PREFAULT=0: off).
 */
int mlpg_hip_forward_host(int device, int dtype, int algo, const void *mean_h,
                          const void *var_h, int var_mode,
                          const int32_t *lengths_h, int B, int Tmax, int D,
                          int num_windows, const int32_t *win_l_h,
                          const int32_t *win_u_h, const double *win_coef_h,
                          void *out_h, int32_t *status_h);

/*
 * mlpg_hip_fastdtw for N utterance pairs held in HOST memory: what DTWAligner.transform does per pair
 * (preprocessing/alignment.py:46-50: trim_zeros_frames on both utterances, fastdtw) for the whole batch, cut into
 * chunks of pairs that alternate between two internal streams (pinned staging, transfers under the kernels of the
 * other chunk), like mlpg_hip_forward_host.  X_h (N, Tx, D), Y_h (N, Ty, D) of `dtype` (float32 is widened to
 * float64 on the device: the distances are float64 either way).  lenx_h / leny_h: valid frames per utterance, or
 * both NULL: trailing frames with sum_d |x| < trim_eps are dropped on the device (preprocessing/generic.py:291-332,
 * eps 1e-7 there).  Outputs as mlpg_hip_fastdtw, in host memory; lenx_out_h / leny_out_h (may be NULL) receive the
 * lengths that were used.  Blocking; one host-entry call at a time per process.
 */
int mlpg_hip_fastdtw_host(int device, int dtype, const void *X_h, const void *Y_h,
                          const int32_t *lenx_h, const int32_t *leny_h, int N, int Tx, int Ty, int D,
                          int radius, int dist_kind, double dist_scale, int tie_rule, double trim_eps,
                          int32_t *path_i_h, int32_t *path_j_h, int32_t *path_len_h, double *cost_h,
                          int32_t *lenx_out_h, int32_t *leny_out_h);
/*
 * The two host-memory calls over SEVERAL devices from one process (the reference's batch loops --
 * util/__init__.py:44-66 over utterances, preprocessing/alignment.py:45 over pairs -- have no dependence between
 * items, so the batch shards with no exchange).  devices[0 .. num_devices): HIP device indices; NULL / 0: every visible
 * device.  Chunk c of the batch runs on list entry c % n, on that entry's stream pair slot (c / n) % 2; per device the
 * behaviour is the single-device call's, results and verdicts land at the chunk's own offset of the caller's arrays.
 * A device may be listed up to 4 times (each occurrence has its own staging buffers and streams).  On an error every
 * stream that was used is drained before the call returns.  mlpg_hip_forward_host(d, ...) == _multi(&d, 1, ...).
 * Environment (read once): MLPG_HIP_HOST_CHUNK_MB (input bytes per chunk, default 64), MLPG_HIP_HOST_COPY_THREADS (threads of the
 * staging copy, default 16, at most 64), MLPG_HIP_HOST_TRACE=1 (one line per call on stderr: where the calling thread and the
 * collector thread spent their time).
 */
int mlpg_hip_forward_host_multi(const int32_t *devices, int num_devices, int dtype, int algo, const void *mean_h,
                                const void *var_h, int var_mode, const int32_t *lengths_h, int B, int Tmax, int D,
                                int num_windows, const int32_t *win_l_h, const int32_t *win_u_h,
                                const double *win_coef_h, void *out_h, int32_t *status_h);
int mlpg_hip_fastdtw_host_multi(const int32_t *devices, int num_devices, int dtype, const void *X_h, const void *Y_h,
                                const int32_t *lenx_h, const int32_t *leny_h, int N, int Tx, int Ty, int D,
                                int radius, int dist_kind, double dist_scale, int tie_rule, double trim_eps,
                                int32_t *path_i_h, int32_t *path_j_h, int32_t *path_len_h, double *cost_h,
                                int32_t *lenx_out_h, int32_t *leny_out_h);
/*
 * The chunk dealing of the host-memory calls, as a pure function (no device needed): n_items utterances / pairs in
 * chunks of min(target_items, ceil(n_items / (4 * num_devices))) items (at least 4 chunks per device when the batch
 * allows).  Fills, for the first max_chunks chunks, the device-list entry, the stream slot, the first item and the
 * item count (any array may be NULL); returns the number of chunks, negative on bad arguments.
 */
long long mlpg_hip_host_chunk_plan(long long n_items, long long target_items, int num_devices, long long max_chunks,
                                   int32_t *entry, int32_t *slot, int64_t *first, int64_t *count);

/* Pinned host memory for arrays that are handed to mlpg_hip_forward_host repeatedly (transferred in place). */
void *mlpg_hip_host_alloc(size_t bytes);
void mlpg_hip_host_free(void *p);
/* Test aid, no GPU involved: dst[0, bytes) = src[0, bytes) by the short path's staging copy -- the calling thread and a few helper
 * threads (MLPG_HIP_HOST_HELPERS, default 3) share 64 KB slices claimed through one atomic word; the helpers spin for
 * MLPG_HIP_HOST_SPIN_US (default 250) after a copy, then sleep.  mlpg_hip_shutdown joins them. */
int mlpg_hip_host_copy(void *dst, const void *src, size_t bytes);

/*
 * Multi-stream MLPG forward over one padded acoustic feature batch (SURVEY 8(f)
 * rank 3).  Replaces the per-utterance, per-stream Python loop that users of
 * the reference write around paramgen.mlpg: util.apply_each2d_padded /
 * apply_each2d_trim (util/__init__.py:19-66) applied to each stream's column
 * slice of the (N, Tmax, D) zero-padded arrays that
 * datasets.PaddedFileSourceDataset.asarray produces (datasets/__init__.py:
 * 152-218), with the stream layout of util/files.py:90-115 (mgc | lf0 | vuv |
 * bap, each stream window-major: static, delta, delta-delta).
 *
 *   mean : (B, Tmax, ld_in) dtype; stream k occupies columns
 *          [in_col, in_col + max(num_windows,1)*static_dim)
 *   var  : MLPG_HIP_VAR_FRAME: (B, Tmax, ld_in), same columns;
 *          MLPG_HIP_VAR_GLOBAL: (ld_in,); MLPG_HIP_VAR_UNIT: NULL
 *   out  : (B, Tmax, ld_out) dtype; stream k's trajectory goes to columns
 *          [out_col, out_col + static_dim); other columns are not touched
 *   windows of stream k: entries win_first .. win_first+num_windows-1 of the
 *          packed tables (total_windows entries; several streams may share
 *          them).  num_windows == 0: no dynamic features, the static columns
 *          are copied through (frames >= lengths[b] zero-filled).
 *   status : int32 (B, sum_k static_dim), streams in table order; may be NULL.
 * The slices are consumed in place (no repacking).  Streams that share their
 * three windows (extents <= 1) are solved by ONE launch -- per-frame variances:
 * of the strip kernel; global (ld_in,) or unit variances (round 5): of the
 * constant-coefficient kernel -- their static dims side by side on the lanes; a
 * stream may be cut to fill the last 64-lane group, its remaining dims then run
 * as a launch of their own; every other stream is one launch.  A narrow stream (or
 * such a remainder) takes the strip kernel's
 * transposed form (see MLPG_HIP_ALGO_STRIP) behind the merged launch on `stream`.  Launches other than the widest go
 * to internal streams forked from and joined back into `stream` with events
 * (no host synchronisation; capturable): when the call returns, everything is
 * ordered on `stream`.  Which kernel solves a dim depends on the grouping, the
 * results agree to rounding (every kernel is held to the same parity bar).
 * Limits: 1 <= num_streams <= 64 (MLPG_HIP_EINVAL beyond), at most 4 streams
 * share one merged launch.  Everything is validated before the first launch,
 * a forced `algo` that one stream cannot take included (the error names the
 * stream and the family): a refused call writes nothing and launches nothing.
 */
typedef struct {
  int32_t in_col;      /* first column of the stream in mean / var rows  */
  int32_t out_col;     /* first column of its trajectory in out rows     */
  int32_t static_dim;  /* static feature dimension of the stream         */
  int32_t num_windows; /* 0 = pass-through                               */
  int32_t win_first;   /* first window of the stream in the window tables */
} mlpg_hip_stream_t;

int mlpg_hip_forward_streams(int device, void *stream, int dtype, int algo,
                             const void *mean, const void *var, int var_mode,
                             int64_t ld_in, const int32_t *lengths, int B,
                             int Tmax, int num_streams,
                             const mlpg_hip_stream_t *streams_h,
                             int total_windows, const int32_t *win_l_h,
                             const int32_t *win_u_h, const double *win_coef_h,
                             void *out, int64_t ld_out, int32_t *status);

/*
 * MLPG backward (gradient w.r.t. the means), batched.  Replaces
 * paramgen.mlpg_grad (paramgen/_mlpg.py:202-281; the reference solves a dense
 * T x T right-hand side with LAPACK dgbsv per static dim and window, :275).
 * Here: z = P_d^-1 o_d with the same banded factor as the forward, then
 *   grad[b, t, w*sd+d] = tau_w[t] * sum_k coeff_w[l_w+k] * z[t+k]      (O(T)).
 *
 *   var      : as in mlpg_hip_forward (in_dtype); grad_out : (B, Tmax, sd) in_dtype
 *   grad_mean: (B, Tmax, D) out_dtype (the reference returns float32, :248)
 * With var_mode == MLPG_HIP_VAR_UNIT this is also the backward of
 * autograd.UnitVarianceMLPG (autograd/_impl/mlpg.py:145-172: R^T . grad).
 */
int mlpg_hip_backward(int device, void *stream, int in_dtype, int out_dtype,
                      int algo, const void *var, int var_mode,
                      const void *grad_out, const int32_t *lengths, int B,
                      int Tmax, int D, int num_windows,
                      const int32_t *win_l_h, const int32_t *win_u_h,
                      const double *win_coef_h, void *grad_mean,
                      int32_t *status);

/*
 * MLPG backward w.r.t. the means AND the variances, batched: what the reference cannot do (autograd/_impl/mlpg.py:44 "we cannot
 * do MLPG on minibatch", and its backward returns no gradient for the variances) and what training a model that predicts a
 * variance per frame (mixture-density, heteroscedastic output layers) through MLPG needs.  For utterance b of length L and
 * static dim d:
 *   tau_w[t] = 1 / var[t, w*sd + d] in the input dtype; for w >= 1 zero where t < mw or t >= L - mw, mw = max_w max(l_w, u_w),
 *   and the whole column when mw == 0 (the reference's [-0:] slice); W_w truncated at 0 and L;
 *   P = sum_w W_w^T diag(tau_w) W_w,  y = P^-1 sum_w W_w^T (tau_w * mu_w),  g = dLoss/dy,  z = P^-1 g;
 *   grad_mean[t, w*sd+d] = tau_w[t] (W_w z)[t]                                   (= mlpg_hip_backward)
 *   dLoss/dtau_w[t]      = (W_w z)[t] (mu_w[t] - (W_w y)[t])
 *   grad_var[t, w*sd+d]  = -tau_w[t]^2 (W_w z)[t] (mu_w[t] - (W_w y)[t]) = -grad_mean[t, w*sd+d] tau_w[t] (mu_w[t] - (W_w y)[t])
 * grad_var is exactly 0 where the mask removes the precision (such var entries are never read: they may hold 0, a negative
 * value or NaN), in rows at and past L, and in every column of a system whose status is non-zero.  Since y does not change
 * when all variances of a system are scaled alike, sum_{w,t} var_w[t] grad_var_w[t] = 0 per system.
 *
 *   dtype    : MLPG_HIP_F32 or MLPG_HIP_F64 for every array; the gradients come back in it
 *   var_mode : MLPG_HIP_VAR_FRAME or MLPG_HIP_VAR_GLOBAL (MLPG_HIP_VAR_UNIT: MLPG_HIP_EINVAL, nothing to differentiate)
 *   mean, var: as in mlpg_hip_forward;  y (B, Tmax, sd): the trajectory mlpg_hip_forward returned for them;  grad_out (B, Tmax, sd)
 *   grad_mean (B, Tmax, D): bit-identical to mlpg_hip_backward(dtype, dtype, algo, ...) -- the same solve by the same route
 *   grad_var  (B, Tmax, D) in both modes; with global (D,) variances entry (b, t, c) is frame t's contribution to the gradient of
 *             the tiled vector: the gradient of the (D,) vector is its sum over b and t (the caller sums; no library scratch)
 *   status   : int32 (B * sd), required; filled as mlpg_hip_backward fills it
 * algo routes the solve as in mlpg_hip_backward (a forced kernel that cannot take the problem: MLPG_HIP_EINVAL, nothing is
 * launched); then ONE launch of the variance-gradient kernel on the same stream (mlpg_hip_launch_count(13)).  Allocates nothing
 * beyond what the solve's route uses; capturable into a HIP graph once that route's scratch exists.
 */
int mlpg_hip_backward_var(int device, void *stream, int dtype, int algo,
                          const void *mean, const void *var, int var_mode, const void *y,
                          const void *grad_out, const int32_t *lengths, int B, int Tmax, int D,
                          int num_windows, const int32_t *win_l_h, const int32_t *win_u_h,
                          const double *win_coef_h, void *grad_mean, void *grad_var, int32_t *status);

/*
 * Backward pass of mlpg_hip_forward_streams: the gradients of every stream of a multi-stream batch w.r.t. its means and (optionally)
 * its variances, written IN PLACE into the streams' own columns -- no slicing copies of the batch, of grad_out or of the gradients.
 * The stream table, the window tables and the layouts are those of mlpg_hip_forward_streams:
 *   mean, var, grad_mean, grad_var : (B, Tmax, ld_in); var (ld_in,) for MLPG_HIP_VAR_GLOBAL, NULL for MLPG_HIP_VAR_UNIT
 *   y, grad_out                    : (B, Tmax, ld_out), stream k at columns [out_col, out_col + static_dim); y is the trajectory
 *                                    the forward call returned
 *   status                         : int32 (B, sum static_dim), table order
 *   grad_var may be NULL: only the means get a gradient, and mean and y may then be NULL too.  A non-NULL grad_var with unit
 *   variances is MLPG_HIP_EINVAL; a non-NULL grad_var requires status.
 * A dynamic stream runs the backward solve of mlpg_hip_backward (same routing by `algo`, same launch counter, same status) on its
 * column slice: grad_mean columns [in_col, in_col + num_windows * static_dim), rows at and past lengths[b] zero.  A pass-through
 * stream (num_windows == 0) gets grad_mean = grad_out on live rows and 0 on padding, grad_var = 0, status = 0; its variance columns
 * are never read.  Columns of grad_mean / grad_var that belong to no stream are not touched.  grad_var follows the formula and the
 * zero rules of mlpg_hip_backward_var (masked entries -- never read --, padding, every column of a failing system); with global
 * variances it holds the per-frame contributions and the caller sums over (b, t).
 * Every launch goes on the caller's stream: the solves in table order, then the stream-table epilogue kernel (launch counter 15) --
 * one launch per distinct window list (win_first, num_windows) for the variance gradient of its streams, one launch for all
 * pass-through streams.  Everything is validated before the first launch: a stream that does not fit ld_in / ld_out, more than 64
 * streams, a bad dtype / mode / algo, or a forced `algo` that cannot take some dynamic stream (the error names the stream and the
 * algo) return MLPG_HIP_EINVAL with nothing launched, no output byte written and no counter moved (forced MLPG_HIP_ALGO_FIR: the
 * tap table of a window set is built on its first use, before the verdict).  Empty batches return 0.  Allocates nothing beyond the
 * scratch of the solve routes; capturable into a HIP graph once that scratch exists.
 */
int mlpg_hip_backward_streams(int device, void *stream, int dtype, int algo,
                              const void *mean, const void *var, int var_mode, int64_t ld_in,
                              const void *y, const void *grad_out, int64_t ld_out,
                              const int32_t *lengths, int B, int Tmax,
                              int num_streams, const mlpg_hip_stream_t *streams_h,
                              int total_windows, const int32_t *win_l_h, const int32_t *win_u_h,
                              const double *win_coef_h,
                              void *grad_mean, void *grad_var, int32_t *status);

/*
 * The same call on HOST memory (ABI 14): the literal paramgen.mlpg_grad(mean_frames, variance_frames, windows, grad_output) of the
 * reference (paramgen/_mlpg.py:202-281: numpy in, float32 numpy out; 0.8 ms there at T = 100 x 2 static dims, seconds at T = 1000 x
 * 60) and the backward of autograd.MLPG on CPU tensors (autograd/_impl/mlpg.py:57-67).  All pointers are HOST pointers: var_h /
 * grad_out_h of in_dtype, grad_h (B, Tmax, D) of out_dtype, status_h (B * D/nw, may be NULL), lengths_h may be NULL.  Synchronous.
 * The batch runs through the short path of mlpg_hip_forward_host -- one stream, cached pinned staging, up to 48 KB of input read
 * by the kernel in place, the gradient written by the kernel into pinned host memory, a polled sequence number -- in pieces of
 * whole utterances of at most MLPG_HIP_HOST_SMALL_MB of input, one after the other (the reference's call is one utterance; a large
 * batch belongs on mlpg_hip_backward).  mlpg_hip_launch_count(10 / 11) counts the pieces.
 */
int mlpg_hip_backward_host(int device, int in_dtype, int out_dtype, int algo,
                           const void *var_h, int var_mode, const void *grad_out_h,
                           const int32_t *lengths_h, int B, int Tmax, int D,
                           int num_windows, const int32_t *win_l_h,
                           const int32_t *win_u_h, const double *win_coef_h,
                           void *grad_h, int32_t *status_h);

/*
 * Delta features (the step BEFORE MLPG in every pipeline).  Replaces
 * preprocessing.delta_features (preprocessing/generic.py:229-288: a Python loop over feature
 * dims of np.correlate(x[:, d], window, "same")), batched:
 *   out[b, t, w*D + d] = sum_{k=-l_w}^{u_w} coeff_w[l_w + k] * x[b, t + k, d]      (x = 0 outside [0, len_b))
 * x : (B, Tmax, D) dtype, out : (B, Tmax, D*nw) dtype; accumulation in float64.  For a window
 * array of length L the reference's "same" correlation is l = L-1-(L-1)/2, u = (L-1)/2.
 */
int mlpg_hip_delta_features(int device, void *stream, int dtype, const void *x,
                            const int32_t *lengths, int B, int Tmax, int D,
                            int num_windows, const int32_t *win_l_h,
                            const int32_t *win_u_h, const double *win_coef_h,
                            void *out);

/*
 * Modulation spectrum of parameter trajectories (the step
 * after MLPG).  Replace preprocessing/modspec.py: modspec (:6-53: power of the
 * rfft along time), inv_modspec (:62-100: irfft of sqrt(ms) * phase),
 * modspec_smoothing (:103-167: remove the modulation-frequency bins >= limit_bin
 * -- in the log domain the removed log-power is set to 0, i.e. unit magnitude
 * with the original phase -- and transform back), and the gradient of the
 * power spectrum of autograd/_impl/modspec.py:30-60 (a Python loop over feature
 * dimensions with dense (n/2+1, T) cos/sin tables).
 * Any DFT length n >= 2, as numpy's rfft / irfft.  A power of two <= 4096 (the
 * reference's defaults are 2048 and 4096): one workgroup per (utterance, pair of
 * feature columns), the n-point FFT lives in LDS, one launch per call.  Any
 * other n <= 2048: the chirp-z (Bluestein) transform on the same FFT at length
 * M = 2^ceil(log2(2n - 1)) <= 4096, the same workgroup shape, two M-point FFTs
 * per workgroup (four for smoothing / backward); two small launches in front
 * build its tables (n + M complex values) in stream scratch on every call.
 * Every other n (no power of two above 2048, or n > 4096): the direct transform
 * (O(n) per output value, exact integer phases; two launches for smoothing /
 * backward, the half spectrum in stream scratch).
 * mlpg_hip_modspec_route(n): the route these four calls take at length n, a
 * function of n and of mlpg_hip_modspec_set_direct's switch alone -- 0 FFT,
 * 1 direct, 2 chirp-z, -1 for n < 2 (refused).  mlpg_hip_launch_count(20) counts
 * the calls the chirp-z route served.
 * All arrays float64, row-major; `ortho` selects numpy's norm="ortho".
 *   x     : (B, T, D), T <= n, zero-padded to n internally
 *   ms    : (B, n/2+1, D)            phase : (B, n/2+1, D, 2) (re, im), may be NULL
 *   inv_modspec output (B, n, D); smoothing / backward output (B, T, D)
 *   backward: grad_x[t] = C * sum_k grad_ms[k] (Re S_k cos(2 pi k t/n) - Im S_k sin(2 pi k t/n)),
 *             C = 2 (2/sqrt(n) for ortho), as modspec.py's analytic gradient.
 */
int mlpg_hip_modspec(int device, void *stream, const double *x, int B, int T,
                     int D, int n, int ortho, double *ms, double *phase);
int mlpg_hip_inv_modspec(int device, void *stream, const double *ms,
                         const double *phase, int B, int n, int D, int ortho,
                         double *x);
int mlpg_hip_modspec_smoothing(int device, void *stream, const double *x,
                               int B, int T, int D, int n, int ortho,
                               int limit_bin, int log_domain, double *out);
int mlpg_hip_modspec_backward(int device, void *stream, const double *x,
                              const double *grad_ms, int B, int T, int D,
                              int n, int ortho, double *grad_x);
/* Testing aid: on != 0 routes every DFT length through the direct transform
 * (process-wide), so that tests can compare it with the FFT and chirp-z paths. */
void mlpg_hip_modspec_set_direct(int on);
int mlpg_hip_modspec_route(int n);

/*
 * The modulation spectrum over a PADDED MINIBATCH, float32 or float64, and the fused log-MS loss step -- what follows the
 * batched MLPG calls in trajectory training:  loss = mse(y, target) + w * mse(log MS(y), log MS(target)).  The reference has
 * no such call: autograd/_impl/modspec.py:9-72 and preprocessing/modspec.py:6-53 take one (T, D) array, so a minibatch is a
 * Python loop over utterances.  `dtype` as in mlpg_hip_forward; x, ms, grad_ms, target_ms and grad_x are all of that dtype
 * (loaded and stored as such, arithmetic in float64).  All pointers are device pointers; every argument is checked before a
 * device is selected or anything is launched (MLPG_HIP_EINVAL, the text names the entry point); B == 0 or D == 0 returns 0 and
 * touches nothing.
 *   x        : (B, Tmax, D); Tmax is the row count and may exceed n
 *   lengths  : int32[B] or NULL (every utterance has Tmax frames).  Utterance b contributes the frames
 *              t < min(lengths[b], n, Tmax), as rfft(x[:len], n) with its crop at n.  What lies in the padding is never read.
 *   ms, grad_ms, target_ms : (B, n/2+1, D)
 *   grad_x   : (B, Tmax, D); EVERY row is written -- the gradient for live frames, 0 from min(lengths[b], n) on
 * Routes: a power of two n <= 4096 takes the in-LDS FFT kernel (mlpg_hip_launch_count(17)), any other n -- or every n after
 * mlpg_hip_modspec_set_direct(1) -- the direct transform (kind 18; at most 65535 utterances per call).
 *
 * mlpg_hip_modspec_loss_step (kind 19): with P = MS(x), f(P) = log(P + eps) (log_domain != 0) or P,
 *   loss   = sum (f(P) - f(target_ms))^2 / n_elems                        one float64
 *   grad_x = d loss / d x = backward of g = 2 (f(P) - f(target_ms)) f'(P) / n_elems
 * in one launch that keeps the spectrum in LDS (forward FFT, residual, inverse FFT) plus one small launch that adds the
 * workgroups' partial sums in a fixed order: the loss is the same bit for bit on every call.  `workspace`: at least
 * mlpg_hip_modspec_loss_workspace_bytes(B, D) bytes, 8-byte aligned, owned by the caller, content irrelevant, not to be shared
 * by calls that may overlap (the Python wrapper keeps one per (device, stream), allocated on first use and again when a batch
 * outgrows it: the wrapper's step is not capturable into a graph; the C call allocates nothing).  n_elems is normally
 * B * (n/2+1) * D.  mlpg_hip_modspec_loss_form(n): 1 when the step takes this
 * n (a power of two in [2, 4096] on the FFT route), 0 when the caller has to compose mlpg_hip_modspec_batch, its own loss
 * and mlpg_hip_modspec_batch_backward (any other n; every n after mlpg_hip_modspec_set_direct(1)).
 */
int mlpg_hip_modspec_batch(int device, void *stream, int dtype, const void *x,
                           const int32_t *lengths, int B, int Tmax, int D, int n,
                           int ortho, void *ms);
int mlpg_hip_modspec_batch_backward(int device, void *stream, int dtype,
                                    const void *x, const void *grad_ms,
                                    const int32_t *lengths, int B, int Tmax, int D,
                                    int n, int ortho, void *grad_x);
int mlpg_hip_modspec_loss_form(int n);
size_t mlpg_hip_modspec_loss_workspace_bytes(int B, int D);
int mlpg_hip_modspec_loss_step(int device, void *stream, int dtype, const void *x,
                               const void *target_ms, const int32_t *lengths, int B,
                               int Tmax, int D, int n, int ortho, int log_domain,
                               double eps, double n_elems, void *grad_x, double *loss,
                               void *workspace, size_t workspace_bytes);

/*
 * Trailing-zero trim.  Replaces preprocessing.trim_zeros_frames with trim="b"
 * (preprocessing/generic.py:291-332) applied to every utterance of a padded
 * (N, T, D) batch: lengths[n] = number of frames left after dropping trailing
 * frames whose sum_d |x| < eps.
 */
int mlpg_hip_trim_lengths(int device, void *stream, int dtype, const void *X,
                          int N, int T, int D, double eps, int32_t *lengths);

/*
 * fastdtw(x, y, radius, dist=L2) for N utterance pairs.  Replaces the
 * per-pair call in DTWAligner.transform (preprocessing/alignment.py:48-54;
 * fastdtw itself is the third-party package slaypni/fastdtw, see
 * oracle/dtw_oracle.c for the restated semantics and tie rule).
 *
 *   X : (N, Tx, D) float64, Y : (N, Ty, D) float64, lenx/leny : int32[N] valid
 *   frames (>= 1).  path_i/path_j : int32 (N, Tx+Ty) 0-based index pairs,
 *   path_len : int32[N] (0 if the pair failed), cost : float64[N] = accumulated
 *   distance D[len_x, len_y] (alignment.py:50, before the :51 normalisation).
 */
/* local distances of mlpg_hip_fastdtw */
#define MLPG_HIP_DIST_L2 0           /* sqrt(sum_k (x_k-y_k)^2), k ascending: DTWAligner's default dist
                                        (alignment.py:35: lambda x, y: norm(x - y)) in the oracle's summation order */
#define MLPG_HIP_DIST_SCALED_L2_NP 1 /* dist_scale * sqrt(((x-y)*(x-y)).sum()) with the sum in numpy's pairwise
                                        order (D <= 128): metrics.melcd(x, y) for two frames
                                        (metrics/__init__.py:27-59) with dist_scale = 10/ln(10)*sqrt(2) */
#define MLPG_HIP_DIST_SCALED_L1_NP 2 /* dist_scale * np.abs(x-y).sum(): city-block distance, numpy's pairwise order */
#define MLPG_HIP_DIST_SCALED_SQL2_NP 3 /* dist_scale * ((x-y)**2).sum(): squared Euclidean, numpy's pairwise order
                                        (what DTWAligner(dist=...) callables of those forms resolve to; the reference
                                        accepts any Python callable, alignment.py:35 -- the kernel evaluates the cost) */
/* tie rules of the DP recurrence D[i,j] = dt + min(D[i-1,j], D[i,j-1], D[i-1,j-1]) when candidates are EQUAL (after
 * adding dt).  The reference does not pin fastdtw's version, and the package ships two implementations of the
 * recurrence that differ only here; continuous data never tie, quantised or shifted-copy data
 * (tests/test_preprocessing.py:441-456 aligns zero-shifted copies) do. */
#define MLPG_HIP_TIE_FIRST_MIN 0 /* upstream's pure-Python __dtw: min(..., key=) keeps the FIRST minimum of
                                    (up, left, diagonal) -- the rule every parity test of this repo is pinned on */
#define MLPG_HIP_TIE_DIAG_LAST 1 /* the strict-less chain recalled for upstream's compiled _fastdtw: up only if it
                                    beats both others, else left only if it beats the diagonal, else the diagonal.
                                    UNVERIFIED: the package is absent from this image (and from /root/reference);
                                    tests/test_dtw_gpu.py reports which rule an installed fastdtw follows */
int mlpg_hip_fastdtw(int device, void *stream, const double *X,
                     const double *Y, const int32_t *lenx,
                     const int32_t *leny, int N, int Tx, int Ty, int D,
                     int radius, int dist_kind, double dist_scale,
                     int tie_rule, int32_t *path_i, int32_t *path_j,
                     int32_t *path_len, double *cost);
/*
 * fastdtw for `dist` callables no device-side cost reproduces (preprocessing/alignment.py:35-38 accepts ANY Python
 * callable): one resolution level at a time, the local costs evaluated on the host by the user's callable, the DP
 * recurrence, the back-trace and the window expansion (upstream's __expand_window in interval form) on the device.
 * The caller walks the levels from the coarsest to the finest (nnmnkwii_amd/preprocessing/alignment.py shows how):
 *
 *   mlpg_hip_dtw_level_windows   level_tx / level_ty: int32[N], the pair's lengths at THIS level (0: the pair's
 *       recursion has not reached the level yet, it is skipped); full[n] != 0: the pair's recursion bottoms out here
 *       (len < radius + 2: full window); otherwise the window comes from cpath_* = the pair's path at the level below
 *       (coarser), as mlpg_hip_dtw_level_from_costs left it.  Out: row_lo / row_hi (N, row_stride) inclusive column
 *       intervals, row_off (N, row_stride + 1) prefix sums of the widths (row_off[n, level_tx[n]] = cells of pair n).
 *   mlpg_hip_dtw_level_from_costs   costs: float64, pair n's cells at costs[cost_base[n] + row_off[n, i] + j - row_lo[n, i]]
 *       (total_cells doubles in all), max_ty >= every level_ty.  Out: path_i / path_j (N, path_stride), path_len[n]
 *       (0: the corner is unreachable), cost[n] = D[len_x, len_y].  tie_rule: MLPG_HIP_TIE_*.
 * All pointers are device pointers; both calls only enqueue work on `stream`.
 */
int mlpg_hip_dtw_level_windows(int device, void *stream, int N, int radius,
                               const int32_t *level_tx, const int32_t *level_ty,
                               const int32_t *full, const int32_t *cpath_i,
                               const int32_t *cpath_j, const int32_t *cpath_len,
                               int cpath_stride, int32_t *row_lo, int32_t *row_hi,
                               int64_t *row_off, int row_stride);
int mlpg_hip_dtw_level_from_costs(int device, void *stream, int N, int tie_rule,
                                  const int32_t *level_tx, const int32_t *level_ty,
                                  const int32_t *row_lo, const int32_t *row_hi,
                                  const int64_t *row_off, int row_stride, int max_ty,
                                  const double *costs, const int64_t *cost_base,
                                  int64_t total_cells, int32_t *path_i,
                                  int32_t *path_j, int32_t *path_len,
                                  int path_stride, double *cost);
/* = mlpg_hip_fastdtw(..., MLPG_HIP_DIST_L2, 1.0, MLPG_HIP_TIE_FIRST_MIN, ...) */
int mlpg_hip_fastdtw_l2(int device, void *stream, const double *X,
                        const double *Y, const int32_t *lenx,
                        const int32_t *leny, int N, int Tx, int Ty, int D,
                        int radius, int32_t *path_i, int32_t *path_j,
                        int32_t *path_len, double *cost);

/*
 * Frame-wise conversion under a joint source/target GMM.  Replaces the per-frame,
 * per-mixture Python loop of baseline/gmm.py:97-120 (MLPGBase.transform: np.linalg.solve(covarXX[m], x - mu_x[m])
 * for every frame and mixture) and :225-244 (MLPG.transform: the same for the most likely mixture of each frame):
 *   out[n, :] = sum_m posterior[n, m] * (mu_y[m] + A[m] (x[n] - mu_x[m])),     A[m] = covarYX[m] covarXX[m]^-1
 * x (N, D), posterior (N, M) or NULL, mixture int32 (N) (used when posterior is NULL: one mixture per frame),
 * mu_x (M, D), mu_y (M, Dy), A (M, Dy, D), out (N, Dy); all float64, row-major.  A is factored once per model by
 * the caller (host LAPACK); the mixture posteriors come from scikit-learn as in the reference.
 */
int mlpg_hip_gmm_convert(int device, void *stream, const double *x,
                         const double *posterior, const int32_t *mixture,
                         const double *mu_x, const double *mu_y,
                         const double *A, int64_t N, int D, int Dy, int M,
                         double *out);

/*
 * Float64 EM for full-covariance Gaussian mixtures on the device (K6, csrc/gmm_em.hip): scikit-learn's _e_step / _m_step
 * (sklearn/mixture/_base.py, _gaussian_mixture.py) restated step by step.  Limits: 1 <= F <= 128 features, 1 <= K <= 64
 * components, N >= 0 rows; all arrays float64, row-major, on the device.  Every argument is checked before a device is
 * selected; N == 0 returns 0 and touches nothing.  No floating-point atomics: two calls on the same inputs give the same bits.
 *
 * mlpg_hip_gmm_workspace_bytes: the workspace one fit of this shape needs (partial sums of the E-step's mean and of the
 * M-step's row slices; their number depends on (N, F, K) alone).  0 for sizes outside the limits.
 *
 * mlpg_hip_gmm_estep: X (N, F), weights (K), means (K, F), prec_chol (K, F, F) upper factors U with U U^T = Sigma^-1,
 * log_det (K) = sum_i log U_ii.  log p_nk = -(F log 2 pi + |(x_n - mu_k) U_k|^2) / 2 + log_det_k; with the log weights added,
 * log_prob_norm_n is their log-sum-exp over k and resp_nk = exp(log p_nk + log w_k - log_prob_norm_n).  Every output may be
 * NULL: resp (N, K), log_prob_norm (N), labels int32 (N) (the arg-max component, the first of equals), mean_log_prob (one
 * double: the mean of log_prob_norm; needs the workspace, which is not read otherwise).
 *
 * mlpg_hip_gmm_mstep: nk = sum_n resp_nk + 10 eps, means = sum_n resp_nk x_n / nk, covariances_k = sum_n resp_nk (x_n - mu_k)
 * (x_n - mu_k)^T / nk + reg_covar I with the new means, weights = nk / sum_k nk.  Outputs weights (K), means (K, F),
 * covariances (K, F, F) (exactly symmetric).
 *
 * mlpg_hip_gmm_precisions: per component the Cholesky factor L of the covariance, prec_chol = L^-T (exact zeros below the
 * diagonal), log_det, and status int32 (K): 0, or the 1-based index of a pivot that is <= 0 or NaN (LAPACK dpotrf's rule;
 * prec_chol and log_det of that component are then not written).
 */
size_t mlpg_hip_gmm_workspace_bytes(int64_t N, int F, int K);
int mlpg_hip_gmm_estep(int device, void *stream, const double *X,
                       const double *weights, const double *means,
                       const double *prec_chol, const double *log_det,
                       int64_t N, int F, int K, double *resp,
                       double *log_prob_norm, int32_t *labels,
                       double *mean_log_prob, void *workspace,
                       size_t workspace_bytes);
int mlpg_hip_gmm_mstep(int device, void *stream, const double *X,
                       const double *resp, int64_t N, int F, int K,
                       double reg_covar, double *weights, double *means,
                       double *covariances, void *workspace,
                       size_t workspace_bytes);
int mlpg_hip_gmm_precisions(int device, void *stream,
                            const double *covariances, int F, int K,
                            double *prec_chol, double *log_det,
                            int32_t *status);

/*
 * Float64 k-means for the start of that EM on the device (K7, csrc/kmeans.hip): the two steps scikit-learn's KMeans spends its
 * time in (sklearn/cluster/_kmeans.py: _kmeans_plusplus, _kmeans_single_lloyd), restated; the draws, the choice among the
 * candidates and the convergence test stay with the caller (nnmnkwii_amd.mixture.kmeans).  Limits: 1 <= F <= 128 features,
 * 1 <= K <= 64 clusters, 1 <= C <= 8 candidates, N >= 0 rows; all arrays row-major on the device, float64 unless said otherwise.
 * Every argument is checked before a device is selected; N == 0 returns 0 and touches nothing.  Both steps read X once, as
 * x - shift when shift (F doubles, the column means) is not NULL: X itself is never written.  No floating-point atomics: every
 * sum over rows is kept per slice of rows in row order and added over the slices in index order; two calls on the same inputs
 * give the same bits.
 *
 * mlpg_hip_kmeans_workspace_bytes: the workspace a fit of this shape needs, a function of the shape alone; 0 for sizes outside
 * the limits.  With S = min(max(ceil(N / 64), 1), 1024) slices (each ceil(ceil(N / 64) / S) tiles of 64 rows) and r(b) = b
 * rounded up to 256:  r(8 * 8 S) [the seed step's partial pots] + r(8 S K (F + 1)) [partial sums and counts] + r(8 S) [partial
 * inertia] + r(8 S) [partial changed-label counts] + r(8 K) [squared shift per cluster].
 *
 * mlpg_hip_kmeans_seed_step: candidates int32 (C) row indices on the device (an index outside [0, N) is clamped into it),
 * closest_in (N) or NULL.  d (C, N): d[j][n] = min(closest_in[n], sum_f (x_n - x_candidates[j])_f^2), without the minimum when
 * closest_in is NULL; pots (C): pots[j] = sum_n d[j][n].  Needs the first region of the workspace only (r(64 S) bytes).
 *
 * mlpg_hip_kmeans_lloyd_step: centers (K, F) (in the shifted frame), labels_prev int32 (N).  labels int32 (N): the arg-min over
 * k of |c_k|^2 - 2 (x_n - shift).c_k, the first of equals (labels may be labels_prev itself); min_dist (N) or NULL:
 * |x_n - shift - c_label|^2 as the direct sum over the features; sums (K, F) and counts (K): the rows of every cluster added up
 * and counted, not averaged; centers_out (K, F), written when update_centers != 0: sums / counts where the count is positive,
 * the old centre elsewhere (relocating an empty cluster is the caller's).  stats, 32 bytes, 8-byte aligned: double shift (sum_k
 * |centers_out_k - centers_k|^2 added in k order; 0 with update_centers == 0), double inertia (sum_n min_dist_n, computed
 * whether or not min_dist is stored), int64 changed (rows with labels != labels_prev), int64 empty (clusters with count 0).
 */
size_t mlpg_hip_kmeans_workspace_bytes(int64_t N, int F, int K);
int mlpg_hip_kmeans_seed_step(int device, void *stream, const double *X,
                              const double *shift, int64_t N, int F,
                              const int32_t *candidates, int C,
                              const double *closest_in, double *d,
                              double *pots, void *workspace,
                              size_t workspace_bytes);
int mlpg_hip_kmeans_lloyd_step(int device, void *stream, const double *X,
                               const double *shift, const double *centers,
                               const int32_t *labels_prev, int64_t N, int F,
                               int K, int update_centers, int32_t *labels,
                               double *min_dist, double *sums, double *counts,
                               double *centers_out, void *stats,
                               void *workspace, size_t workspace_bytes);

/*
 * The Merlin post-filter for mel-cepstra (K8, csrc/postfilter.hip; the reference's postfilters/__init__.py:7-62, whose four
 * SPTK operations -- freqt, c2acr, mc2b, b2mc -- are restated from their published definitions; parity with the pysptk package
 * itself is unpinned).  Per frame c of D coefficients, with v = weight * c:
 *   r0 = c2acr0(freqt(c, order, -alpha), fftlen), p0 = the same of v, b = mc2b(v, alpha), b[0] += log(r0 / p0) / 2,
 *   out = b2mc(b, alpha).
 * Limits, checked before a device is selected: 1 <= D <= 64, fftlen a power of two in [4, 4096], D - 1 <= order < fftlen,
 * |alpha| < 1.
 *
 * mlpg_hip_postfilter_table: host code, touches no device.  Writes G (fftlen/2 + 1, D) row-major float64 into HOST memory:
 * Re DFT_fftlen(freqt(c, order, -alpha))[k] = sum_d G[k][d] c[d] (csrc/postfilter_table.h).  The library keeps no copy.
 *
 * mlpg_hip_merlin_post_filter: mgc and out (B, Tmax, .) of `dtype` with row strides ld_in, ld_out >= D in elements (the mgc
 * columns of a wider multi-stream array are filtered where they lie; the utterance stride is Tmax * ld); out == mgc with equal
 * strides is allowed (a frame is read whole before it is written).  weight (D doubles) and G (the table above, built with the
 * same D, alpha and fftlen) are DEVICE pointers.  Arithmetic is float64, storage typed.  lengths: device int32 (B) or NULL; a
 * frame at or past min(max(len_b, 0), Tmax) is never loaded and the first D elements of its out row are written as exactly 0;
 * columns of out beyond D are never touched.  B == 0 or Tmax == 0 returns 0 and launches nothing.  One launch, a workgroup per
 * MLPG_HIP_POSTFILTER_FRAME_TILE frames; no atomics: two calls on the same inputs give the same bits.  The exponentials are not
 * rescaled: an input whose exp(2 L) overflows gives what the formula gives.
 */
#define MLPG_HIP_POSTFILTER_FRAME_TILE 64
int mlpg_hip_postfilter_table(int D, double alpha, int order, int fftlen,
                              double *G);
int mlpg_hip_merlin_post_filter(int device, void *stream, int dtype,
                                const void *mgc, int64_t ld_in,
                                const int32_t *lengths, int B, int Tmax, int D,
                                double alpha, const double *weight,
                                const double *G, int fftlen, void *out,
                                int64_t ld_out);

/*
 * The modulation-spectrum filter over a padded minibatch (K9, csrc/modspec_filter.hip): the MS post-filter of Takamichi et al.
 * (ICASSP 2014, TASLP 2016 -- the application the reference's preprocessing/modspec.py cites) and the low-pass smoothing of
 * modspec_smoothing (:103-167), either or both, in ONE launch (mlpg_hip_launch_count(31)).  The reference has no such call.
 * With live_b = min(max(lengths[b], 0), Tmax), nb = n/2 + 1, and for every column d < D:
 *   S = rfft(x[b, :live_b, d], n) (times 1/sqrt(n) if ortho), P = |S|^2;
 *   k <  limit_bin, tables given: S'_k = S_k * exp(((A[k,d] - 1) log P_k + C[k,d]) / 2), i.e. P'_k = exp(A log P_k + C) with the
 *                                 phase kept; a bin with P_k == 0 stays 0.  Without tables these bins are unchanged.
 *   k >= limit_bin:               the rule of mlpg_hip_modspec_smoothing -- log_domain != 0: unit magnitude with the phase kept
 *                                 (1 for a zero bin), else 0.  limit_bin == nb removes nothing.
 *   y = irfft(S', n) with the same norm; out[b, t, d] = y[t] for t < live_b and exactly 0 for live_b <= t < Tmax.
 * x, out: (B, Tmax, .) of `dtype` (float32 / float64 storage, float64 arithmetic) with row strides ld_x, ld_out >= D in elements
 * (a column slice of a wider matrix; the utterance stride is Tmax * ld); columns beyond D are never touched; a row at or past
 * live_b is never read.  out == x with equal strides is in place (a workgroup holds its two columns on the chip before it stores
 * them); any other overlap is the caller's error.  A, C: DEVICE float64 (nb, D) row-major, both or neither (NULL).  lengths:
 * device int32 (B) or NULL.  Tmax <= n is required.
 * mlpg_hip_modspec_filter_form(n): 1 for a power of two in [2, 4096] while mlpg_hip_modspec_set_direct's switch is off -- the
 * lengths the call takes; 0 otherwise (the caller composes mlpg_hip_modspec and mlpg_hip_inv_modspec).
 * Every argument is checked before a device is selected (MLPG_HIP_EINVAL, the text starts "modspec_filter:").  B == 0 or D == 0
 * returns 0 and touches nothing; Tmax == 0 writes nothing.  No atomics: two calls on the same inputs give the same bits.
 */
int mlpg_hip_modspec_filter_form(int n);
int mlpg_hip_modspec_filter(int device, void *stream, int dtype, const void *x,
                            int64_t ld_x, const int32_t *lengths, int B, int Tmax,
                            int D, int n, int ortho, const double *A,
                            const double *C, int limit_bin, int log_domain,
                            void *out, int64_t ld_out);

/*
 * The statistics of trajectory GMM conversion over a padded batch (K10, csrc/gmm_traj.hip; the reference's
 * baseline/gmm.py:225-247, MLPG.transform): ONE launch (mlpg_hip_launch_count(33)) turns source frames and their hard mixture
 * labels into the two inputs of mlpg_hip_forward.  All float64; row (b, t) of x, mean and var is at base + (b * Tmax + t) * ld
 * with row strides ld_x, ld_mean, ld_var >= D in elements (column slices of wider arrays, such as the source half of a joint
 * [x | y] matrix); columns D .. ld - 1 of mean and var are never touched.  labels int32 (B * Tmax), mu_x and mu_y (M, D),
 * A (M, D, D) = covarYX covarXX^-1 row-major, cvar (M, D) = the diagonal approximation of eq. 23 (gmm.py:245); lengths: device
 * int32 (B) or NULL (every row live).  With live_b = min(max(lengths[b], 0), Tmax):
 *   t <  live_b, m = labels[b * Tmax + t] in [0, M):   mean = mu_y[m] + A[m] (x - mu_x[m]),  var = cvar[m] (copied bit for bit);
 *   t <  live_b, m outside [0, M):                     the D elements of the mean row and of the var row are NaN (nothing is read
 *                                                      out of bounds; x of that row is not read);
 *   t >= live_b:                                       mean = 0 and var = 1 exactly; neither x nor the label of the row is read.
 * Limits: 1 <= D <= 128, 1 <= M <= 65536, B, Tmax >= 0.  Every argument is checked before a device is selected; B == 0 or
 * Tmax == 0 returns 0 and touches nothing.  A workgroup takes MLPG_HIP_GMM_TRAJ_ROW_TILE rows of the flattened (B * Tmax) axis.
 * No floating-point atomics and one summation order over k: a row's result does not depend on what else is in its tile or batch,
 * and two calls give the same bits.
 */
#define MLPG_HIP_GMM_TRAJ_ROW_TILE 64
int mlpg_hip_gmm_trajectory_stats(int device, void *stream, const double *x,
                                  int64_t ld_x, const int32_t *lengths, int B,
                                  int Tmax, int D, const int32_t *labels,
                                  const double *mu_x, const double *mu_y,
                                  const double *A, const double *cvar, int M,
                                  double *mean, int64_t ld_mean, double *var,
                                  int64_t ld_var);

/*
 * Parameter generation with the likelihood of the trajectory's gv (K11, csrc/mlpg_gv.hip; Toda, Black, Tokuda 2007, section
 * IV; the reference has no such call).  The gv of a system (utterance b, static dim d) with T = live_b frames is the variance
 * over time v(y) = (1/T) sum_t (y_t - m)^2, m = (1/T) sum_t y_t.  With P = sum_w W_w^T diag(tau_w) W_w and
 * r = sum_w W_w^T diag(tau_w) mu_w -- what mlpg_hip_forward assembles from mean, var, var_mode and the windows: the same
 * tau = 1/var per dtype, the same first and last frames -- and omega = omega_scale / (2 T):
 *   L(y) = omega (-1/2 y^T P y + y^T r) - 1/2 gv_prec[d] (v(y) - gv_mean[d])^2
 *   g(y) = omega (r - P y) - (2/T) gv_prec[d] (v(y) - gv_mean[d]) (y - m)
 * and the call runs y <- y + alpha g(y) n_iter times from the start: y_in as given (init 0), or scaled about its mean to the gv
 * gv_mean[d] (init 1; unchanged where v(y_in) or gv_mean[d] is not positive).  alpha = step where step > 0; else, per system,
 * alpha = 1 / (omega G + (2/T) gv_prec (|v - gv_mean| + 2 max(v, gv_mean))) at the start, G = max_t sum_j |P_tj| (a bound on the
 * curvature at the start: a heuristic, not a guarantee).  ONE launch (mlpg_hip_launch_count(35)) for all systems and all
 * iterations: one wavefront per system, its y, P and r in LDS, the halo by cross-lane moves; no atomics, and a system's bits do
 * not depend on the rest of the batch.
 * mean, var, var_mode, lengths, the windows: as mlpg_hip_forward.  y_in, y_out: (B, Tmax, D / num_windows) of `dtype` (float64
 * arithmetic); y_out == y_in is in place.  Frames at or past live_b of y_out are 0.  gv_mean, gv_prec: device float64
 * (D / num_windows).  report: device float64 (B * sd * 4): L(start), L(final), v(y_in), v(final); status: device int32 (B * sd):
 * 0 fine, 1 a non-finite value appeared, 2 L(final) < L(start) - 2^-40 max(|L(start)|, |L(final)|) (no ascent: the step is too
 * large).  A system with live_b = 0 gets report 0 and status 0.
 * Limits: window extents <= 1; Tmax <= mlpg_hip_gv_max_frames() (2048); n_iter in [0, 100000]; init 0 or 1; omega_scale > 0.
 * Anything else is refused with MLPG_HIP_EINVAL and a text that starts "gv_ascent:" before a device is selected, with nothing
 * launched.  An empty batch returns 0 and touches nothing.
 */
int mlpg_hip_gv_max_frames(void);
int mlpg_hip_gv_ascent(int device, void *stream, int dtype, const void *mean,
                       const void *var, int var_mode, const int32_t *lengths,
                       int B, int Tmax, int D, int num_windows,
                       const int32_t *win_l_h, const int32_t *win_u_h,
                       const double *win_coef_h, const void *y_in, void *y_out,
                       const double *gv_mean, const double *gv_prec,
                       double omega_scale, int n_iter, double step, int init,
                       double *report, int32_t *status);
/*
 * The gv of every (b, d) of a padded batch: x of `dtype`, row (b, t) at x + (b * Tmax + t) * ld_x, ld_x >= D; out float64
 * (B, D).  Two passes (mean, then squared deviations) over the live frames in frame order; live_b = 0 gives 0.  One launch
 * (mlpg_hip_launch_count(37)).
 */
int mlpg_hip_gv(int device, void *stream, int dtype, const void *x,
                int64_t ld_x, const int32_t *lengths, int B, int Tmax, int D,
                double *out);

/*
 * Corpus normalisation (csrc/colstats.hip; tools/norm_model.py is the executable specification).
 *
 * mlpg_hip_column_stats replaces the reference's host loops preprocessing/generic.py:496-549 (meanvar: one scikit-learn
 * _incremental_mean_and_var call per utterance), :552-602 (meanstd) and :605-636 (minmax: a second pass) with ONE pass over a
 * padded batch: x of `dtype`, row (b, t) at x + (b * Tmax + t) * ld_x, ld_x >= D (a column slice of a wider array is fine);
 * lengths: device int32 (B) or NULL; frames at or past live_b = min(max(lengths[b], 0), Tmax) are never read.  state_in,
 * state_out: device float64 (5, D), rows count, mean, M2 = sum (x - mean)^2, min, max over every live frame seen so far;
 * state_in NULL is the empty state (0, 0, 0, +inf, -inf), state_in == state_out is allowed, and the incoming state is merged
 * first.  Arithmetic is float64.  A column that is constant over the live frames gives mean == the constant and M2 == 0
 * exactly; a column with a non-finite live value gives mean = M2 = NaN; min and max propagate NaN as np.minimum / np.maximum.
 * A workgroup takes MLPG_HIP_COLSTATS_BLOCK_ROWS frames of one utterance in chunks of MLPG_HIP_COLSTATS_CHUNK_ROWS and writes
 * its partial state to `workspace` (device memory, at least mlpg_hip_column_stats_workspace(B, Tmax, D) bytes, 8-byte
 * aligned); a second small launch merges the partials in a fixed order.  No atomics, no synchronisation with the host, and a
 * division of the work that depends on (B, Tmax, D) alone: the same bits on every call and every device, and the call can be
 * captured into a graph.  B == 0 or Tmax == 0 with D > 0 still writes state_out (state_in, or the empty state); D == 0
 * returns 0.  mlpg_hip_launch_count(39) counts the calls that launched.
 * mlpg_hip_column_stats_workspace: host code, touches no device; -1 if a size is negative or the byte count does not fit.
 *
 * mlpg_hip_column_affine replaces :639-665 (scale), :668-684 (inv_scale), :734-786 (minmax_scale) and :789-828
 * (inv_minmax_scale): mode 0  y = (x - c[d]) / a[d],  mode 1  y = a[d] * x + c[d]  in float64 with separate operations
 * (float64 results equal numpy's bit for bit), rounded once to out_dtype.  a, c: device float64 (D).  x of in_dtype with row
 * stride ld_x, y of out_dtype with row stride ld_y, both >= D; y == x (one dtype, equal strides) is in place.  Rows at or past
 * live_b are never read and come out as exact zeros in columns 0 .. D - 1; columns past D are never touched.  One launch
 * (mlpg_hip_launch_count(41)).  Apart from y == x, the elements of y must not overlap those of x (other columns of the same
 * wide array are fine): that is the caller's duty, the call cannot tell such slices from overlapping ones and checks nothing.
 *
 * Refused with MLPG_HIP_EINVAL before a device is selected, with nothing launched, in a text that starts "column_stats:" /
 * "column_affine:": a dtype other than MLPG_HIP_F32 / _F64, a negative size, a row stride below D, a device outside [0, 16), a
 * required pointer that is NULL, a workspace that is too small or not 8-byte aligned, a mode other than 0 or 1.
 */
#define MLPG_HIP_COLSTATS_CHUNK_ROWS 16
#define MLPG_HIP_COLSTATS_BLOCK_ROWS 512
int64_t mlpg_hip_column_stats_workspace(int B, int Tmax, int D);
int mlpg_hip_column_stats(int device, void *stream, int dtype, const void *x,
                          int64_t ld_x, const int32_t *lengths, int B, int Tmax,
                          int D, const double *state_in, double *state_out,
                          void *workspace, int64_t workspace_bytes);
int mlpg_hip_column_affine(int device, void *stream, int in_dtype,
                           int out_dtype, int mode, const void *x, int64_t ld_x,
                           void *y, int64_t ld_y, const int32_t *lengths, int B,
                           int Tmax, int D, const double *a, const double *c);

/*
 * Gather rows along the warping path into zero-padded outputs.  Replaces
 * alignment.py:52-54,72-73:  out[n, k, :] = src[n, path[n, k], :] for
 * k < path_len[n], zeros after.  src (N, Tsrc, D), out (N, Tout, D), same dtype.
 */
int mlpg_hip_gather_path(int device, void *stream, int dtype, const void *src,
                         const int32_t *path, const int32_t *path_len, int N,
                         int Tsrc, int path_stride, int D, int Tout, void *out);

#ifdef __cplusplus
}
#endif
#endif /* MLPG_HIP_H_ */
