// Shared host/device definitions for libmlpg_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <mutex>

#include "../../include/mlpg_hip.h"

namespace mlpg {

constexpr int kMaxWindows = 8;
constexpr int kMaxCoef = 48;   // sum over windows of (l+u+1)
constexpr int kMaxExtent = 4;  // max l or u of any window (half-bandwidth <= 8)

// Window table passed BY VALUE as a kernel argument (lands in SGPRs / the
// kernarg segment; no device allocation, no __constant__ upload to order).
struct WinSet {
  int nw;
  int q;   // half-bandwidth of P: max_w (l_w + u_w)            (_mlpg.py:72-73)
  int mw;  // edge width: max_w max(l_w, u_w)                   (_mlpg.py:177)
  int l[kMaxWindows];
  int u[kMaxWindows];
  int off[kMaxWindows];  // offset of window w's coefficients in c[]
  double c[kMaxCoef];
};

// Problem description shared by the forward and backward kernels.
struct Problem {
  const void *mean;      // (B, Tmax, D)   forward only
  const void *var;       // per var_mode
  const void *grad_out;  // (B, Tmax, sd)  backward only
  const int32_t *lengths;
  void *out;             // forward: (B, Tmax, sd); backward: (B, Tmax, D)
  int32_t *status;
  int var_mode;
  int B, Tmax, D, sd;
  // Columns between a dim's windows in a row; 0 = sd.  Differs from sd when the problem is a PIECE of a stream (some of
  // its static dims: mlpg_hip_forward_streams cuts streams to fill lane groups): forward pass on the wave-per-system
  // and the natural-order kernels only.
  int pitch = 0;
  // Row strides in elements; the utterance stride is Tmax * row stride (the parent array is a
  // densely packed (B, Tmax, ld) batch of which this problem is a column slice: one stream of a
  // multi-stream acoustic feature matrix).  Dense problems: ld_in = D, ld_gout = sd,
  // ld_out = sd (forward) | D (backward), ld_status = sd.
  long ld_in;     // mean and per-frame var rows
  long ld_gout;   // grad_out rows (backward)
  long ld_out;    // out rows
  int ld_status;  // status[b * ld_status + d]
};

// Several streams of one (B, Tmax, ld) batch solved by ONE strip-kernel launch: their static dims sit side by side on
// the lanes (merged index begin[s] .. begin[s+1]).  Columns are absolute in the parent arrays; unused entries of
// begin[] are INT_MAX.
struct StreamMap {
  int n, total;
  int begin[4], in_col[4], sd[4], out_col[4], stat_col[4];
  // Transposed form (tr_u > 0; strip kernel, round 5): ONE narrow stream whose lanes run over tr_u consecutive UTTERANCES x its
  // tr_nd static dims (lane = u * tr_nd + d; total = tr_u * tr_nd <= 64), so that a stream of 1 .. 32 dims fills the 64 lanes
  // it would otherwise leave idle.  A system group is then a block of tr_u utterances (tr_B utterances in all: the last block may
  // be short); sd[0] is the window pitch, in_col[0] / out_col[0] / stat_col[0] the stream's columns, and tr_in / tr_out / tr_stat
  // the element strides from one utterance to the next in the input, output and status arrays.  With a lengths vector the group
  // runs to its longest utterance and every lane masks its own dead frames (strip::assemble_eliminate<..., LT>).
  int tr_u, tr_nd, tr_B, tr_in, tr_out, tr_stat;
};

// The strip, constant-coefficient and chunked kernels address an utterance's rows through a buffer descriptor with 32-bit byte
// offsets from the utterance's first row (2 GB window): longer utterances (Tmax * row stride * 8 bytes) go to the natural-order kernel.
inline bool rows_fit_buffer(const Problem &p) {
  const long ld = p.ld_in > p.ld_out ? (p.ld_in > p.ld_gout ? p.ld_in : p.ld_gout) : (p.ld_out > p.ld_gout ? p.ld_out : p.ld_gout);
  return (double)p.Tmax * (double)ld * 8.0 < 2147483647.0;
}

void set_error(const char *fmt, ...);

// ---- the host layer's shared pieces (capi.hip; used by the entry points of capi.hip, streams_api.hip and host_api.hip) ----
constexpr int kMaxDevices = 16;  // device indices the entry points accept
// The dense problem of the rule above: mean / grad_out (B, Tmax, D | sd) in, out (B, Tmax, sd | D).
inline Problem dense_problem(const void *mean, const void *var, const void *grad_out, const int32_t *lengths, void *out,
                             int32_t *status, bool backward, int var_mode, int B, int Tmax, int D, int sd) {
  Problem p;
  p.mean = mean;
  p.var = var;
  p.grad_out = grad_out;
  p.lengths = lengths;
  p.out = out;
  p.status = status;
  p.var_mode = var_mode;
  p.B = B;
  p.Tmax = Tmax;
  p.D = D;
  p.sd = sd;
  p.ld_in = D;
  p.ld_gout = backward ? sd : 0;
  p.ld_out = backward ? D : sd;
  p.ld_status = sd;
  return p;
}
// One-line argument checks: 0, or MLPG_HIP_EINVAL with the error text "<who>: ..." set (who: the entry point's name).
int check_dtype(const char *who, int dtype);
int check_var(const char *who, int var_mode, const void *var);  // var_mode in range, and an array unless the variances are unit
int check_device(const char *who, int device);                  // device in [0, kMaxDevices): asked before the runtime is touched
// Window tables -> WinSet (extents and the coefficient count are checked).
int pack_windows(int nw, const int32_t *wl, const int32_t *wu, const double *wc, WinSet *ws);
// Offset of window win_first's coefficients in a packed coefficient table; the extents of the windows in front are checked on the way.
int coef_offset(const char *who, const int32_t *wl, const int32_t *wu, int win_first, size_t *off);
// Makes `device` current for the scope; rc != 0 (error text set): it could not -- `DeviceGuard g(who, device); if (g.rc) return g.rc;`.
struct DeviceGuard {
  int prev = -1, target = -1, rc = 0;
  DeviceGuard(const char *who, int device) : target(device) {
    if (hipGetDevice(&prev) != hipSuccess || (device != prev && hipSetDevice(device) != hipSuccess)) {
      set_error("%s: cannot select device %d", who, device);
      rc = MLPG_HIP_ERUNTIME;
    }
  }
  ~DeviceGuard() {
    if (prev >= 0 && prev != target) (void)hipSetDevice(prev);
  }
};
// Which kernel family takes a problem, and the launch of it (capi.hip: kernel choice in one place).  check_algo: can the family `algo`
// names take this problem?  Pure host logic -- what dispatch_solve refuses before it launches anything.
int check_algo(int in_dtype, int out_dtype, int algo, const Problem &p, const WinSet &ws);
bool takes_strip_tr(int dtype, int algo, const Problem &p, const WinSet &ws);  // will dispatch_solve's first choice be the transposed strip form?
int dispatch_solve(hipStream_t st, int in_dtype, int out_dtype, int algo, bool backward, const Problem &p, const WinSet &ws, int device);
// Side streams for the independent streams of one multi-stream call (per device, created once; nullptr: none to be had).
struct SideStreams {
  static constexpr int kN = 3;
  hipStream_t st[kN];
  hipEvent_t fork, join[kN];
  std::mutex mu;  // held by mlpg_hip_forward_streams while it enqueues (two host threads on one device)
};
SideStreams *side_streams(int device);
// launches per kernel family since the library was loaded (mlpg_hip_launch_count: a test aid)
// (kinds 12 and 14 count nothing and read -1; 13: the variance-gradient epilogue of mlpg_hip_backward_var; 15: the stream-table
// epilogue of mlpg_hip_backward_streams; 16 counts nothing and reads -1; 17: the typed in-LDS FFT kernel of mlpg_hip_modspec_batch /
// _batch_backward; 18: their direct transform; 19: the fused loss kernel of mlpg_hip_modspec_loss_step; 20: calls of the float64 modulation-spectrum entries that
// the chirp-z kernel of modspec_chirp.hip served; 21 counts nothing and reads -1; 22, 23, 24: calls of mlpg_hip_gmm_estep, _mstep and
// _precisions that launched their kernels (gmm_em.hip); 25 counts nothing and reads -1; 26, 27: calls of mlpg_hip_kmeans_seed_step and
// _lloyd_step that launched their kernels (kmeans.hip); 28 counts nothing and reads -1; 29: calls of mlpg_hip_merlin_post_filter that
// launched (postfilter.hip); 30 counts nothing and reads -1; 31: launches of the kernel of mlpg_hip_modspec_filter (modspec_filter.hip); 32 counts nothing and reads -1; 33: launches of the
// kernel of mlpg_hip_gmm_trajectory_stats (gmm_traj.hip); 34 and 36 count nothing and read -1; 35: launches of the kernel of
// mlpg_hip_gv_ascent, 37: of mlpg_hip_gv (mlpg_gv.hip); 38 and 40 count nothing and read -1; 39: calls of mlpg_hip_column_stats that
// launched, 41: of mlpg_hip_column_affine (colstats.hip))
enum { kCountGeneric = 0, kCountWave, kCountStrip, kCountStripMulti, kCountConst, kCountFused, kCountChunk, kCountFir, kCountConstMulti, kCountStripTr, kCountHostSmall, kCountHostSmallDirect, kCountUnused12, kCountVarGrad, kCountUnused14, kCountStreamsBwd, kCountUnused16, kCountModspecBatch, kCountModspecBatchDft, kCountModspecLoss, kCountModspecChirp, kCountUnused21, kCountGmmEstep, kCountGmmMstep, kCountGmmPrecisions, kCountUnused25, kCountKmeansSeed, kCountKmeansLloyd, kCountUnused28, kCountPostfilter, kCountUnused30, kCountModspecFilter, kCountUnused32, kCountGmmTraj, kCountUnused34, kCountGvAscent, kCountUnused36, kCountGv, kCountUnused38, kCountColStats, kCountUnused40, kCountColAffine, kCountKinds };
void note_launch(int kind);
// Grow-only scratch, cached per (device, stream, slot): slot 0 generic factor, 1 fastdtw pyramids,
// 2 generic status, 3 strip records, 4 constant-coefficient kernel (factor table), 5 fastdtw from host costs (D rows, back-pointers), 6 chunked kernel (records, block factors, separator solutions, marks).  Returns nullptr (and sets the error) on failure.
void *scratch(int device, hipStream_t stream, int slot, size_t bytes, unsigned long long *gen = nullptr);

// launchers (one per translation unit)
int launch_generic(hipStream_t s, int dtype, int out_dtype, bool backward, const Problem &p, const WinSet &w,
                   int device);
bool generic_grid_fits(const Problem &p);                   // the natural-order kernel's grids are ones a launch takes
bool elementwise_grid_fits(int B, int Tmax, int cols);      // ... and the one-thread-per-element grid of delta_features / copy_cols
bool wave_supported(const Problem &p, const WinSet &w);
int launch_wave(hipStream_t s, int dtype, int out_dtype, bool backward, const Problem &p, const WinSet &w,
                int device);
bool strip_supported(const Problem &p, const WinSet &w);
bool strip_preferred(const Problem &p, const WinSet &w, bool backward, int in_dtype);
bool strip_tr_supported(const Problem &p, const WinSet &w, bool backward, int in_dtype, int out_dtype);
bool strip_tr_preferred(const Problem &p, const WinSet &w, bool backward, int in_dtype, int out_dtype);
int launch_strip_tr(hipStream_t s, int dtype, const Problem &p, const WinSet &w, int device);
int launch_strip(hipStream_t s, int dtype, int out_dtype, bool backward, const Problem &p, const WinSet &w,
                 int device, bool try_tr = true);
// (launch_strip_multi returns strip::kNotResident, mlpg_strip_geom.h, if fewer workgroups can be resident than an utterance has strips)
// forward pass of several streams (p: the parent arrays, sd/D unused) -- per-frame variances, three windows of extent <= 1
int launch_strip_multi(hipStream_t s, int dtype, const Problem &p, const WinSet &w, const StreamMap &sm, int device);
bool unit_mse_supported(int Tmax, const WinSet &w);
long unit_mse_workgroups(int B, int sd);  // the one-launch kernel's grid (256 threads per workgroup)
size_t unit_mse_workspace_bytes(int B, int sd);
int launch_unit_mse(hipStream_t s, int dtype, const Problem &p, const WinSet &w, const void *target, void *y_out,
                    double n_elems, double *loss, void *workspace);
bool const_supported(const Problem &p, const WinSet &w);
// true once per scratch allocation (device, stream): the constant-coefficient kernel's table holds nothing yet
bool const_scratch_fresh(int device, hipStream_t stream, unsigned long long gen);
// unit variances: true if this (device, stream) last built its table from the same key on the same scratch allocation
bool const_unit_table_cached(int device, hipStream_t stream, unsigned long long gen, bool fresh, const double *key, int n);
// strip kernel: do the workgroups of a launch on the current device spread evenly over eight XCDs (HW_REG_XCC_ID)?  Probed once
// per device with a small kernel (mlpg_strip.hip); false while `st` is being captured and the device has not been probed yet.
bool strip_xcd_lists_ok(hipStream_t st);
bool const_preferred(const Problem &p, const WinSet &w);
int launch_const(hipStream_t s, int dtype, int out_dtype, bool backward, const Problem &p, const WinSet &w, int device);
int launch_const_multi(hipStream_t s, int dtype, const Problem &p, const WinSet &w, const StreamMap &sm, int device);
bool chunk_supported(const Problem &p, const WinSet &w);
bool chunk_grid_fits(const Problem &p, const WinSet &w);    // its grids are ones a launch takes (chunk_supported asks)
bool chunk_preferred(const Problem &p, const WinSet &w, bool backward);
int launch_chunk(hipStream_t s, int dtype, int out_dtype, bool backward, const Problem &p, const WinSet &w, int device);
int launch_chunk_fwd_f64(hipStream_t s, const Problem &p, const WinSet &w, int device);
int launch_chunk_fwd_f32(hipStream_t s, const Problem &p, const WinSet &w, int device);
int launch_chunk_bwd_f64(hipStream_t s, const Problem &p, const WinSet &w, int device);
int launch_chunk_bwd_f32(hipStream_t s, const Problem &p, const WinSet &w, int device);
// unit variances on float32 tensors as a FIR filter; launch_fir returns kFirNotApplicable when the window set's inverse does not decay
// fast enough (or its tap table cannot be built now: stream capture)
constexpr int kFirNotApplicable = -2000;
bool fir_shape_supported(const Problem &p, const WinSet &w, int in_dtype, int out_dtype);
long fir_workgroups(const Problem &p);  // the largest grid the form launches for p (512 threads per workgroup)
bool fir_grid_fits(const Problem &p);   // ... is one a launch takes (fir_shape_supported asks)
bool fir_preferred(const Problem &p, bool backward);
bool fir_table_ready(hipStream_t s, int device, const WinSet &w);
void fir_shutdown();
int launch_fir(hipStream_t s, bool backward, const Problem &p, const WinSet &w, int device);
size_t fir_mse_workspace_bytes(int B, int Tmax, int sd);
int launch_fir_mse(hipStream_t s, const Problem &p, const WinSet &w, int device, const void *target, void *y_out, double n_elems,
                   double *loss, void *workspace);
int launch_copy_cols(hipStream_t s, int dtype, const void *src, long ld_src, const int32_t *lengths, int B, int Tmax,
                     int ncols, void *dst, long ld_dst);
int launch_stream_copy(hipStream_t s, const void *src, void *dst, size_t nbytes);
int launch_modspec(hipStream_t s, int mode, const double *x, const double *ms, const double *ph, double *out,
                   double *out_ph, int B, int T, int D, int n, int ortho, int limit_bin, int log_domain);
void host_api_shutdown();  // host_api.hip: streams, events, pinned and device staging buffers of the _host entry points
int launch_modspec_dft(hipStream_t s, int device, int mode, const double *x, const double *ms, const double *ph,
                       double *out, double *out_ph, int B, int T, int D, int n, int ortho, int limit_bin,
                       int log_domain);
// modspec_chirp.hip: the same four modes at a DFT length in [3, 2048] that is no power of two (chirp-z on the in-LDS FFT; the two
// tables go to scratch slot 0 of the stream)
bool modspec_chirp_takes(int n);
int modspec_chirp_length(int n);  // M = 2^ceil(log2(2n - 1)), the length of its circular convolution
int launch_modspec_chirp(hipStream_t s, int device, int mode, const double *x, const double *ms, const double *ph, double *out,
                         double *out_ph, int B, int T, int D, int n, int ortho, int limit_bin, int log_domain);
// padded minibatches, float32 / float64 (modspec_api.hip): mode 0 spectrum, 1 gradient (aux: grad_ms), 2 -- FFT form only -- the fused
// loss step (aux: target_ms; partial: one double per workgroup, B * ceil(D / 2); loss: one double)
bool modspec_fft_takes(int n);  // a power of two in [2, 4096]: the in-LDS FFT
bool modspec_direct();          // mlpg_hip_modspec_set_direct's switch
int launch_modspec_batch(hipStream_t s, int mode, int dtype, const void *x, const void *aux, const int32_t *lengths, void *out,
                         int B, int Tmax, int D, int n, int ortho, int log_domain, double eps, double n_elems, double *partial,
                         double *loss);
int launch_modspec_dft_batch(hipStream_t s, int device, int mode, int dtype, const void *x, const void *grad_ms,
                             const int32_t *lengths, void *out, int B, int Tmax, int D, int n, int ortho);
int launch_delta(hipStream_t s, int dtype, const void *x, const int32_t *lengths, int B, int Tmax, int D,
                 const WinSet &w, void *out);
// mlpg_vargrad.hip: grad_var from grad_mean, var, mean and y behind the backward solve (one launch, kind kCountVarGrad)
int launch_var_grad(hipStream_t s, int dtype, const void *grad_mean, const void *var, int var_mode, const void *mean,
                    const void *y, const int32_t *lengths, const int32_t *status, int B, int Tmax, int sd, const WinSet &w,
                    void *grad_var);
// mlpg_streams_bwd.hip: the member streams of one epilogue launch of mlpg_hip_backward_streams, their static dims side by side on
// a merged index (member m: [begin[m], begin[m] + sd[m])); columns are absolute in the parent arrays.  Passed by value.
constexpr int kMaxStreams = 64;
struct ColTable {
  int n, total;
  int begin[kMaxStreams], in_col[kMaxStreams], out_col[kMaxStreams], sd[kMaxStreams], stat_col[kMaxStreams];
};
constexpr int kStreamsBwdPass = 3;  // launch_streams_bwd's mode for pass-through members (otherwise MLPG_HIP_VAR_FRAME / _GLOBAL)
bool streams_bwd_fits(int B, int Tmax, int total);
// One launch (kind kCountStreamsBwd).  Dynamic members (one window list): grad_var from grad_mean, var, mean and y behind their
// solves; pass-through members: grad_mean = grad_out (0 on padding), grad_var = 0 where given, status = 0 where given.
int launch_streams_bwd(hipStream_t s, int dtype, int mode, const void *grad_out, const void *var, const void *mean, const void *y,
                       const int32_t *lengths, int32_t *status, int B, int Tmax, long ld_in, long ld_out, int ld_status,
                       const ColTable &ct, const WinSet &w, void *grad_mean, void *grad_var);
int launch_trim(hipStream_t s, int dtype, const void *X, int N, int T, int D, double eps, int32_t *lengths);
int launch_fastdtw(hipStream_t s, int device, const double *X, const double *Y, const int32_t *lenx,
                   const int32_t *leny, int N, int Tx, int Ty, int D, int radius, int dist_kind, double dist_scale,
                   int tie_rule, int32_t *path_i, int32_t *path_j, int32_t *path_len, double *cost);
int launch_dtw_window(hipStream_t s, int device, int N, int radius, const int32_t *ltx, const int32_t *lty,
                      const int32_t *full, const int32_t *cpath_i, const int32_t *cpath_j, const int32_t *cpath_len,
                      int cpath_stride, int32_t *row_lo, int32_t *row_hi, int64_t *row_off, int row_stride);
int launch_dtw_costs(hipStream_t s, int device, int N, int tie_rule, const int32_t *ltx, const int32_t *lty,
                     const int32_t *row_lo, const int32_t *row_hi, const int64_t *row_off, int row_stride, int max_ty,
                     const double *costs, const int64_t *cost_base, int64_t total_cells, int32_t *path_i, int32_t *path_j,
                     int32_t *path_len, int path_stride, double *cost_out);
int launch_gmm_convert(hipStream_t s, const double *x, const double *post, const int32_t *mix, const double *mu_x,
                       const double *mu_y, const double *A, long N, int D, int Dy, int M, double *out);
// postfilter.hip: the Merlin post-filter over the frames of a padded batch, one launch (kind kCountPostfilter)
int launch_postfilter(hipStream_t s, int dtype, const void *mgc, long ld_in, const int32_t *lengths, int B, int Tmax, int D,
                      double alpha, const double *weight, const double *G, int fftlen, void *out, long ld_out);
// gmm_traj.hip: conditional means and variances of trajectory GMM conversion over a padded batch, one launch (kind kCountGmmTraj)
int launch_gmm_traj(hipStream_t s, const double *x, long ld_x, const int32_t *lengths, int B, int Tmax, int D, const int32_t *labels,
                    const double *mu_x, const double *mu_y, const double *A, const double *cvar, int M, double *mean, long ld_mean,
                    double *var, long ld_var);
// colstats.hip: column statistics of a padded batch (the statistics kernel and its finish step; kind kCountColStats) and the
// per-column affine map (one launch, kind kCountColAffine)
int launch_colstats(hipStream_t s, int dtype, const void *x, long ld_x, const int32_t *lengths, int B, int Tmax, int D,
                    const double *state_in, double *state_out, double *workspace);
int launch_colaffine(hipStream_t s, int in_dtype, int out_dtype, int mode, const void *x, long ld_x, void *y, long ld_y,
                     const int32_t *lengths, int B, int Tmax, int D, const double *a, const double *c);
int launch_gather(hipStream_t s, int dtype, const void *src, const int32_t *path, const int32_t *path_len, int N,
                  int Tsrc, int path_stride, int D, int Tout, void *out);

// A grid is 32 bits of threads: workgroups * threads per workgroup < 2^32, and a larger launch runs the threads that remain
// modulo 2^32 and reports nothing (profiles/grid_limit_notes.md).  The most workgroups of `threads` threads one launch takes:
// 2^22 - 1 of 1024, 2^23 - 1 of 512, 2^24 - 1 of 256, 2^26 - 1 of 64.
constexpr long max_workgroups(int threads) { return ((1L << 32) - 1) / threads; }
// The most batch items one launch takes when every item is `per_item` workgroups of `threads` threads (0: one item alone is over
// the limit).  Launchers of one-workgroup-set-per-item kernels walk the batch in slices of this many items.
inline long items_per_launch(long per_item, int threads) { return per_item > 0 ? max_workgroups(threads) / per_item : 0; }

#define MLPG_HIP_CHECK(expr)                                                        \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                         \
      ::mlpg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return MLPG_HIP_ERUNTIME;                                                     \
    }                                                                               \
  } while (0)

}  // namespace mlpg
