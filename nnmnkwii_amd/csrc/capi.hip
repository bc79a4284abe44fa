// C-ABI entry points of libmlpg_hip.so (declared in include/mlpg_hip.h).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <map>
#include <mutex>
#include <utility>

#include "common.h"
#include "mlpg_strip_geom.h"

namespace mlpg {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

std::atomic<long long> g_launches[kCountKinds];
void note_launch(int kind) {
  if (kind >= 0 && kind < kCountKinds) g_launches[kind].fetch_add(1);
}

std::atomic<bool> g_modspec_direct{false};  // mlpg_hip_modspec_set_direct
bool modspec_direct() { return g_modspec_direct; }

// ---- grow-only scratch, one set of buffers per (device, stream) ------------------------------
// Launches on different streams of one device never share a buffer; a buffer is only ever
// reused, grown or freed behind work of its own stream.
namespace {
constexpr int kSlots = 7;
struct Slot {
  void *ptr = nullptr;
  size_t bytes = 0;
  unsigned long long gen = 0;  // allocation number: a caller that remembers the buffer's content checks this
};
unsigned long long g_scratch_gen = 0;
struct StreamScratch {
  Slot slot[kSlots];
};
std::map<std::pair<int, hipStream_t>, StreamScratch> g_scratch;
std::mutex g_mu;
SideStreams *g_side[kMaxDevices] = {};  // side streams of mlpg_hip_forward_streams (created on first use)
}  // namespace

void *scratch(int device, hipStream_t stream, int slot, size_t bytes, unsigned long long *gen) {
  if (device < 0 || device >= kMaxDevices || slot < 0 || slot >= kSlots) {
    set_error("scratch: bad device/slot %d/%d", device, slot);
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(g_mu);
  Slot &s = g_scratch[std::make_pair(device, stream)].slot[slot];
  if (s.bytes >= bytes && s.ptr) {
    if (gen) *gen = s.gen;
    return s.ptr;
  }
  if (s.ptr) {
    // the previous users of this buffer were enqueued on this very stream
    (void)hipStreamSynchronize(stream);
    (void)hipFree(s.ptr);
    s.ptr = nullptr;
    s.bytes = 0;
  }
  size_t want = bytes + bytes / 8 + 256;
  void *p = nullptr;
  if (hipMalloc(&p, want) != hipSuccess) {
    (void)hipGetLastError();
    want = bytes;
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      set_error("scratch: hipMalloc of %zu bytes failed", bytes);
      return nullptr;
    }
  }
  s.ptr = p;
  s.bytes = want;
  s.gen = ++g_scratch_gen;
  if (gen) *gen = s.gen;
  return p;
}

SideStreams *side_streams(int device) {
  if (device < 0 || device >= kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_side[device]) return g_side[device];
  SideStreams *s = new SideStreams();
  bool ok = hipEventCreateWithFlags(&s->fork, hipEventDisableTiming) == hipSuccess;
  for (int q = 0; ok && q < SideStreams::kN; ++q)
    ok = hipStreamCreateWithFlags(&s->st[q], hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&s->join[q], hipEventDisableTiming) == hipSuccess;
  if (!ok) {  // no side streams: the caller falls back to its own stream
    (void)hipGetLastError();
    delete s;
    return nullptr;
  }
  g_side[device] = s;
  return s;
}

int pack_windows(int nw, const int32_t *wl, const int32_t *wu, const double *wc, WinSet *ws) {
  if (nw < 1 || nw > kMaxWindows || !wl || !wu || !wc) {
    set_error("num_windows must be in [1, %d] and the window tables non-NULL", kMaxWindows);
    return MLPG_HIP_EINVAL;
  }
  memset(ws, 0, sizeof(*ws));
  ws->nw = nw;
  int off = 0;
  for (int w = 0; w < nw; ++w) {
    if (wl[w] < 0 || wu[w] < 0 || wl[w] > kMaxExtent || wu[w] > kMaxExtent) {
      set_error("window %d: extents (l=%d, u=%d) must be in [0, %d]", w, wl[w], wu[w], kMaxExtent);
      return MLPG_HIP_EINVAL;
    }
    const int n = wl[w] + wu[w] + 1;
    if (off + n > kMaxCoef) {
      set_error("too many window coefficients (> %d)", kMaxCoef);
      return MLPG_HIP_EINVAL;
    }
    ws->l[w] = wl[w];
    ws->u[w] = wu[w];
    ws->off[w] = off;
    for (int i = 0; i < n; ++i) ws->c[off + i] = wc[off + i];
    off += n;
    if (wl[w] + wu[w] > ws->q) ws->q = wl[w] + wu[w];
    const int m = wl[w] > wu[w] ? wl[w] : wu[w];
    if (m > ws->mw) ws->mw = m;
  }
  return 0;
}

int coef_offset(const char *who, const int32_t *wl, const int32_t *wu, int win_first, size_t *off) {
  size_t coff = 0;
  for (int w = 0; w < win_first; ++w) {
    if (wl[w] < 0 || wu[w] < 0 || wl[w] > kMaxExtent || wu[w] > kMaxExtent) {
      set_error("%s: window %d: extents (l=%d, u=%d) must be in [0, %d]", who, w, wl[w], wu[w], kMaxExtent);
      return MLPG_HIP_EINVAL;
    }
    coff += (size_t)(wl[w] + wu[w] + 1);
  }
  *off = coff;
  return 0;
}

int check_dtype(const char *who, int dtype) {
  if (dtype == MLPG_HIP_F32 || dtype == MLPG_HIP_F64) return 0;
  set_error("%s: dtype must be MLPG_HIP_F32 or MLPG_HIP_F64 (got %d)", who, dtype);
  return MLPG_HIP_EINVAL;
}

int check_var(const char *who, int var_mode, const void *var) {
  if (var_mode >= 0 && var_mode <= 2 && (var_mode == MLPG_HIP_VAR_UNIT || var)) return 0;
  set_error("%s: bad var_mode %d / NULL var", who, var_mode);
  return MLPG_HIP_EINVAL;
}

int check_device(const char *who, int device) {
  if (device >= 0 && device < kMaxDevices) return 0;
  set_error("%s: bad device %d", who, device);
  return MLPG_HIP_EINVAL;
}

namespace {

int check_common(int B, int Tmax, int D, int nw) {
  if (B < 0 || Tmax < 0 || D < 0 || nw < 1) {
    set_error("negative size (B=%d, Tmax=%d, D=%d) or num_windows=%d", B, Tmax, D, nw);
    return MLPG_HIP_EINVAL;
  }
  if (D % nw != 0) {
    set_error("D=%d is not a multiple of num_windows=%d", D, nw);
    return MLPG_HIP_EINVAL;
  }
  return 0;
}

}  // namespace

// Kernel choice, in ONE place (round 6): which kernel a problem goes to, as a pure function of the problem -- used by
// dispatch_solve, which launches it (and asks again with a kernel excluded when that kernel declines at launch time: the FIR form
// whose tap table fails its decay test, the transposed strip form the grid cannot hold), and by the stream plan of
// mlpg_hip_forward_streams (plan_streams, streams_api.hip), which must know beforehand whether a stream will occupy the device with a
// persistent grid (takes_strip_tr).
// AUTO = the FIR form for float32 unit variances without lengths; the strip kernel's transposed form for narrow streams; the
// constant-coefficient kernel for global / unit variances; the chunked kernel for window extents of 2; the strip kernel for wide
// streams (static dims on lanes); the wave-per-system kernel for narrow ones and small launches; else the natural-order kernel.
enum Route { kRouteFir, kRouteStripTr, kRouteConst, kRouteChunk, kRouteStrip, kRouteWave, kRouteGeneric, kRoutePieceBackward };
enum { kExcludeFir = 1, kExcludeTr = 2 };
static Route route_of(int in_dtype, int out_dtype, int algo, bool backward, const Problem &p, const WinSet &ws, unsigned exclude) {
  const bool piece = p.pitch && p.pitch != p.sd;  // some of a stream's static dims: window pitch != number of dims
  if (algo == MLPG_HIP_ALGO_PIPE) algo = strip_supported(p, ws) ? MLPG_HIP_ALGO_STRIP : MLPG_HIP_ALGO_AUTO;  // retired: the scheme it pipelined
  if (algo == MLPG_HIP_ALGO_FIR) return kRouteFir;
  // (the FIR form first: it has no chain at all; not for a piece of a stream)
  if (algo == MLPG_HIP_ALGO_AUTO && !piece && !(exclude & kExcludeFir) && fir_shape_supported(p, ws, in_dtype, out_dtype) && fir_preferred(p, backward))
    return kRouteFir;
  // a narrow stream (or the piece a merged launch left over): the strip kernel with its lanes over several utterances
  if (!(exclude & kExcludeTr) && ((algo == MLPG_HIP_ALGO_AUTO && strip_tr_preferred(p, ws, backward, in_dtype, out_dtype)) ||
                                 (algo == MLPG_HIP_ALGO_STRIP && piece && strip_tr_supported(p, ws, backward, in_dtype, out_dtype))))
    return kRouteStripTr;
  if (piece) {  // otherwise the kernels that take the pitch separately
    if (backward) return kRoutePieceBackward;
    return wave_supported(p, ws) ? kRouteWave : kRouteGeneric;
  }
  if (algo == MLPG_HIP_ALGO_AUTO) {
    if (const_preferred(p, ws)) return kRouteConst;
    if (in_dtype == out_dtype && chunk_preferred(p, ws, backward)) return kRouteChunk;
    if (strip_preferred(p, ws, backward, in_dtype) || (strip_supported(p, ws) && !wave_supported(p, ws))) return kRouteStrip;
    return wave_supported(p, ws) ? kRouteWave : kRouteGeneric;
  }
  switch (algo) {
    case MLPG_HIP_ALGO_CONST: return kRouteConst;
    case MLPG_HIP_ALGO_CHUNK: return kRouteChunk;
    case MLPG_HIP_ALGO_STRIP: return kRouteStrip;
    case MLPG_HIP_ALGO_WAVE: return kRouteWave;
    default: return kRouteGeneric;
  }
}

// Can the kernel family `algo` names take this problem?  Pure host logic (no device is touched): what dispatch_solve refuses before
// it launches anything, asked beforehand by the stream-table entry points for every stream of their table.
int check_algo(int in_dtype, int out_dtype, int algo, const Problem &p, const WinSet &ws) {
  if (algo < MLPG_HIP_ALGO_AUTO || algo > MLPG_HIP_ALGO_FIR) {
    set_error("unknown algo %d", algo);
    return MLPG_HIP_EINVAL;
  }
  if (algo == MLPG_HIP_ALGO_WAVE && !wave_supported(p, ws)) {
    set_error("MLPG_HIP_ALGO_WAVE does not support this problem (T=%d, half-bandwidth %d)", p.Tmax, ws.q);
    return MLPG_HIP_EINVAL;
  }
  if (algo == MLPG_HIP_ALGO_STRIP && !strip_supported(p, ws)) {
    set_error("MLPG_HIP_ALGO_STRIP does not support this problem (T=%d, half-bandwidth %d)", p.Tmax, ws.q);
    return MLPG_HIP_EINVAL;
  }
  if (algo == MLPG_HIP_ALGO_CONST && !const_supported(p, ws)) {
    set_error("MLPG_HIP_ALGO_CONST needs global or unit variances and 2-3 windows of extent <= 1 (var_mode %d, %d windows, T=%d)", p.var_mode, ws.nw, p.Tmax);
    return MLPG_HIP_EINVAL;
  }
  if (algo == MLPG_HIP_ALGO_GENERIC && !generic_grid_fits(p)) {
    set_error("MLPG_HIP_ALGO_GENERIC: B * sd * Tmax = %d * %d * %d cells are more than the %ld workgroups of 256 threads one launch takes: "
              "a grid is 32 bits of threads", p.B, p.sd, p.Tmax, max_workgroups(256));
    return MLPG_HIP_EINVAL;
  }
  if (algo == MLPG_HIP_ALGO_CHUNK && ws.mw >= 1 && ws.mw <= 2 && !chunk_grid_fits(p, ws)) {
    set_error("MLPG_HIP_ALGO_CHUNK: B = %d, sd = %d, Tmax = %d take more than the %ld workgroups of 256 threads (%ld of 64 in the "
              "reductions) one launch takes: a grid is 32 bits of threads", p.B, p.sd, p.Tmax, max_workgroups(256), max_workgroups(64));
    return MLPG_HIP_EINVAL;
  }
  if (algo == MLPG_HIP_ALGO_CHUNK && (in_dtype != out_dtype || !chunk_supported(p, ws))) {
    set_error("MLPG_HIP_ALGO_CHUNK: input dtype = output dtype, 1-3 windows of extent 1 or 2 (%d windows, extent %d)", ws.nw, ws.mw);
    return MLPG_HIP_EINVAL;
  }
  if (algo == MLPG_HIP_ALGO_FIR && p.B >= 1 && p.sd >= 1 && !fir_grid_fits(p)) {
    set_error("MLPG_HIP_ALGO_FIR: %ld workgroups of 512 threads are more than one launch takes (%ld): a grid is 32 bits of threads",
              fir_workgroups(p), max_workgroups(512));
    return MLPG_HIP_EINVAL;
  }
  if (algo == MLPG_HIP_ALGO_FIR && !fir_shape_supported(p, ws, in_dtype, out_dtype)) {
    set_error("MLPG_HIP_ALGO_FIR: unit variances, float32 in and out, no lengths, T >= 96, 1-3 windows of extent <= 2 (the first a single tap)");
    return MLPG_HIP_EINVAL;
  }
  return 0;
}

bool takes_strip_tr(int dtype, int algo, const Problem &p, const WinSet &ws) {
  return route_of(dtype, dtype, algo, false, p, ws, 0) == kRouteStripTr;  // (the decision dispatch_solve will take)
}

int dispatch_solve(hipStream_t st, int in_dtype, int out_dtype, int algo, bool backward, const Problem &p,
                   const WinSet &ws, int device) {
  if (int rc = check_algo(in_dtype, out_dtype, algo, p, ws)) return rc;
  unsigned exclude = 0;
  for (;;) {
    switch (route_of(in_dtype, out_dtype, algo, backward, p, ws, exclude)) {
      case kRouteFir: {
        const int rc = launch_fir(st, backward, p, ws, device);
        if (rc != kFirNotApplicable) return rc;
        if (algo == MLPG_HIP_ALGO_FIR) {
          set_error("MLPG_HIP_ALGO_FIR: the inverse of this window set does not decay to 2^-26 within 24 frames (or the stream is being captured before the tap table exists)");
          return MLPG_HIP_EINVAL;
        }
        exclude |= kExcludeFir;  // the other kernels take the call
        continue;
      }
      case kRouteStripTr: {
        const int rc = launch_strip_tr(st, in_dtype, p, ws, device);
        if (rc != strip::kNotResident) return rc;
        exclude |= kExcludeTr;  // a launch the grid cannot hold: the other kernels
        continue;
      }
      case kRoutePieceBackward:
        set_error("a stream piece (pitch %d, %d dims) has no backward pass", p.pitch, p.sd);
        return MLPG_HIP_EINVAL;
      case kRouteConst: return launch_const(st, in_dtype, out_dtype, backward, p, ws, device);
      case kRouteChunk: return launch_chunk(st, in_dtype, out_dtype, backward, p, ws, device);
      // (the strip launcher tries the transposed form itself when asked for by name: not again after it declined here)
      case kRouteStrip: return launch_strip(st, in_dtype, out_dtype, backward, p, ws, device, !(exclude & kExcludeTr));
      case kRouteWave: return launch_wave(st, in_dtype, out_dtype, backward, p, ws, device);
      default: return launch_generic(st, in_dtype, out_dtype, backward, p, ws, device);
    }
  }
}

namespace {

int solve_entry(int device, void *stream, int in_dtype, int out_dtype, int algo, bool backward, const void *mean,
                const void *var, int var_mode, const void *grad_out, const int32_t *lengths, int B, int Tmax,
                int D, int nw, const int32_t *wl, const int32_t *wu, const double *wc, void *out,
                int32_t *status) {
  const char *who = backward ? "backward" : "forward";
  if (int rc = check_common(B, Tmax, D, nw)) return rc;
  if (int rc = check_dtype(who, in_dtype)) return rc;
  if (int rc = check_dtype(who, out_dtype)) return rc;
  if (int rc = check_var(who, var_mode, var)) return rc;
  if (B * (long)Tmax * D > 0 && (!out || (backward ? !grad_out : !mean))) {
    set_error("%s: NULL data pointer", who);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  WinSet ws;
  if (int rc = pack_windows(nw, wl, wu, wc, &ws)) return rc;
  if (B == 0 || Tmax == 0 || D == 0) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  const Problem p = dense_problem(mean, var, grad_out, lengths, out, status, backward, var_mode, B, Tmax, D, D / nw);
  return dispatch_solve((hipStream_t)stream, in_dtype, out_dtype, algo, backward, p, ws, device);
}

}  // namespace
long long host_chunks_on_device(int device);  // host_api.hip
}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int mlpg_hip_abi_version(void) { return 14; }

__attribute__((visibility("default"))) long long mlpg_hip_launch_count(int kind) {
  if (kind >= 100) return host_chunks_on_device(kind - 100);  // chunks the host-memory calls enqueued on device kind - 100
  return kind >= 0 && kind < kCountKinds && kind != kCountUnused12 && kind != kCountUnused14 && kind != kCountUnused16 && kind != kCountUnused21 && kind != kCountUnused25 && kind != kCountUnused28 && kind != kCountUnused30 && kind != kCountUnused32 && kind != kCountUnused34 && kind != kCountUnused36 && kind != kCountUnused38 && kind != kCountUnused40 ? g_launches[kind].load() : -1;
}

__attribute__((visibility("default"))) const char *mlpg_hip_last_error(void) { return g_err; }

__attribute__((visibility("default"))) int mlpg_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

__attribute__((visibility("default"))) void mlpg_hip_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (auto &kv : g_scratch) {
    (void)hipSetDevice(kv.first.first);
    (void)hipDeviceSynchronize();
    for (int s = 0; s < kSlots; ++s)
      if (kv.second.slot[s].ptr) (void)hipFree(kv.second.slot[s].ptr);
  }
  g_scratch.clear();
  for (int d = 0; d < kMaxDevices; ++d) {
    if (!g_side[d]) continue;
    (void)hipSetDevice(d);
    for (int q = 0; q < SideStreams::kN; ++q) {
      (void)hipStreamSynchronize(g_side[d]->st[q]);
      (void)hipStreamDestroy(g_side[d]->st[q]);
      (void)hipEventDestroy(g_side[d]->join[q]);
    }
    (void)hipEventDestroy(g_side[d]->fork);
    delete g_side[d];
    g_side[d] = nullptr;
  }
  fir_shutdown();
  host_api_shutdown();
  if (prev >= 0) (void)hipSetDevice(prev);
}

__attribute__((visibility("default"))) int mlpg_hip_forward(int device, void *stream, int dtype, int algo,
                                                            const void *mean, const void *var, int var_mode,
                                                            const int32_t *lengths, int B, int Tmax, int D,
                                                            int num_windows, const int32_t *win_l_h,
                                                            const int32_t *win_u_h, const double *win_coef_h,
                                                            void *out, int32_t *status) {
  return solve_entry(device, stream, dtype, dtype, algo, false, mean, var, var_mode, nullptr, lengths, B, Tmax, D,
                     num_windows, win_l_h, win_u_h, win_coef_h, out, status);
}

namespace {
// The form mlpg_hip_unit_mse_step takes for a problem -- decided HERE and nowhere else (the step and mlpg_hip_unit_mse_form both ask):
// 2 the FIR form (two launches; needs the workspace of mlpg_hip_unit_mse_workspace_bytes_t), 1 the one-launch wave-per-system kernel,
// 0 neither.  `with_fir_workspace`: the caller can provide the larger workspace.
int unit_mse_form(hipStream_t st, int device, int dtype, const Problem &p, const WinSet &ws, bool with_fir_workspace) {
  if (with_fir_workspace && dtype == MLPG_HIP_F32 && fir_shape_supported(p, ws, dtype, dtype) && fir_table_ready(st, device, ws)) return 2;
  return unit_mse_supported(p.Tmax, ws) ? 1 : 0;
}
}  // namespace

__attribute__((visibility("default"))) int mlpg_hip_unit_mse_form(int device, void *stream, int dtype, int has_lengths, int B,
                                                                  int Tmax, int D, int num_windows, const int32_t *win_l_h,
                                                                  const int32_t *win_u_h, const double *win_coef_h) {
  const char *who = "unit_mse_form";
  if (int rc = check_common(B, Tmax, D, num_windows)) return rc;
  if (int rc = check_dtype(who, dtype)) return rc;
  if (int rc = check_device(who, device)) return rc;
  WinSet ws;
  if (int rc = pack_windows(num_windows, win_l_h, win_u_h, win_coef_h, &ws)) return rc;
  if (B == 0 || Tmax == 0 || D == 0) return 1;  // (the step answers an empty batch itself: loss 0)
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  static const int32_t some_lengths = 0;  // (the lengths are only looked at as "given or not")
  Problem p = dense_problem(nullptr, nullptr, nullptr, has_lengths ? &some_lengths : nullptr, nullptr, nullptr, false, MLPG_HIP_VAR_UNIT,
                            B, Tmax, D, D / num_windows);
  p.ld_out = D;  // (the step's output is the gradient, (B, Tmax, D))
  return unit_mse_form((hipStream_t)stream, device, dtype, p, ws, true);
}

__attribute__((visibility("default"))) int mlpg_hip_unit_mse_step(int device, void *stream, int dtype, const void *mean,
                                                                  const void *target, const int32_t *lengths, int B,
                                                                  int Tmax, int D, int num_windows,
                                                                  const int32_t *win_l_h, const int32_t *win_u_h,
                                                                  const double *win_coef_h, double n_elems, void *y_out,
                                                                  void *grad_mean, double *loss, int32_t *status,
                                                                  void *workspace, size_t workspace_bytes) {
  const char *who = "unit_mse_step";
  if (int rc = check_common(B, Tmax, D, num_windows)) return rc;
  if (int rc = check_dtype(who, dtype)) return rc;
  if (int rc = check_device(who, device)) return rc;
  if (!(n_elems > 0.0)) {
    set_error("unit_mse_step: n_elems must be positive");
    return MLPG_HIP_EINVAL;
  }
  WinSet ws;
  if (int rc = pack_windows(num_windows, win_l_h, win_u_h, win_coef_h, &ws)) return rc;
  if (!loss) {
    set_error("unit_mse_step: NULL loss pointer");
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  hipStream_t st = (hipStream_t)stream;
  if (B == 0 || Tmax == 0 || D == 0) {
    MLPG_HIP_CHECK(hipMemsetAsync(loss, 0, sizeof(double), st));
    return 0;
  }
  if (!mean || !target || !grad_mean) {
    set_error("unit_mse_step: NULL data pointer");
    return MLPG_HIP_EINVAL;
  }
  Problem p = dense_problem(mean, nullptr, nullptr, lengths, grad_mean, status, false, MLPG_HIP_VAR_UNIT, B, Tmax, D, D / num_windows);
  p.ld_out = D;  // (a forward problem whose output is the gradient, (B, Tmax, D))
  // float32 batches without lengths, given the larger workspace (mlpg_hip_unit_mse_workspace_bytes_t): the FIR form, two launches
  const bool fir_ws = workspace && !((uintptr_t)workspace & 127) && workspace_bytes >= fir_mse_workspace_bytes(B, Tmax, p.sd);
  const int form = unit_mse_form(st, device, dtype, p, ws, fir_ws);
  if (form == 2) {
    const int rc = launch_fir_mse(st, p, ws, device, target, y_out, n_elems, loss, workspace);
    if (rc != kFirNotApplicable) return rc;
  }
  if (!unit_mse_supported(Tmax, ws)) {
    set_error("unit_mse_step: needs window extents <= 1 and T <= 1024 (T=%d, half-bandwidth %d), or a float32 batch without lengths "
              "of T >= 96 whose window set passes the FIR form's decay test (mlpg_hip_unit_mse_form says which), with the workspace of "
              "mlpg_hip_unit_mse_workspace_bytes_t; inside a stream capture the FIR form needs its tap table built by an earlier call",
              Tmax, ws.q);
    return MLPG_HIP_EINVAL;
  }
  if (unit_mse_workgroups(B, D / num_windows) > max_workgroups(256)) {  // (one launch with one arrival counter: not sliced)
    set_error("unit_mse_step: %ld workgroups of 256 threads (8 per block of 8 utterances and group of 4 static dims) are more than one "
              "launch takes (%ld): a grid is 32 bits of threads; split the batch", unit_mse_workgroups(B, D / num_windows),
              max_workgroups(256));
    return MLPG_HIP_EINVAL;
  }
  if (!workspace || workspace_bytes < unit_mse_workspace_bytes(B, D / num_windows) || ((uintptr_t)workspace & 127)) {
    set_error("unit_mse_step: workspace of %zu bytes (128-byte aligned) needed, see mlpg_hip_unit_mse_workspace_bytes",
              unit_mse_workspace_bytes(B, D / num_windows));
    return MLPG_HIP_EINVAL;
  }
  return launch_unit_mse(st, dtype, p, ws, target, y_out, n_elems, loss, workspace);
}

__attribute__((visibility("default"))) size_t mlpg_hip_unit_mse_workspace_bytes(int B, int D, int num_windows) {
  if (B < 0 || D < 0 || num_windows < 1) return 0;
  return unit_mse_workspace_bytes(B, D / num_windows);
}

__attribute__((visibility("default"))) size_t mlpg_hip_unit_mse_workspace_bytes_t(int B, int Tmax, int D, int num_windows) {
  if (B < 0 || Tmax < 0 || D < 0 || num_windows < 1) return 0;
  return std::max(unit_mse_workspace_bytes(B, D / num_windows), fir_mse_workspace_bytes(B, Tmax, D / num_windows));
}

__attribute__((visibility("default"))) int mlpg_hip_stream_copy(int device, void *stream, const void *src, void *dst,
                                                                size_t nbytes) {
  if (nbytes == 0) return 0;
  if (!src || !dst || (((uintptr_t)src | (uintptr_t)dst) & 15)) {
    set_error("stream_copy: NULL or not 16-byte aligned pointer");
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g("stream_copy", device);
  if (g.rc) return g.rc;
  return launch_stream_copy((hipStream_t)stream, src, dst, nbytes);
}

__attribute__((visibility("default"))) int mlpg_hip_backward(int device, void *stream, int in_dtype, int out_dtype,
                                                             int algo, const void *var, int var_mode,
                                                             const void *grad_out, const int32_t *lengths, int B,
                                                             int Tmax, int D, int num_windows,
                                                             const int32_t *win_l_h, const int32_t *win_u_h,
                                                             const double *win_coef_h, void *grad_mean,
                                                             int32_t *status) {
  return solve_entry(device, stream, in_dtype, out_dtype, algo, true, nullptr, var, var_mode, grad_out, lengths, B,
                     Tmax, D, num_windows, win_l_h, win_u_h, win_coef_h, grad_mean, status);
}

__attribute__((visibility("default"))) int mlpg_hip_backward_var(int device, void *stream, int dtype, int algo,
                                                                 const void *mean, const void *var, int var_mode, const void *y,
                                                                 const void *grad_out, const int32_t *lengths, int B, int Tmax,
                                                                 int D, int num_windows, const int32_t *win_l_h,
                                                                 const int32_t *win_u_h, const double *win_coef_h,
                                                                 void *grad_mean, void *grad_var, int32_t *status) {
  // every argument is checked here or by solve_entry before its solve is enqueued; the epilogue itself cannot be refused
  const char *who = "backward_var";
  if (int rc = check_common(B, Tmax, D, num_windows)) return rc;
  if (int rc = check_dtype(who, dtype)) return rc;
  if (var_mode == MLPG_HIP_VAR_UNIT) {
    set_error("backward_var: unit variances (MLPG_HIP_VAR_UNIT) have no variances to differentiate");
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_var(who, var_mode, var)) return rc;
  if (!status) {
    set_error("backward_var: status is required (int32, B * D/num_windows): a failing system's gradients are zeroed from it");
    return MLPG_HIP_EINVAL;
  }
  if (B * (long)Tmax * D > 0 && (!mean || !y || !grad_out || !grad_mean || !grad_var)) {
    set_error("backward_var: NULL data pointer (mean, y, grad_out, grad_mean and grad_var are required)");
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device(who, device)) return rc;
  WinSet ws;
  if (int rc = pack_windows(num_windows, win_l_h, win_u_h, win_coef_h, &ws)) return rc;
  // the solve z = P^-1 g and grad_mean, exactly as mlpg_hip_backward(dtype, dtype, algo, ...) computes them
  if (int rc = solve_entry(device, stream, dtype, dtype, algo, true, nullptr, var, var_mode, grad_out, lengths, B, Tmax, D,
                           num_windows, win_l_h, win_u_h, win_coef_h, grad_mean, status))
    return rc;
  if (B == 0 || Tmax == 0 || D == 0) return 0;
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  return launch_var_grad((hipStream_t)stream, dtype, grad_mean, var, var_mode, mean, y, lengths, status, B, Tmax, D / num_windows,
                         ws, grad_var);
}

__attribute__((visibility("default"))) int mlpg_hip_delta_features(int device, void *stream, int dtype, const void *x,
                                                                   const int32_t *lengths, int B, int Tmax, int D,
                                                                   int num_windows, const int32_t *win_l_h,
                                                                   const int32_t *win_u_h, const double *win_coef_h,
                                                                   void *out) {
  if (B < 0 || Tmax < 0 || D < 0 || (dtype != MLPG_HIP_F32 && dtype != MLPG_HIP_F64)) {
    set_error("delta_features: bad arguments");
    return MLPG_HIP_EINVAL;
  }
  WinSet ws;
  if (int rc = pack_windows(num_windows, win_l_h, win_u_h, win_coef_h, &ws)) return rc;
  if ((long)B * Tmax * D == 0) return 0;
  if (!elementwise_grid_fits(B, Tmax, D)) {
    set_error("delta_features: B * Tmax * D = %d * %d * %d elements are more than the %ld workgroups of 256 threads one launch takes: a "
              "grid is 32 bits of threads", B, Tmax, D, max_workgroups(256));
    return MLPG_HIP_EINVAL;
  }
  if (!x || !out) {
    set_error("delta_features: NULL pointer");
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g("delta_features", device);
  if (g.rc) return g.rc;
  return launch_delta((hipStream_t)stream, dtype, x, lengths, B, Tmax, D, ws, out);
}

namespace {
// The route of the float64 entries, by the DFT length and the direct switch alone (mlpg_hip_modspec_route): 0 the in-LDS FFT,
// 1 the direct transform, 2 chirp-z, -1 no transform (n < 2)
int modspec_route(int n) {
  if (n < 2) return -1;
  if (g_modspec_direct) return 1;
  if (modspec_fft_takes(n)) return 0;
  return modspec_chirp_takes(n) ? 2 : 1;
}

int modspec_entry(int device, void *stream, int mode, const double *x, const double *ms, const double *ph, double *out,
                  double *out_ph, int B, int T, int D, int n, int ortho, int limit_bin, int log_domain) {
  if (B < 0 || T < 0 || D < 0 || n < 1) {
    set_error("modspec: negative size");
    return MLPG_HIP_EINVAL;
  }
  if (n < 2) {
    set_error("modspec: the DFT length must be at least 2 (got %d)", n);
    return MLPG_HIP_EINVAL;
  }
  if (T > n) {
    set_error("modspec: DFT length %d must not be smaller than the time length %d", n, T);
    return MLPG_HIP_EINVAL;
  }
  if ((long)B * D == 0) return 0;
  if (!out || (mode == 1 ? (!ms || !ph) : !x) || (mode == 3 && !ms)) {
    set_error("modspec: NULL pointer");
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_device("modspec", device)) return rc;  // (as the padded-minibatch entries: asked before the runtime is touched)
  DeviceGuard g("modspec", device);
  if (g.rc) return g.rc;
  const hipStream_t st = (hipStream_t)stream;
  switch (modspec_route(n)) {
    case 0:  // powers of two up to 4096 (the reference's defaults are 2048 and 4096): the fused in-LDS FFT
      return launch_modspec(st, mode, x, ms, ph, out, out_ph, B, T, D, n, ortho, limit_bin, log_domain);
    case 2: {  // any other length up to 2048: the chirp-z transform on that FFT
      const int rc = launch_modspec_chirp(st, device, mode, x, ms, ph, out, out_ph, B, T, D, n, ortho, limit_bin, log_domain);
      if (rc == 0) note_launch(kCountModspecChirp);
      return rc;
    }
  }
  // the rest, and every length behind mlpg_hip_modspec_set_direct(1): the direct transform of modspec_dft.hip
  return launch_modspec_dft(st, device, mode, x, ms, ph, out, out_ph, B, T, D, n, ortho, limit_bin, log_domain);
}
}  // namespace

// Testing aid: route every DFT length through the direct transform (so that it can be compared with the FFT path).
__attribute__((visibility("default"))) void mlpg_hip_modspec_set_direct(int on) { g_modspec_direct = on != 0; }

// The route mlpg_hip_modspec, _inv_modspec, _modspec_smoothing and _modspec_backward take at DFT length n (modspec_entry decides
// with this very function).
__attribute__((visibility("default"))) int mlpg_hip_modspec_route(int n) { return modspec_route(n); }

__attribute__((visibility("default"))) int mlpg_hip_modspec(int device, void *stream, const double *x, int B, int T,
                                                            int D, int n, int ortho, double *ms, double *phase) {
  return modspec_entry(device, stream, 0, x, nullptr, nullptr, ms, phase, B, T, D, n, ortho, 0, 0);
}

__attribute__((visibility("default"))) int mlpg_hip_inv_modspec(int device, void *stream, const double *ms,
                                                                const double *phase, int B, int n, int D, int ortho,
                                                                double *x) {
  return modspec_entry(device, stream, 1, nullptr, ms, phase, x, nullptr, B, 0, D, n, ortho, 0, 0);
}

__attribute__((visibility("default"))) int mlpg_hip_modspec_smoothing(int device, void *stream, const double *x, int B,
                                                                      int T, int D, int n, int ortho, int limit_bin,
                                                                      int log_domain, double *out) {
  return modspec_entry(device, stream, 2, x, nullptr, nullptr, out, nullptr, B, T, D, n, ortho, limit_bin, log_domain);
}

__attribute__((visibility("default"))) int mlpg_hip_modspec_backward(int device, void *stream, const double *x,
                                                                     const double *grad_ms, int B, int T, int D,
                                                                     int n, int ortho, double *grad_x) {
  return modspec_entry(device, stream, 3, x, grad_ms, nullptr, grad_x, nullptr, B, T, D, n, ortho, 0, 0);
}

__attribute__((visibility("default"))) int mlpg_hip_trim_lengths(int device, void *stream, int dtype, const void *X,
                                                                 int N, int T, int D, double eps,
                                                                 int32_t *lengths) {
  if (N < 0 || T < 0 || D < 0 || (dtype != MLPG_HIP_F32 && dtype != MLPG_HIP_F64)) {
    set_error("trim_lengths: bad arguments");
    return MLPG_HIP_EINVAL;
  }
  if (N == 0) return 0;
  if (!lengths || (!X && (long)T * D > 0)) {
    set_error("trim_lengths: NULL pointer");
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g("trim_lengths", device);
  if (g.rc) return g.rc;
  return launch_trim((hipStream_t)stream, dtype, X, N, T, D, eps, lengths);
}

__attribute__((visibility("default"))) int mlpg_hip_fastdtw(int device, void *stream, const double *X,
                                                            const double *Y, const int32_t *lenx,
                                                            const int32_t *leny, int N, int Tx, int Ty, int D,
                                                            int radius, int dist_kind, double dist_scale,
                                                            int tie_rule, int32_t *path_i, int32_t *path_j,
                                                            int32_t *path_len, double *cost) {
  if (N < 0 || Tx < 1 || Ty < 1 || D < 1 || radius < 1) {
    set_error("fastdtw: need N >= 0, Tx, Ty, D >= 1 and radius >= 1");
    return MLPG_HIP_EINVAL;
  }
  if (N == 0) return 0;
  if (!X || !Y || !lenx || !leny || !path_i || !path_j || !path_len || !cost) {
    set_error("fastdtw: NULL pointer");
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g("fastdtw", device);
  if (g.rc) return g.rc;
  return launch_fastdtw((hipStream_t)stream, device, X, Y, lenx, leny, N, Tx, Ty, D, radius, dist_kind, dist_scale,
                        tie_rule, path_i, path_j, path_len, cost);
}

__attribute__((visibility("default"))) int mlpg_hip_dtw_level_windows(int device, void *stream, int N, int radius,
                                                                      const int32_t *level_tx, const int32_t *level_ty,
                                                                      const int32_t *full, const int32_t *cpath_i,
                                                                      const int32_t *cpath_j, const int32_t *cpath_len,
                                                                      int cpath_stride, int32_t *row_lo, int32_t *row_hi,
                                                                      int64_t *row_off, int row_stride) {
  if (N < 0 || radius < 1 || row_stride < 1 || (N > 0 && (!level_tx || !level_ty || !full || !row_lo || !row_hi || !row_off))) {
    set_error("dtw_level_windows: bad argument");
    return MLPG_HIP_EINVAL;
  }
  if (N == 0) return 0;
  DeviceGuard g("dtw_level_windows", device);
  if (g.rc) return g.rc;
  return launch_dtw_window((hipStream_t)stream, device, N, radius, level_tx, level_ty, full, cpath_i, cpath_j, cpath_len,
                           cpath_stride, row_lo, row_hi, row_off, row_stride);
}

__attribute__((visibility("default"))) int mlpg_hip_dtw_level_from_costs(int device, void *stream, int N, int tie_rule,
                                                                         const int32_t *level_tx, const int32_t *level_ty,
                                                                         const int32_t *row_lo, const int32_t *row_hi,
                                                                         const int64_t *row_off, int row_stride, int max_ty,
                                                                         const double *costs, const int64_t *cost_base,
                                                                         int64_t total_cells, int32_t *path_i,
                                                                         int32_t *path_j, int32_t *path_len,
                                                                         int path_stride, double *cost) {
  if (N < 0 || row_stride < 1 || max_ty < 1 || path_stride < 1 || total_cells < 0 ||
      (tie_rule != MLPG_HIP_TIE_FIRST_MIN && tie_rule != MLPG_HIP_TIE_DIAG_LAST) ||
      (N > 0 && (!level_tx || !level_ty || !row_lo || !row_hi || !row_off || !costs || !cost_base || !path_i || !path_j ||
                 !path_len || !cost))) {
    set_error("dtw_level_from_costs: bad argument");
    return MLPG_HIP_EINVAL;
  }
  if (N == 0) return 0;
  DeviceGuard g("dtw_level_from_costs", device);
  if (g.rc) return g.rc;
  return launch_dtw_costs((hipStream_t)stream, device, N, tie_rule, level_tx, level_ty, row_lo, row_hi, row_off, row_stride,
                          max_ty, costs, cost_base, total_cells, path_i, path_j, path_len, path_stride, cost);
}

__attribute__((visibility("default"))) int mlpg_hip_fastdtw_l2(int device, void *stream, const double *X,
                                                               const double *Y, const int32_t *lenx,
                                                               const int32_t *leny, int N, int Tx, int Ty, int D,
                                                               int radius, int32_t *path_i, int32_t *path_j,
                                                               int32_t *path_len, double *cost) {
  return mlpg_hip_fastdtw(device, stream, X, Y, lenx, leny, N, Tx, Ty, D, radius, MLPG_HIP_DIST_L2, 1.0,
                          MLPG_HIP_TIE_FIRST_MIN, path_i, path_j, path_len, cost);
}

__attribute__((visibility("default"))) int mlpg_hip_gmm_convert(int device, void *stream, const double *x,
                                                                const double *posterior, const int32_t *mixture,
                                                                const double *mu_x, const double *mu_y,
                                                                const double *A, int64_t N, int D, int Dy, int M,
                                                                double *out) {
  if (N < 0 || D < 1 || Dy < 1 || M < 1) {
    set_error("gmm_convert: bad sizes");
    return MLPG_HIP_EINVAL;
  }
  if (N == 0) return 0;
  if ((double)N * Dy > (double)max_workgroups(256) * 256.0) {
    set_error("gmm_convert: N * Dy = %lld * %d elements are more than the %ld workgroups of 256 threads one launch takes: a grid is 32 "
              "bits of threads", (long long)N, Dy, max_workgroups(256));
    return MLPG_HIP_EINVAL;
  }
  if (!x || !mu_x || !mu_y || !A || !out || (!posterior && !mixture)) {
    set_error("gmm_convert: NULL pointer");
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g("gmm_convert", device);
  if (g.rc) return g.rc;
  return launch_gmm_convert((hipStream_t)stream, x, posterior, mixture, mu_x, mu_y, A, (long)N, D, Dy, M, out);
}

__attribute__((visibility("default"))) int mlpg_hip_gather_path(int device, void *stream, int dtype, const void *src,
                                                                const int32_t *path, const int32_t *path_len, int N,
                                                                int Tsrc, int path_stride, int D, int Tout,
                                                                void *out) {
  if (N < 0 || Tsrc < 0 || D < 0 || Tout < 0 || path_stride < 0 ||
      (dtype != MLPG_HIP_F32 && dtype != MLPG_HIP_F64)) {
    set_error("gather_path: bad arguments");
    return MLPG_HIP_EINVAL;
  }
  if (N == 0 || Tout == 0 || D == 0) return 0;
  if ((long)Tout * D > max_workgroups(256) * 256) {  // (utterances go in slices of launches; one utterance is one launch at least)
    set_error("gather_path: Tout * D = %d * %d elements per utterance are more than the %ld workgroups of 256 threads one launch takes: a "
              "grid is 32 bits of threads", Tout, D, max_workgroups(256));
    return MLPG_HIP_EINVAL;
  }
  if (!src || !path || !path_len || !out) {
    set_error("gather_path: NULL pointer");
    return MLPG_HIP_EINVAL;
  }
  DeviceGuard g("gather_path", device);
  if (g.rc) return g.rc;
  return launch_gather((hipStream_t)stream, dtype, src, path, path_len, N, Tsrc, path_stride, D, Tout, out);
}

}  // extern "C"
