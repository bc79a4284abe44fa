// The stream-table entry points, mlpg_hip_forward_streams and mlpg_hip_backward_streams (include/mlpg_hip.h): several streams of one
// (B, Tmax, ld) batch, consumed in place.  Both are validate -> (plan ->) refuse -> enqueue: check_stream_table and
// pack_stream_windows answer every fault of the arguments, plan_streams decides what the forward call launches as a value
// (StreamPlan: pure host logic), every stream's kernel family is asked with check_algo, and only then is anything enqueued -- a
// refused call writes nothing and moves no counter.
#include <climits>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "common.h"
#include "mlpg_strip_geom.h"

extern "C" const char *mlpg_hip_last_error(void);

namespace mlpg {
namespace {

// ---- validate -------------------------------------------------------------------------------------------------------------------

// The arguments both entry points share, as given, and what check_stream_table derives from the table.
struct StreamCall {
  int dtype, var_mode, B, Tmax, n;
  long ld_in, ld_out;
  const mlpg_hip_stream_t *streams;
  const int32_t *wl, *wu;
  const double *wc;
  const void *var;
  const int32_t *lengths;
  int32_t *status;
  long sd_total;                 // sum of static_dim: the row length of status
  bool any_dynamic;              // some stream has windows and static dims
  int status_cols[kMaxStreams];  // stream k's first status column (table order)
};

int check_stream_table(const char *who, int device, int dtype, int algo, const void *var, int var_mode, int64_t ld_in, int64_t ld_out,
                       const int32_t *lengths, int B, int Tmax, int num_streams, const mlpg_hip_stream_t *streams, int total_windows,
                       const int32_t *wl, const int32_t *wu, const double *wc, int32_t *status, StreamCall *c) {
  if (B < 0 || Tmax < 0 || num_streams < 0 || total_windows < 0 || ld_in < 0 || ld_out < 0 || ld_in > INT32_MAX ||
      ld_out > INT32_MAX) {
    set_error("%s: negative or oversized size argument", who);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = check_dtype(who, dtype)) return rc;
  if (algo < MLPG_HIP_ALGO_AUTO || algo > MLPG_HIP_ALGO_FIR) {
    set_error("%s: unknown algo %d", who, algo);
    return MLPG_HIP_EINVAL;
  }
  if (num_streams > 0 && !streams) {
    set_error("%s: NULL stream table", who);
    return MLPG_HIP_EINVAL;
  }
  if (num_streams > kMaxStreams) {
    set_error("%s: more than %d streams", who, kMaxStreams);
    return MLPG_HIP_EINVAL;
  }
  *c = StreamCall{dtype, var_mode, B, Tmax, num_streams, (long)ld_in, (long)ld_out, streams, wl, wu, wc, var, lengths, status, 0, false, {}};
  for (int k = 0; k < num_streams; ++k) {
    const mlpg_hip_stream_t &sm = streams[k];
    const long width = (long)(sm.num_windows > 0 ? sm.num_windows : 1) * sm.static_dim;
    if (sm.static_dim < 0 || sm.num_windows < 0 || sm.in_col < 0 || sm.out_col < 0 || sm.win_first < 0 ||
        sm.win_first + sm.num_windows > total_windows || sm.in_col + width > ld_in || (long)sm.out_col + sm.static_dim > ld_out) {
      set_error("%s: stream %d does not fit (in_col=%d, out_col=%d, static_dim=%d, num_windows=%d)", who, k, sm.in_col, sm.out_col,
                sm.static_dim, sm.num_windows);
      return MLPG_HIP_EINVAL;
    }
    c->status_cols[k] = (int)c->sd_total;
    c->sd_total += sm.static_dim;
    c->any_dynamic = c->any_dynamic || (sm.num_windows > 0 && sm.static_dim > 0);
  }
  if (int rc = check_var(who, var_mode, var)) return rc;
  if (total_windows > 0 && (!wl || !wu || !wc)) {
    set_error("%s: NULL window tables", who);
    return MLPG_HIP_EINVAL;
  }
  return check_device(who, device);
}

// The window list of every stream that has one, packed once per call (its extents and coefficient count are checked by the packing).
int pack_stream_windows(const char *who, const StreamCall &c, WinSet *wsets) {
  for (int k = 0; k < c.n; ++k) {
    const mlpg_hip_stream_t &sm = c.streams[k];
    if (sm.num_windows == 0) continue;
    size_t coff = 0;
    if (int rc = coef_offset(who, c.wl, c.wu, sm.win_first, &coff)) return rc;
    if (int rc = pack_windows(sm.num_windows, c.wl + sm.win_first, c.wu + sm.win_first, c.wc + coff, &wsets[k])) return rc;
  }
  return 0;
}

inline bool dynamic(const mlpg_hip_stream_t &sm) { return sm.num_windows > 0 && sm.static_dim > 0; }

// One stream as a Problem: a column slice of the parent arrays.  Forward: mean / var columns [in_col, in_col + nw*sd) of the
// (B, Tmax, ld_in) matrices, trajectory written to columns [out_col, out_col + sd) of the (B, Tmax, ld_out) `out`.  Backward: grad_out
// read from those output columns, `out` = grad_mean written to the input columns.  [d_first, d_first + d_count): the stream's static
// dims the problem holds (all of them by default; forward only).  NULL arrays stay NULL.
Problem stream_problem(const StreamCall &c, int k, bool backward, const void *mean, const void *grad_out, void *out, int d_first = 0,
                       int d_count = -1) {
  const mlpg_hip_stream_t &sm = c.streams[k];
  const size_t esz = c.dtype == MLPG_HIP_F32 ? 4 : 8;
  const size_t in_off = esz * (size_t)(sm.in_col + d_first), out_off = esz * (size_t)(sm.out_col + d_first);
  auto at = [](const void *base, size_t off) -> const char * { return base ? (const char *)base + off : nullptr; };
  const int sd = d_count < 0 ? sm.static_dim : d_count;
  Problem p;
  p.mean = at(mean, in_off);
  p.var = at(c.var, in_off);
  p.grad_out = at(grad_out, out_off);
  p.lengths = c.lengths;
  p.out = (char *)at(out, backward ? in_off : out_off);
  p.status = c.status ? c.status + c.status_cols[k] + d_first : nullptr;
  p.var_mode = c.var_mode;
  p.B = c.B;
  p.Tmax = c.Tmax;
  p.D = sm.num_windows * sd;
  p.sd = sd;
  p.pitch = sd != sm.static_dim ? sm.static_dim : 0;
  p.ld_in = c.ld_in;
  p.ld_gout = backward ? c.ld_out : 0;
  p.ld_out = backward ? c.ld_in : c.ld_out;
  p.ld_status = (int)c.sd_total;
  return p;
}

// Appends a stream to a member list (StreamMap of a merged forward launch, ColTable of a backward epilogue launch): `lanes` of its
// static dims from merged index t.total on; columns are absolute in the parent arrays.
template <class Table>
void append_member(Table &t, const mlpg_hip_stream_t &sm, int stat_col, int lanes) {
  t.begin[t.n] = t.total;
  t.in_col[t.n] = sm.in_col;
  t.out_col[t.n] = sm.out_col;
  t.sd[t.n] = sm.static_dim;
  t.stat_col[t.n] = stat_col;
  t.total += lanes;
  ++t.n;
}

// Asks the kernel family `algo` names for one stream (or piece) before anything is enqueued.  Pure host logic.
int check_stream_algo(const char *who, int k, int dtype, int algo, const Problem &p, const WinSet &ws) {
  if (!check_algo(dtype, dtype, algo, p, ws)) return 0;
  char why[400];
  snprintf(why, sizeof(why), "%s", mlpg_hip_last_error());
  set_error("%s: stream %d: %s", who, k, why);
  return MLPG_HIP_EINVAL;
}

// The one refusal the FIR form can only give with its tap table in hand (built on first use per window set; the device is current):
// asked for every stream under MLPG_HIP_ALGO_FIR, so that no stream is solved before another one is refused.
int check_stream_fir(const char *who, int k, hipStream_t st, int device, const WinSet &ws) {
  if (fir_table_ready(st, device, ws)) return 0;
  set_error("%s: stream %d: MLPG_HIP_ALGO_FIR: the inverse of this window set does not decay to 2^-26 within 24 frames (or the stream "
            "is being captured before the tap table exists)", who, k);
  return MLPG_HIP_EINVAL;
}

// ---- plan (forward) ---------------------------------------------------------------------------------------------------------------

// One stream, or the piece of the cut stream, that a launch of its own solves (or copies: a pass-through stream).
struct StreamRun {
  int k;      // the stream's table index
  Problem p;
  int algo;   // the family asked for: the call's, but AUTO for a piece under CONST / CHUNK / FIR
  bool tr;    // dispatch_solve will hand it to the transposed strip form: a persistent grid like the merged launch's
};

// What one mlpg_hip_forward_streams call launches, decided by plan_streams before anything is enqueued.
struct StreamPlan {
  // The merged launch: streams with the same three windows share ONE launch, their static dims side by side on the lanes.
  bool merged, merge_strip;  // there is one; on the strip kernel (per-frame variances), else on the constant-coefficient kernel
  StreamMap smap;
  Problem p_merged;          // the parent arrays
  int ws_of;                 // the member whose WinSet the launch uses (all members' are equal)
  bool member[kMaxStreams];  // stream k is a WHOLE member
  int cap;                   // the lanes the launch may hold
  int piece_stream, piece_first;  // stream cut between the merged launch (dims < piece_first) and a run of its own; -1: none
  // Every other stream with static dims, and the piece, in table order.
  int widest;                // the stream that goes last on the caller's stream (-1 with a merged launch: that one takes its place)
  int nruns, n_side;
  StreamRun run[kMaxStreams];
  // Enqueue order, as indices into run[]: order[0, n_side) beside the caller's stream (side streams while they last), in front of the
  // merged launch; order[n_side, nruns) on the caller's stream behind it -- the transposed-form runs, the widest stream last.
  int order[kMaxStreams];
};

// The run of stream k, or of its static dims [d_first, d_first + d_count).
StreamRun stream_run(const StreamCall &c, int k, int algo, const void *mean, void *out, const WinSet *wsets, int d_first = 0,
                     int d_count = -1) {
  StreamRun r;
  r.k = k;
  r.p = stream_problem(c, k, false, mean, nullptr, out, d_first, d_count);
  // a piece of a stream (what a merged launch left over) goes to the kernels that take the window pitch separately, whatever
  // kernel was asked for the call as a whole
  const bool to_auto = r.p.pitch && (algo == MLPG_HIP_ALGO_CONST || algo == MLPG_HIP_ALGO_CHUNK || algo == MLPG_HIP_ALGO_FIR);
  r.algo = to_auto ? MLPG_HIP_ALGO_AUTO : algo;
  // A stream (or piece) that takes the transposed strip form is a persistent grid like the merged launch's: it is queued on the
  // caller's stream behind that one instead of beside it on a side stream (two persistent grids that share the device each hold
  // fewer workgroups than their work lists were dealt for).
  r.tr = c.streams[k].num_windows == 3 && takes_strip_tr(c.dtype, r.algo, r.p, wsets[k]);
  return r;
}

// The merged launch of a call, if it makes one: fills pl->merged, merge_strip, smap, p_merged, ws_of, member[], cap, piece_*.
void plan_merged_launch(const StreamCall &c, int algo, const void *mean, void *out, const WinSet *wsets, StreamPlan *pl) {
  pl->merged = false;
  pl->cap = 0;
  pl->piece_stream = -1;
  pl->piece_first = 0;
  pl->ws_of = -1;
  memset(pl->member, 0, sizeof(pl->member));
  // Streams with the same three windows (extent <= 1) and per-frame variances can share ONE strip-kernel launch: their
  // static dims sit side by side on the lanes (66 = 60 + 1 + 5 dims of a Merlin-style row: one group of 64 and one of
  // 2), every row of the batch is fetched once instead of once per stream.  Taken when it does not add lane groups
  // and the launch is one the strip kernel would be chosen for anyway.
  // Global (D,) and unit variances (round 5): the same packing, on the constant-coefficient kernel (one workgroup walks one
  // (utterance, group of 64 lanes) sequence: 60 + 1 + 3 dims of a Merlin-style row in one group, the other 2 bap dims as a piece).
  pl->merge_strip = (algo == MLPG_HIP_ALGO_AUTO || algo == MLPG_HIP_ALGO_STRIP) && c.var_mode == MLPG_HIP_VAR_FRAME;
  const bool merge_const = (algo == MLPG_HIP_ALGO_AUTO || algo == MLPG_HIP_ALGO_CONST) &&
                           (c.var_mode == MLPG_HIP_VAR_GLOBAL || c.var_mode == MLPG_HIP_VAR_UNIT);
  if (!pl->merge_strip && !merge_const) return;
  // candidates: the streams whose packed window set equals, byte for byte, that of the first stream with three windows of extent <= 1
  int cand[kMaxStreams], cnt = 0, total = 0;
  for (int k = 0; k < c.n; ++k) {
    const mlpg_hip_stream_t &sm = c.streams[k];
    if (sm.static_dim <= 0 || sm.num_windows != 3 || wsets[k].mw > 1) continue;
    if (cnt > 0 && memcmp(&wsets[k], &wsets[cand[0]], sizeof(WinSet)) != 0) continue;
    cand[cnt++] = k;
    total += sm.static_dim;
  }
  if (cnt < 2) return;
  pl->ws_of = cand[0];
  // (Round 6 measured NOT merging for global / unit variances when every narrow member would take the transposed strip form on its own:
  // config 5 in one call 0.73 ms against 0.64-0.65 ms merged -- although the same three launches as three calls sum to 0.61 ms.  Merged.)
  // The merged launch holds full groups of 64 lanes only: a last group of a few lanes would hold its workgroup slots
  // as long as a full group's while moving almost nothing (66 dims in one launch: 1.39 ms on the config-5 batch, the
  // full row in 64 lanes + the rest alone: see DESIGN.md).  So when the dims do not fill their last group at least half,
  // the streams are packed greedily (widest first) into the full groups and the others run on their own as before.
  int cap = total;
  if (total > 64 && total % 64 < 32) cap = total - total % 64;
  pl->cap = cap;
  // widest first (insertion sort, stable), then greedy
  for (int i = 1; i < cnt; ++i)
    for (int j = i; j > 0 && c.streams[cand[j]].static_dim > c.streams[cand[j - 1]].static_dim; --j) {
      const int t_ = cand[j]; cand[j] = cand[j - 1]; cand[j - 1] = t_;
    }
  StreamMap &smap = pl->smap;
  memset(&smap, 0, sizeof(smap));
  for (int q = 0; q < 4; ++q) smap.begin[q] = INT_MAX;
  for (int i = 0; i < cnt && smap.n < 4; ++i) {
    const mlpg_hip_stream_t &sm = c.streams[cand[i]];
    if (smap.total + sm.static_dim > cap) continue;
    append_member(smap, sm, c.status_cols[cand[i]], sm.static_dim);
    pl->member[cand[i]] = true;
  }
  // lanes left over: the first dims of one more stream; the rest of it runs as a piece (wave-per-system kernel)
  if (smap.total < cap && smap.n < 4)
    for (int i = 0; i < cnt; ++i) {
      const int k = cand[i];
      if (pl->member[k]) continue;
      pl->piece_stream = k;
      pl->piece_first = cap - smap.total;
      append_member(smap, c.streams[k], c.status_cols[k], pl->piece_first);
      break;
    }
  const int pos = smap.total;
  bool ok = smap.n >= 2 && (pos + 63) / 64 <= smap.n;
  if (ok) {
    const WinSet &ws = wsets[pl->ws_of];
    Problem &p = pl->p_merged;
    p = dense_problem(mean, c.var, nullptr, c.lengths, out, c.status, false, c.var_mode, c.B, c.Tmax, 3 * pos, pos);
    p.ld_in = c.ld_in;
    p.ld_out = c.ld_out;
    p.ld_status = (int)c.sd_total;
    if (pl->merge_strip) {
      // the decision the widest group would get alone (long utterances, or enough 64-frame strips)
      Problem pw = p;
      pw.sd = pos < 64 ? pos : 64;
      pw.D = 3 * pw.sd;
      ok = strip_supported(p, ws) && (algo == MLPG_HIP_ALGO_STRIP || strip_preferred(pw, ws, false, c.dtype));
    } else {
      // the constant-coefficient kernel's conditions (const_supported / const_preferred for groups of 64 lanes): a dynamic
      // window of extent 1, and about a sequence per CU
      ok = ws.mw == 1 && rows_fit_buffer(p) && (algo == MLPG_HIP_ALGO_CONST || (long)c.B * ((pos + 63) / 64) >= 192);
    }
  }
  pl->merged = ok;
  if (!ok) {
    memset(pl->member, 0, sizeof(pl->member));
    pl->piece_stream = -1;
  }
}

// The whole plan of a forward call.  Pure host logic: no HIP call, no allocation.
// The streams are independent: the widest one runs on the caller's stream, every other one on a side stream of
// this device that is forked from and joined back into the caller's stream with events (no host synchronisation,
// capturable), so that a narrow stream's launch fills the tail of the wide one instead of queueing behind it.
void plan_streams(const StreamCall &c, int algo, const void *mean, void *out, const WinSet *wsets, StreamPlan *pl) {
  plan_merged_launch(c, algo, mean, out, wsets, pl);
  pl->widest = -1;
  for (int k = 0; k < c.n && !pl->merged; ++k)  // (with a merged launch, that one takes the caller's stream)
    if (c.streams[k].static_dim > 0 &&
        (pl->widest < 0 || c.streams[k].static_dim * (c.streams[k].num_windows + 1) >
                               c.streams[pl->widest].static_dim * (c.streams[pl->widest].num_windows + 1)))
      pl->widest = k;
  pl->nruns = 0;
  for (int k = 0; k < c.n; ++k) {
    const mlpg_hip_stream_t &sm = c.streams[k];
    if (sm.static_dim <= 0 || pl->member[k]) continue;
    const bool piece = k == pl->piece_stream;
    pl->run[pl->nruns++] = stream_run(c, k, algo, mean, out, wsets, piece ? pl->piece_first : 0, piece ? sm.static_dim - pl->piece_first : -1);
  }
  int n = 0;
  for (int i = 0; i < pl->nruns; ++i)
    if (pl->run[i].k != pl->widest && !pl->run[i].tr) pl->order[n++] = i;
  pl->n_side = n;
  for (int i = 0; i < pl->nruns; ++i)
    if (pl->run[i].k != pl->widest && pl->run[i].tr) pl->order[n++] = i;
  for (int i = 0; i < pl->nruns; ++i)
    if (pl->run[i].k == pl->widest) pl->order[n++] = i;
}

// ---- enqueue -----------------------------------------------------------------------------------------------------------------------

int enqueue_run(const StreamCall &c, const StreamRun &r, const WinSet *wsets, hipStream_t st, int device) {
  const mlpg_hip_stream_t &sm = c.streams[r.k];
  if (sm.num_windows > 0) return dispatch_solve(st, c.dtype, c.dtype, r.algo, false, r.p, wsets[r.k], device);
  if (int rc = launch_copy_cols(st, c.dtype, r.p.mean, c.ld_in, c.lengths, c.B, c.Tmax, r.p.sd, r.p.out, c.ld_out)) return rc;
  if (c.status)  // pass-through streams cannot fail: their status columns are cleared
    MLPG_HIP_CHECK(hipMemset2DAsync(r.p.status, sizeof(int32_t) * (size_t)c.sd_total, 0, sizeof(int32_t) * (size_t)sm.static_dim,
                                    (size_t)c.B, st));
  return 0;
}

// The merged launch; where the grid cannot hold an utterance (nothing was enqueued): its members one after the other.
int enqueue_merged(const StreamCall &c, const StreamPlan &pl, int algo, const void *mean, void *out, const WinSet *wsets,
                   hipStream_t st, int device) {
  const WinSet &ws = wsets[pl.ws_of];
  const int rc = pl.merge_strip ? launch_strip_multi(st, c.dtype, pl.p_merged, ws, pl.smap, device)
                                : launch_const_multi(st, c.dtype, pl.p_merged, ws, pl.smap, device);
  if (rc != strip::kNotResident) return rc;
  for (int k = 0; k < c.n; ++k)
    if (pl.member[k])
      if (int rc2 = enqueue_run(c, stream_run(c, k, algo, mean, out, wsets), wsets, st, device)) return rc2;
  if (pl.piece_stream < 0) return 0;  // and the head of the cut stream
  return enqueue_run(c, stream_run(c, pl.piece_stream, algo, mean, out, wsets, 0, pl.piece_first), wsets, st, device);
}

int enqueue_streams(const StreamCall &c, const StreamPlan &pl, int algo, const void *mean, void *out, const WinSet *wsets,
                    hipStream_t main_st, int device) {
  SideStreams *side = side_streams(device);
  // one caller at a time per device: the side streams and their fork/join events are shared
  std::unique_lock<std::mutex> side_lock;
  if (side) side_lock = std::unique_lock<std::mutex>(side->mu);
  int nside = 0;
  // The fork is recorded BEFORE anything of this call is queued on the caller's stream and the widest stream is
  // launched last: the narrow streams' kernels then only wait for what preceded the call, not for the wide kernel.
  if (side && pl.n_side > 0) MLPG_HIP_CHECK(hipEventRecord(side->fork, main_st));
  auto join_side = [&]() -> int {  // also on the error paths: an unjoined side stream would break a graph capture
    for (int q = 0; q < nside; ++q) {
      MLPG_HIP_CHECK(hipEventRecord(side->join[q], side->st[q]));
      MLPG_HIP_CHECK(hipStreamWaitEvent(main_st, side->join[q], 0));
    }
    nside = 0;
    return 0;
  };
  auto enqueue_all = [&]() -> int {
    for (int i = 0; i < pl.n_side; ++i) {
      hipStream_t st = main_st;
      if (side && nside < SideStreams::kN) {
        st = side->st[nside];
        if (hipStreamWaitEvent(st, side->fork, 0) != hipSuccess) {
          (void)hipGetLastError();
          st = main_st;
        } else {
          ++nside;
        }
      }
      if (int rc = enqueue_run(c, pl.run[pl.order[i]], wsets, st, device)) return rc;
    }
    if (pl.merged)
      if (int rc = enqueue_merged(c, pl, algo, mean, out, wsets, main_st, device)) return rc;
    for (int i = pl.n_side; i < pl.nruns; ++i)
      if (int rc = enqueue_run(c, pl.run[pl.order[i]], wsets, main_st, device)) return rc;
    return 0;
  };
  if (int rc = enqueue_all()) {
    (void)join_side();
    return rc;
  }
  return join_side();
}

// The epilogue of a backward call: one launch per window list for the variance gradient (where grad_var is given), one for all
// pass-through streams.
int enqueue_bwd_epilogue(const StreamCall &c, const WinSet *wsets, hipStream_t st, const void *mean, const void *y, const void *grad_out,
                         void *grad_mean, void *grad_var) {
  bool done[kMaxStreams] = {};
  static thread_local ColTable ct;
  for (int k = 0; k < c.n && grad_var; ++k) {
    const mlpg_hip_stream_t &sm = c.streams[k];
    if (done[k] || !dynamic(sm)) continue;
    memset(&ct, 0, sizeof(ct));
    for (int j = k; j < c.n; ++j) {
      const mlpg_hip_stream_t &sj = c.streams[j];
      if (done[j] || sj.static_dim == 0 || sj.num_windows != sm.num_windows || sj.win_first != sm.win_first) continue;
      done[j] = true;
      append_member(ct, sj, c.status_cols[j], sj.static_dim);
    }
    if (int rc = launch_streams_bwd(st, c.dtype, c.var_mode, grad_out, c.var, mean, y, c.lengths, c.status, c.B, c.Tmax, c.ld_in, c.ld_out,
                                    (int)c.sd_total, ct, wsets[k], grad_mean, grad_var))
      return rc;
  }
  memset(&ct, 0, sizeof(ct));
  for (int k = 0; k < c.n; ++k)
    if (c.streams[k].num_windows == 0 && c.streams[k].static_dim != 0) append_member(ct, c.streams[k], c.status_cols[k], c.streams[k].static_dim);
  if (ct.n == 0) return 0;
  WinSet none;
  memset(&none, 0, sizeof(none));
  return launch_streams_bwd(st, c.dtype, kStreamsBwdPass, grad_out, nullptr, nullptr, nullptr, c.lengths, c.status, c.B, c.Tmax, c.ld_in,
                            c.ld_out, (int)c.sd_total, ct, none, grad_mean, grad_var);
}

}  // namespace
}  // namespace mlpg

using namespace mlpg;

extern "C" {

__attribute__((visibility("default"))) int mlpg_hip_forward_streams(
    int device, void *stream, int dtype, int algo, const void *mean, const void *var, int var_mode, int64_t ld_in,
    const int32_t *lengths, int B, int Tmax, int num_streams, const mlpg_hip_stream_t *streams_h, int total_windows,
    const int32_t *win_l_h, const int32_t *win_u_h, const double *win_coef_h, void *out, int64_t ld_out,
    int32_t *status) {
  const char *who = "forward_streams";
  static thread_local StreamCall c;
  static thread_local WinSet wsets[kMaxStreams];
  static thread_local StreamPlan plan;
  // ---- every refusal comes before the first launch: a refused call writes nothing and moves no counter ----
  if (int rc = check_stream_table(who, device, dtype, algo, var, var_mode, ld_in, ld_out, lengths, B, Tmax, num_streams, streams_h,
                                  total_windows, win_l_h, win_u_h, win_coef_h, status, &c))
    return rc;
  if (int rc = pack_stream_windows(who, c, wsets)) return rc;
  if (B == 0 || Tmax == 0 || c.sd_total == 0) return 0;
  if (!mean || !out) {
    set_error("%s: NULL data pointer", who);
    return MLPG_HIP_EINVAL;
  }
  plan_streams(c, algo, mean, out, wsets, &plan);
  for (int i = 0; i < plan.nruns; ++i) {
    const StreamRun &r = plan.run[i];
    if (c.streams[r.k].num_windows > 0) {
      if (int rc = check_stream_algo(who, r.k, dtype, r.algo, r.p, wsets[r.k])) return rc;
    } else if (!elementwise_grid_fits(c.B, c.Tmax, r.p.sd)) {  // (a pass-through stream: one launch of copy_cols, a thread per element)
      set_error("%s: stream %d: B * Tmax * static_dim = %d * %d * %d elements to copy are more than the %ld workgroups of 256 threads one "
                "launch takes: a grid is 32 bits of threads", who, r.k, c.B, c.Tmax, r.p.sd, max_workgroups(256));
      return MLPG_HIP_EINVAL;
    }
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  for (int i = 0; i < plan.nruns; ++i) {
    const StreamRun &r = plan.run[i];
    if (r.algo == MLPG_HIP_ALGO_FIR && c.streams[r.k].num_windows > 0)
      if (int rc = check_stream_fir(who, r.k, (hipStream_t)stream, device, wsets[r.k])) return rc;
  }
  return enqueue_streams(c, plan, algo, mean, out, wsets, (hipStream_t)stream, device);
}

__attribute__((visibility("default"))) int mlpg_hip_backward_streams(
    int device, void *stream, int dtype, int algo, const void *mean, const void *var, int var_mode, int64_t ld_in, const void *y,
    const void *grad_out, int64_t ld_out, const int32_t *lengths, int B, int Tmax, int num_streams,
    const mlpg_hip_stream_t *streams_h, int total_windows, const int32_t *win_l_h, const int32_t *win_u_h,
    const double *win_coef_h, void *grad_mean, void *grad_var, int32_t *status) {
  const char *who = "backward_streams";
  static thread_local StreamCall c;
  static thread_local WinSet wsets[kMaxStreams];
  static thread_local Problem probs[kMaxStreams];
  // ---- every refusal comes before the first launch: a refused call writes nothing and moves no counter ----
  if (int rc = check_stream_table(who, device, dtype, algo, var, var_mode, ld_in, ld_out, lengths, B, Tmax, num_streams, streams_h,
                                  total_windows, win_l_h, win_u_h, win_coef_h, status, &c))
    return rc;
  if (grad_var && var_mode == MLPG_HIP_VAR_UNIT) {
    set_error("%s: unit variances (MLPG_HIP_VAR_UNIT) have no variances to differentiate (pass grad_var = NULL)", who);
    return MLPG_HIP_EINVAL;
  }
  if (grad_var && !status) {
    set_error("%s: grad_var needs status (int32, B * sum static_dim): a failing system's gradients are zeroed from it", who);
    return MLPG_HIP_EINVAL;
  }
  if (int rc = pack_stream_windows(who, c, wsets)) return rc;
  if (B == 0 || Tmax == 0 || c.sd_total == 0) return 0;
  if (!grad_out || !grad_mean || (grad_var && c.any_dynamic && (!mean || !y))) {
    set_error("%s: NULL data pointer (grad_out and grad_mean are required; mean and y too when grad_var is given)", who);
    return MLPG_HIP_EINVAL;
  }
  if (!streams_bwd_fits(B, Tmax, (int)(c.sd_total > INT32_MAX ? INT32_MAX : c.sd_total)) || c.sd_total > INT32_MAX) {
    set_error("%s: batch too large", who);
    return MLPG_HIP_EINVAL;
  }
  for (int k = 0; k < num_streams; ++k) {
    if (!dynamic(streams_h[k])) continue;
    probs[k] = stream_problem(c, k, true, nullptr, grad_out, grad_mean);
    if (int rc = check_stream_algo(who, k, dtype, algo, probs[k], wsets[k])) return rc;
  }
  DeviceGuard g(who, device);
  if (g.rc) return g.rc;
  hipStream_t st = (hipStream_t)stream;
  for (int k = 0; k < num_streams && algo == MLPG_HIP_ALGO_FIR; ++k)
    if (dynamic(streams_h[k]))
      if (int rc = check_stream_fir(who, k, st, device, wsets[k])) return rc;
  // ---- the solves: every dynamic stream through the backward dispatcher on its column slice, in table order, on the caller's stream
  // (no side streams: two persistent strip grids side by side are only co-resident by construction in the forward plan) ----
  for (int k = 0; k < num_streams; ++k)
    if (dynamic(streams_h[k]))
      if (int rc = dispatch_solve(st, dtype, dtype, algo, true, probs[k], wsets[k], device)) return rc;
  return enqueue_bwd_epilogue(c, wsets, st, mean, y, grad_out, grad_mean, grad_var);
}

}  // extern "C"
