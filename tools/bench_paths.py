#!/usr/bin/env python
"""Secondary measurements (1 GPU) for the other BASELINE.json configs; one JSON line per path.

    python tools/bench_paths.py [--quick]

  lit : the LITERAL drop-in calls: one numpy -> numpy paramgen.mlpg per utterance at BASELINE config 1 and at one config-2
        utterance, the reference's loop shape over 256 utterances, autograd.mlpg on CPU tensors, DTWAligner.transform on one
        pair -- wall clock per call beside the reference's on the same host (litq: without the reference's 7 s mlpg_grad)
  c2h : config 2 end to end from host memory (numpy -> numpy), PCIe-inclusive wall clock
  c2g : config 2 with global (D,) variances and with unit variances (32 B per (frame, dim))
  c3  : autograd.unit_variance_mlpg forward+backward, B=64 x T=500 x 180, float32 tensors on the GPU
  c3m : autograd.mlpg (generic variances) forward+backward, one utterance T=500 x 180 float32
  c4  : DTWAligner on 128 pairs (1 GPU share of config 4), T in [700, 900], 25-dim, radius 1
  ms  : modspec_smoothing / modspec (n = 4096) of a config-2 sized trajectory batch 256 x 1000 x 60, float64
  c5  : Merlin-style acoustic paramgen mgc(60)+lf0(1)+bap(5), T=2000, B=512 (1 GPU share of config 5), float64;
        per-stream dense tensors, and the three streams in place from one (B, T, 198) batch (forward_streams)
  msb : (only with --only msb) forward + backward of the log-MS loss over a padded 256 x 1000 x 60 minibatch, lengths in
        [600, 1000], float32 and float64, n = 2048 and 4096: (a) a Python loop of autograd.modspec + torch ops, (b)
        autograd.modspec_batch + torch ops, (c) the fused autograd.modspec_mse_loss
  c5b : (only with --only c5b) forward + backward of the same (512, 2000, 198) batch with gradients for means and variances:
        autograd.multi_stream_mlpg in place against three mlpg_batch on .contiguous() slices plus cat; the epilogue kernel's share
  gmm : (only with --only gmm) one aligner iteration's joint-GMM fit at config 4 (128 pairs, T in [700, 900], 25 dims: F = 50,
        K = 16, max_iter = 100) by scikit-learn on the host and by mixture.fit_gaussian_mixture from the same start: wall time,
        iterations run, milliseconds per EM iteration of each of the three kernels; also written to profiles/gmm_em.json
        (NNMNKWII_GMM_PROFILE names another file)
  kmeans : (only with --only kmeans) the start of that fit on the same joint matrix with one seed: GaussianMixture(max_iter=0).fit
        on the host against mixture.fit_gaussian_mixture(init="kmeans", max_iter=0): wall time of both, Lloyd iterations of both,
        milliseconds per seed step and per Lloyd step; also written to profiles/kmeans.json (NNMNKWII_KMEANS_PROFILE names
        another file)
  postfilter : (only with --only postfilter) the Merlin post-filter over a padded 512 x 2000 x 60 mgc batch at the defaults (order
        511, fftlen 1024), lengths in [1200, 2000], float64 and float32: milliseconds per call, the achieved fraction of the float64
        matrix peak (flops = valid frames * 2 * 513 * 60 * 2), the numpy model's time per frame on the host as context; also
        written to profiles/postfilter.json (NNMNKWII_POSTFILTER_PROFILE names another file)
  msfilter : (only with --only msfilter) the modulation-spectrum post-filter plus low-pass smoothing (tables and cutoff, n = 4096)
        over the 60 mgc columns of a padded 512 x 2000 x 187 batch, lengths in [1200, 2000], float32 and float64: (a) the one launch
        of mlpg_hip_modspec_filter on the column slice, (b) the same filter composed from modspec with phase, torch arithmetic and
        inv_modspec on float64 copies; milliseconds of both, their ratio, the fraction of the HBM floor (x read plus result written
        at 8 TB/s); also written to profiles/msfilter.json (NNMNKWII_MSFILTER_PROFILE names another file)
  vc : (only with --only vc) trajectory GMM voice conversion of a corpus: 256 utterances, T in [700, 900], 24 static dims x 3
        windows (D = 72), M = 64, posterior="device": (a) the loop of MLPG.transform, (b) MLPG.transform_batch, (c) transform_padded
        on a resident tensor and its three launches, (d) mlpg_hip_gmm_trajectory_stats against gmm_convert(mixture=labels) plus
        cvar[labels], alternating; medians with their spread, and the stats kernel's bytes over time beside the 8 TB/s peak; also
        written to profiles/gmm_vc.json (NNMNKWII_GMM_VC_PROFILE names another file)
  gv : (only with --only gv) MLPG with the gv likelihood on the corpus of vc, 100 iterations: the one launch of mlpg_hip_gv_ascent
        against the same iteration composed from torch operations on resident tensors (banded product by shifted slices),
        alternating; medians with [min, max], the ratio and the agreement of the two routes; also written to
        profiles/gvmlpg.json (NNMNKWII_GVMLPG_PROFILE names another file)
  norm : (only with --only norm) corpus normalisation over a padded 512 x 2000 x 187 batch, lengths in [1000, 2000], float32 and
        float64: one mlpg_hip_column_stats call against the same five statistics composed from masked torch reductions, and
        mlpg_hip_column_affine (scale, inv_scale) against the broadcast torch expression plus masking; milliseconds and the
        fraction of 8 TB/s; also written to profiles/norm.json (NNMNKWII_NORM_PROFILE names another file)
  metrics : (only with --only metrics) the four-term Merlin evaluation (mgc MCD, bap distortion, lf0 RMSE, V/UV error) over a padded
        512 x 2000 x 187 float32 prediction / target pair, lengths in [1000, 2000]: one nnmk_metrics_batch call against the
        reference's per-utterance loop and against masked vectorised torch expressions on the same tensors; milliseconds and the
        fraction of 8 TB/s; also written to profiles/metrics.json (NNMNKWII_METRICS_PROFILE names another file)
  frontend : (only with --only frontend) phone-level linguistic features expanded to frames: 512 utterances of 60 .. 100 phones x 5
        states, 1000 .. 2000 frames each, Dl = 416, kind full, float32 (512, 2000, 425) out, without and with the fused affine map:
        one nnmk_frontend_expand launch against the same result composed from torch operations and against the specification's
        per-frame loop on eight utterances (scaled); milliseconds and the fraction of 8 TB/s; also written to
        profiles/frontend.json (NNMNKWII_FRONTEND_PROFILE names another file)
  f0 : (only with --only f0) continuous F0 over a padded 512 x 2000 x 187 float32 batch, lengths in [1000, 2000], about 40 % of the lf0
        column unvoiced in runs: one nnmk_f0_interp launch that fills the column and writes the V/UV flag, against torch's plain
        copy and fill of the same bytes, the same result composed from torch operations, and the reference-style per-utterance
        loop over host copies (scaled); milliseconds per call over windows of back-to-back calls with their spread; also written
        to profiles/f0.json (NNMNKWII_F0_PROFILE names another file)
  wave : (only with --only wave) the waveform codec at float32 32 x 160000 and 512 x 16000, lengths in [Lmax / 2, Lmax]: one
        nnmk_wave_encode launch (pre-emphasis, mu-law, int16 classes) and one nnmk_wave_decode launch (table, de-emphasis; at the
        built-in segment length, 16384, 65536 and unsplit) against torch's plain copy of the same bytes, the same result composed
        from torch operations, and the per-utterance host loop through the reference's expressions (scaled); protocol as f0;
        also written to profiles/wave.json (NNMNKWII_WAVE_PROFILE names another file)
  joint : (only with --only joint) the joint rows of 512 aligned pairs, Tmax = 2000, lengths in [1000, 2000], 60-dim float32 with
        column 0 dropped, static + delta + delta-delta, float64 rows (W = 354), about 5 % silent frames: nnmk_joint_count and
        nnmk_joint_write together and apart, the LIVE keep rule, the same rows composed from delta_features and torch operations,
        torch's plain copy of the rows the write stage stores, and the reference-style per-utterance host loop (scaled); protocol
        as f0; also written to profiles/joint.json (NNMNKWII_JOINT_PROFILE names another file)
  trajcov : (only with --only trajcov) the trajectory covariance (nnmk_traj_covariance: band of R^-1, log det R) and covariance +
        likelihood with both gradients (nnmk_traj_nll) at float64 256 x 1000 x 180, lengths in [500, 1000], per-frame variances:
        each against torch's plain copy of the bytes it must move, and -- at 8 x 500 x 180, where the dense matrices fit -- against
        the composed route (batched dense torch.linalg.inv / logdet, and autograd of the dense likelihood); protocol as f0; also
        written to profiles/trajcov.json (NNMNKWII_TRAJCOV_PROFILE names another file)
  trajsample : (only with --only trajsample) draws from the trajectory distribution at the same shape: nnmk_draw_factor (against
        nnmk_traj_covariance's forward sweep), nnmk_draw_sample at K = 1, kDrawGroup and 16, nnmk_draw_whiten at K = 1, each against
        torch's plain copy of the bytes it must move, and -- at 8 x 500 x 180 -- against the composed route (dense R, torch's Cholesky
        factor, a triangular solve); protocol as f0; also written to profiles/trajsample.json (NNMNKWII_TRAJSAMPLE_PROFILE names
        another file)

Each line carries the GPU time (HIP events on the launch stream), the algorithmic bytes, GB/s, and a
bounded CPU baseline from the oracle on the same host (the checker, timed like bench.py's cpu_baseline).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]


def gpu_time(fn, steps=10, warmup=2, settle_ms=None):
    """Median HIP-event time of one call.  After the warm-up calls the function is run for about `settle_ms` of device time
    (default 25, NNMNKWII_BENCH_SETTLE_MS; at most 400 calls) before the timed calls: the device's clocks take tens of milliseconds
    of work to settle and fall back within milliseconds of idling (profiles/r05_notes.md section 18), and every path here is
    measured behind a pause."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if settle_ms is None:
        settle_ms = float(os.environ.get("NNMNKWII_BENCH_SETTLE_MS", "25"))
    if settle_ms > 0:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        for _ in range(int(min(400, settle_ms / max(a.elapsed_time(b), 1e-3)))):
            fn()
    evs = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs]))


def wall_time(fn, steps=1000, warmup=50, repeats=3):
    """Wall-clock milliseconds per call over a back-to-back loop with one synchronize at its end (best of `repeats`): what a
    training loop sees, and how the reference times its own loop (perf/autograd_mlpg_perf.py:56-86: time.time() around the loop).
    For host-bound steps the event pair of gpu_time() around every single call reads 1.5-2.5 x this (profiles/r06_notes.md section 10)."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / steps * 1e3)
    return best


HBM_PEAK_GBS = 8000.0
F64_MATRIX_PEAK_TFLOPS = 78.6     # AMD's published float64 matrix rate of the MI355X (v_mfma_f64_16x16x4_f64)


_SINK = None      # run(sink=[...]) collects the lines instead of printing them (bench.py's `secondary` object)


def emit(**kw):
    if "GBps" in kw and kw["GBps"] is not None:
        kw["roofline_frac"] = kw["GBps"] / HBM_PEAK_GBS      # algorithmic bytes / time against the 8 TB/s HBM3E peak
    if _SINK is not None:
        _SINK.append(kw)
    else:
        print(json.dumps(kw), flush=True)


def fastdtw_window_cells(x, y, radius=1):
    """DP cells fastdtw visits for one pair, over all levels of the halving pyramid (the kernel's work measure beside
    bytes): the full matrix at the coarsest level, else the per-row intervals that upstream's __expand_window builds
    from the coarser path (union of (2r+1)^2 neighbourhoods, each coarse cell = 2x2 fine cells, one run per row)."""
    from oracle import dtw as OD
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if len(x) < radius + 2 or len(y) < radius + 2:
        return len(x) * len(y)
    xs = (x[0:len(x) - len(x) % 2:2] + x[1:len(x):2][: len(x) // 2]) / 2
    ys = (y[0:len(y) - len(y) % 2:2] + y[1:len(y):2][: len(y) // 2]) / 2
    cells = fastdtw_window_cells(xs, ys, radius)
    _, path = OD.fastdtw(xs, ys, radius)
    lo = np.full(len(xs) + 2 * radius + 2, 1 << 30)
    hi = np.full(len(xs) + 2 * radius + 2, -1)
    for i, j in path:
        for a in range(-radius, radius + 1):
            r = i + a + radius
            lo[r] = min(lo[r], j - radius)
            hi[r] = max(hi[r], j + radius)
    tot = 0
    for i in range(len(x)):
        r = i // 2 + radius
        if hi[r] < 0:
            continue
        tot += min(2 * hi[r] + 1, len(y) - 1) - max(2 * lo[r], 0) + 1
    return cells + tot


def _wall_us(fn, n, warm=5):
    """(median, min) wall-clock microseconds of one call of fn (host clock: these are host-memory calls)."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6, float(np.min(ts)) * 1e6


def literal_calls(emit, quick=False, long_reference_backward=True):
    """The drop-in API exactly as `north_star` names it and as the reference's users call it: ONE numpy -> numpy
    `paramgen.mlpg(mean_frames (T, D), variance_frames, windows)` per utterance (paramgen/_mlpg.py:92), in a Python loop
    over utterances (util/__init__.py:56-66); `autograd.mlpg` on a CPU tensor; `DTWAligner.transform` on one pair.  Each
    beside the reference's own time on this host (oracle/_ref: the reference compiled unmodified; the checker, timed) and
    with the deviation from it.  Wall clock per call, everything included (staging, transfers, launch, synchronisation)."""
    import torch
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd import paramgen as G
    from nnmnkwii_amd.preprocessing.alignment import DTWAligner
    from oracle import dtw as OD
    from oracle import mlpg as O
    from oracle import ref
    Gref = ref.load() if ref.available() else None
    ref_mlpg = Gref.mlpg if Gref is not None else O.mlpg
    ref_kind = "reference (oracle/_ref)" if Gref is not None else "port (oracle/mlpg_oracle.c)"
    rng = np.random.RandomState(1234)
    n_small = 50 if quick else 300

    def one(name, m, v, n):
        y = G.mlpg(m, v, WINDOWS)
        yr = ref_mlpg(m, v, WINDOWS)
        err = float(np.abs(y - yr).max() / max(np.abs(yr).max(), 1e-300))
        us, us_min = _wall_us(lambda: G.mlpg(m, v, WINDOWS), n)
        rus, rus_min = _wall_us(lambda: ref_mlpg(m, v, WINDOWS), max(10, n // 5), warm=2)
        emit(path=name, us_per_call=us, us_per_call_min=us_min, cpu_us_per_call=rus, cpu_us_per_call_min=rus_min, cpu_kind=ref_kind,
             speedup_vs_cpu=rus / us, T=int(m.shape[0]), D=int(m.shape[1]), frames_per_s=m.shape[0] / us * 1e6,
             rel_err_vs_cpu=err, out_dtype=str(y.dtype))

    # BASELINE config 1: T = 100, 2 static dims, 3 windows (means = rng.rand(100, 6), vars = rng.rand(6) tiled)
    m1 = rng.rand(100, 6)
    v1g = rng.rand(6)
    v1 = np.tile(v1g, (100, 1))
    one("lit-c1-paramgen.mlpg-T100-sd2", m1, v1, n_small)
    one("lit-c1-paramgen.mlpg-T100-sd2-global-variances", m1, v1g, n_small)
    # one utterance of BASELINE config 2: T = 1000, 60 static dims, per-frame variances
    m2 = rng.randn(1000, 180)
    v2 = rng.rand(1000, 180) + 0.1
    one("lit-c2utt-paramgen.mlpg-T1000-sd60", m2, v2, n_small)
    m2f, v2f = m2.astype(np.float32), v2.astype(np.float32)
    one("lit-c2utt-paramgen.mlpg-T1000-sd60-float32", m2f, v2f, n_small)
    # the reference's loop shape over config 2: 256 utterances, one call each (distinct arrays: 5.8 MB per utterance)
    nu = 64 if quick else 256
    utts = [(rng.randn(1000, 180), rng.rand(1000, 180) + 0.1) for _ in range(nu)]
    for m, v in utts[:8]:
        G.mlpg(m, v, WINDOWS)
    t0 = time.perf_counter()
    ys = [G.mlpg(m, v, WINDOWS) for m, v in utts]
    loop_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    yr = [ref_mlpg(m, v, WINDOWS) for m, v in utts[:32]]
    ref_s = (time.perf_counter() - t0) * nu / 32
    err = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(ys, yr))
    t0 = time.perf_counter()
    yb = G.mlpg_batch(np.stack([m for m, _ in utts]), np.stack([v for _, v in utts]), WINDOWS)
    batch_s = time.perf_counter() - t0
    assert np.array_equal(yb[3], ys[3]) or float(np.abs(yb[3] - ys[3]).max()) < 1e-12
    emit(path="lit-c2-loop-per-utterance-calls", utterances=nu, ms=loop_s * 1e3, us_per_call=loop_s / nu * 1e6, frames_per_s=nu * 1000 / loop_s,
         cpu_ms=ref_s * 1e3, cpu_kind=ref_kind + ", 32 utterances timed, scaled", speedup_vs_cpu=ref_s / loop_s, rel_err_vs_cpu=err,
         ms_one_mlpg_batch_call_incl_stacking=batch_s * 1e3,
         note="[paramgen.mlpg(m, v, windows) for m, v in utterances]: the reference's own loop shape (util/__init__.py:56-66), numpy in, numpy out")
    del utts, ys, yr, yb
    # autograd.mlpg on CPU tensors (the reference's tensors are CPU tensors: autograd/_impl/mlpg.py:50-67), forward + backward.
    # One torch CPU thread, as the reference's CI pins it (OMP_NUM_THREADS=1, ci.yaml:16-17): with the default pool of one thread per
    # core (128 here) torch's own small CPU ops take milliseconds (a 60 k-element sum 27 us -> 2 us, an autograd step on (1000, 180) 2 ms -> 63 us,
    # tools/dbg/torch_cpu_threads.py) and its idle workers spin under the calls that follow; both sides of the comparison run under the same setting.
    torch_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    for name, T, sd, nrep in (("lit-c1-autograd.mlpg-cpu-tensor-T100-sd2", 100, 2, n_small), ("lit-c2utt-autograd.mlpg-cpu-tensor-T1000-sd60", 1000, 60, 30)):
        torch.manual_seed(1234)
        mt = torch.rand(T, 3 * sd, requires_grad=True)
        vt = torch.rand(T, 3 * sd) + 0.1

        def fb():
            mt.grad = None
            AF.mlpg(mt, vt, WINDOWS).sum().backward()

        us_f, _ = _wall_us(lambda: AF.mlpg(mt.detach(), vt, WINDOWS), nrep)
        us_fb, _ = _wall_us(fb, nrep)
        mn, vn = mt.detach().numpy(), vt.numpy()
        go_n = np.random.RandomState(5).randn(T, sd).astype(np.float32)
        us_g, _ = _wall_us(lambda: G.mlpg_grad(mn, vn, WINDOWS, go_n), nrep)    # the literal numpy -> numpy paramgen.mlpg_grad call

        class RefMLPG(torch.autograd.Function):
            # what the reference's node does (autograd/_impl/mlpg.py:50-67): paramgen.mlpg / mlpg_grad on .numpy() views
            @staticmethod
            def forward(ctx, means, variances):
                ctx.save_for_backward(means, variances)
                return torch.from_numpy(ref_mlpg(means.detach().numpy(), variances.detach().numpy(), WINDOWS))

            @staticmethod
            def backward(ctx, go):
                means, variances = ctx.saved_tensors
                return torch.from_numpy(Gref.mlpg_grad(means.detach().numpy(), variances.detach().numpy(), WINDOWS, go.numpy())), None

        rus_f, _ = _wall_us(lambda: RefMLPG.apply(mt.detach(), vt), 10, warm=1)
        rus_b = None
        if Gref is not None and (T <= 100 or (long_reference_backward and not quick)):
            go = np.ones((T, sd), dtype=np.float32)
            t0 = time.perf_counter()
            gr = Gref.mlpg_grad(mn, vn, WINDOWS, go)
            rus_b = (time.perf_counter() - t0) * 1e6
            fb()
            gerr = float(np.abs(mt.grad.numpy() - gr).max())
        else:
            gerr = None
        emit(path=name, us_forward=us_f, us_forward_backward=us_fb, us_paramgen_mlpg_grad=us_g, cpu_us_forward=rus_f, cpu_us_backward_mlpg_grad=rus_b,
             cpu_kind=ref_kind + " inside a torch.autograd.Function, as the reference's node calls it",
             grad_abs_err_vs_cpu=gerr, T=T, D=3 * sd, torch_cpu_threads=1)
    torch.set_num_threads(torch_threads)
    # paramgen.unit_variance_mlpg_matrix(windows, T) (a9: _mlpg.py:297-373; once per minibatch length in the reference's training loop)
    if not quick:
        for T in (100, 500):
            us_m, us_m_min = _wall_us(lambda: G.unit_variance_mlpg_matrix(WINDOWS, T), 10, warm=2)
            rus_m = merr = None
            if Gref is not None:
                t0 = time.perf_counter()
                Rr = Gref.unit_variance_mlpg_matrix(WINDOWS, T)
                rus_m = (time.perf_counter() - t0) * 1e6
                merr = float(np.abs(G.unit_variance_mlpg_matrix(WINDOWS, T) - Rr).max())
            emit(path="lit-unit_variance_mlpg_matrix-T%d" % T, us_per_call=us_m, us_per_call_min=us_m_min, cpu_us_per_call=rus_m, cpu_kind=ref_kind,
                 abs_err_vs_cpu=merr, speedup_vs_cpu=(rus_m / us_m if rus_m else None), T=T)
    # DTWAligner.transform on ONE pair (alignment.py:41-76 is a per-pair loop)
    a, b = 812, 777
    X = np.zeros((1, 900, 25))
    Y = np.zeros((1, 900, 25))
    X[0, :a] = np.cumsum(rng.randn(a, 25), 0) * 0.1
    Y[0, :b] = np.cumsum(rng.randn(b, 25), 0) * 0.1
    al = DTWAligner()
    Xa, Ya = al.transform((X, Y))
    Xo, Yo = OD.dtw_align(X, Y, 1, use_c=True)[:2]
    same = bool(np.array_equal(Xa, Xo) and np.array_equal(Ya, Yo))
    us, us_min = _wall_us(lambda: al.transform((X, Y)), 50 if quick else 200)
    cus, _ = _wall_us(lambda: OD.dtw_align(X, Y, 1, use_c=True), 10, warm=1)
    emit(path="lit-dtw-DTWAligner.transform-one-pair", us_per_call=us, us_per_call_min=us_min, cpu_us_per_call=cus,
         cpu_kind="oracle/dtw_oracle.c through oracle/dtw.py dtw_align (C restatement of fastdtw; the reference's pure-Python fastdtw package is absent)",
         aligned_arrays_equal_oracle=same, Tx=a, Ty=b, D=25)


def spread(ts):
    ts = np.sort(np.asarray(ts, dtype=np.float64))
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts[0]), max_ms=float(ts[-1]),
                q1_ms=float(np.percentile(ts, 25)), q3_ms=float(np.percentile(ts, 75)), n=int(len(ts)))


def events(fn, steps):
    """HIP-event milliseconds of `steps` calls of fn, one pair of events per call."""
    import torch
    evs = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def vc_corpus(quick, dev):
    """The synthetic corpus of --only vc and --only gv: 256 utterances (16 with --quick), T in [700, 900], 24 static dims x 3
    windows, a joint model of 64 separated components built directly.  Returns (g, utts, X, lens, Xd, Ld, B, sd, M, D, Tmax, frames)."""
    import torch
    from sklearn.mixture import GaussianMixture
    from nnmnkwii_amd.baseline.gmm import MLPG
    B, sd, M = (16, 24, 64) if quick else (256, 24, 64)
    D = sd * len(WINDOWS)
    rng = np.random.RandomState(1234)
    lens = rng.randint(700, 901, size=B).astype(np.int32)
    Tmax, frames = int(lens.max()), int(lens.sum())
    # a joint model built directly (no fit): separated means, well-conditioned full covariances
    F = 2 * D
    Q = rng.randn(M, F, F) / np.sqrt(F)
    cov = Q @ Q.transpose(0, 2, 1) + 0.5 * np.eye(F)
    gmm = GaussianMixture(n_components=M, covariance_type="full")
    gmm.weights_, gmm.means_, gmm.covariances_ = np.full(M, 1.0 / M), 1.5 * rng.randn(M, F), 0.5 * (cov + cov.transpose(0, 2, 1))
    g = MLPG(gmm, windows=WINDOWS, posterior="device")
    # speech-like label runs: every utterance is a chain of segments of 5 .. 30 frames, each drawn from one component of p(x)
    chol = np.linalg.cholesky(g.covarXX)
    utts = []
    for n in lens:
        seg = []
        while sum(seg) < n:
            seg.append(int(rng.randint(5, 31)))
        lab = np.repeat(rng.randint(M, size=len(seg)), seg)[:n]
        utts.append(g.src_means[lab] + np.einsum("nfg,ng->nf", chol[lab], rng.randn(n, D)))
    X = np.zeros((B, Tmax, D))
    for i, u in enumerate(utts):
        X[i, :len(u)] = u
    Xd, Ld = torch.from_numpy(X).to(dev), torch.from_numpy(lens).to(dev)
    return g, utts, X, lens, Xd, Ld, B, sd, M, D, Tmax, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    run(only=args.only, quick=args.quick)


def run(only="", quick=False, sink=None, device_index=0):
    """Run the selected paths (comma-separated keys, empty = all); with `sink` (a list) the result dicts are appended to
    it instead of being printed."""
    global _SINK
    _SINK = sink
    try:
        _run(only, quick, device_index)
    finally:
        _SINK = None


def _run(only, quick, device_index):
    class _A(object):
        pass
    args = _A()
    args.only, args.quick = only, quick
    import torch
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd import paramgen as G
    from nnmnkwii_amd.preprocessing.alignment import DTWAligner
    from oracle import dtw as OD
    from oracle import mlpg as O
    O.build()
    dev = torch.device("cuda", device_index)
    gen = torch.Generator(device=dev).manual_seed(1234)
    want = lambda k: not args.only or k in args.only.split(",")  # noqa: E731

    # ---- c2k: config 2 through every forward kernel (generic / wave-per-system / strip) ----
    if want("c2k"):
        B, T, sd = 256, 1000, 60
        m = torch.randn(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
        v = torch.rand(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen) + 0.1
        by = 56.0 * sd * B * T
        for name, algo in (("generic", 1), ("wave", 2), ("strip", 3)):
            ms = gpu_time(lambda: _hip.forward(m, v, WINDOWS, algo=algo, want_status=False), steps=20)
            emit(path="c2k-forward-" + name, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
        for name, algo in (("wave", 2), ("strip", 3)):
            go = torch.randn(B, T, sd, dtype=torch.float64, device=dev, generator=gen)
            ms = gpu_time(lambda: _hip.backward(v, go, WINDOWS, 3 * sd, out_dtype=torch.float64, algo=algo, want_status=False))
            byb = 8.0 * 7 * sd * B * T
            emit(path="c2k-backward-f64-" + name, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=byb, GBps=byb / ms / 1e6)
        # The same shape with variances as TTS acoustic models have them: the dynamic features 100 x / 1000 x tighter
        # than the static ones.  The trajectory is then smooth over hundreds of frames, the strip kernel's 5-strip
        # level-3 window is rejected by its damping bound and every strip sweeps the whole utterance.
        vt = v.clone()
        vt[:, :, sd:2 * sd] *= 1e-2
        vt[:, :, 2 * sd:] *= 1e-3
        for name, algo in (("wave", 2), ("strip", 3)):
            ms = gpu_time(lambda: _hip.forward(m, vt, WINDOWS, algo=algo, want_status=False), steps=20)
            emit(path="c2t-forward-tight-dynamic-variances-" + name, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
        vt = v.clone()                      # moderately tight (10 x / 100 x): the 9-strip window
        vt[:, :, sd:2 * sd] *= 1e-1
        vt[:, :, 2 * sd:] *= 1e-2
        ms = gpu_time(lambda: _hip.forward(m, vt, WINDOWS, algo=3, want_status=False), steps=20)
        emit(path="c2t-forward-moderately-tight-dynamic-variances-strip", ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
        del vt
        # delta_features (the step before MLPG): read sd, write 3 sd per frame
        x = torch.randn(B, T, sd, dtype=torch.float64, device=dev, generator=gen)
        ms = gpu_time(lambda: _hip.delta_features(x, WINDOWS))
        byd = 8.0 * 4 * sd * B * T
        emit(path="c2k-delta_features", ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=byd, GBps=byd / ms / 1e6)
        # long utterances (T = 4000: beyond the wave kernel): strip vs generic
        B2, T2 = 64, 4000
        m2 = torch.randn(B2, T2, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
        v2 = torch.rand(B2, T2, 3 * sd, dtype=torch.float64, device=dev, generator=gen) + 0.1
        by2 = 56.0 * sd * B2 * T2
        for name, algo in (("generic", 1), ("strip", 3)):
            ms = gpu_time(lambda: _hip.forward(m2, v2, WINDOWS, algo=algo, want_status=False), steps=5)
            emit(path="long-T4000-forward-" + name, ms=ms, frames_per_s=B2 * T2 / ms * 1e3, alg_bytes=by2, GBps=by2 / ms / 1e6)
        v2[:, :, sd:2 * sd] *= 1e-2          # the same with tight dynamic variances: windows of 8 / 16 strips per side
        v2[:, :, 2 * sd:] *= 1e-3
        ms = gpu_time(lambda: _hip.forward(m2, v2, WINDOWS, algo=3, want_status=False), steps=5)
        emit(path="long-T4000-forward-tight-dynamic-variances-strip", ms=ms, frames_per_s=B2 * T2 / ms * 1e3, alg_bytes=by2, GBps=by2 / ms / 1e6)
        del m, v, x, m2, v2

    # ---- c2t: the config-2 shape with TIGHT dynamic variances through AUTO (the strip kernel's slower level-3 rungs) ----
    # Variances as acoustic models have them: the dynamic features 10 x - 1000 x tighter than the static ones.  The trajectory is
    # then smooth over hundreds of frames; the strip kernel's 3-strip level-3 window is rejected by its damping bound and the
    # strips climb the ladder (5 / 9 / 33 strips, the whole utterance).  bench.py's metric data (variances ~ U(0.1, 1.1) in all
    # three windows) never leaves the 3-strip window: these entries put the other rungs into the driver's record.
    if want("c2t"):
        B, T, sd = 256, 1000, 60
        m = torch.randn(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
        v = torch.rand(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen) + 0.1
        by = 56.0 * sd * B * T
        for name, s1, s2 in (("10x-100x", 1e-1, 1e-2), ("100x-1000x", 1e-2, 1e-3)):
            vt = v.clone()
            vt[:, :, sd:2 * sd] *= s1
            vt[:, :, 2 * sd:] *= s2
            ms = gpu_time(lambda: _hip.forward(m, vt, WINDOWS, want_status=False), steps=20)
            y, st = _hip.forward(m, vt, WINDOWS)
            yo = O.mlpg(m[B - 1].cpu().numpy(), vt[B - 1].cpu().numpy(), WINDOWS)
            err = float(np.abs(y[B - 1].cpu().numpy() - yo).max() / np.abs(yo).max())
            emit(path="c2t-forward-dynamic-variances-tighter-" + name, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6,
                 status_max=int(st.abs().max().item()), rel_err_vs_oracle_last_utterance=err)
            del vt
        del m, v

    # ---- c2g: global / unit variances ----
    if want("c2g"):
        B, T, sd = 256, 1000, 60
        m = torch.randn(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
        vg = torch.rand(3 * sd, dtype=torch.float64, device=dev, generator=gen) + 0.1
        for name, var in (("global", vg), ("unit", None)):
            ms = gpu_time(lambda: _hip.forward(m, var, WINDOWS, want_status=False))
            by = 32.0 * sd * B * T
            emit(path="c2g-" + name, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
        # the same variances, backward (constant-coefficient kernel): read grad_out, write 3 gradient rows per (frame, dim)
        go = torch.randn(B, T, sd, dtype=torch.float64, device=dev, generator=gen)
        for name, var in (("global", vg), ("unit", None)):
            ms = gpu_time(lambda: _hip.backward(var, go, WINDOWS, 3 * sd, out_dtype=torch.float64, want_status=False))
            by = 32.0 * sd * B * T
            emit(path="c2g-" + name + "-backward", ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
        del m, go
        # config 5's mgc stream (T = 2000, 512 utterances = one GPU's share) with global variances
        B5, T5 = 512, 2000
        m5 = torch.randn(B5, T5, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
        ms = gpu_time(lambda: _hip.forward(m5, vg, WINDOWS, want_status=False))
        by = 32.0 * sd * B5 * T5
        emit(path="c5g-mgc-global-variances", ms=ms, frames_per_s=B5 * T5 / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
        del m5
        # the reference's 5-tap test windows (tests/test_paramgen.py:21-26: P has half-bandwidth 4), config-2 shape, per-frame
        # variances: the chunked kernel (AUTO) and the natural-order kernel
        wide = [(0, 0, np.array([1.0])), (2, 2, np.array([1.0, -8.0, 0.0, 8.0, -1.0]) / 12.0),
                (2, 2, np.array([-1.0, 16.0, -30.0, 16.0, -1.0]) / 12.0)]
        mw_ = torch.randn(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
        vw_ = torch.rand(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen) + 0.1
        byw = 56.0 * sd * B * T
        for name, algo in (("", 0), ("-natural-order-kernel", 1)):
            ms = gpu_time(lambda: _hip.forward(mw_, vw_, wide, algo=algo, want_status=False), steps=5 if algo else 10)
            emit(path="c2w-forward-5-tap-windows" + name, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=byw, GBps=byw / ms / 1e6)
        del mw_, vw_
        # long utterances, per-frame variances (T = 4000: 63 strips per utterance, dealt to the XCD work lists in two blocks)
        B2, T2 = 64, 4000
        m2 = torch.randn(B2, T2, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
        v2 = torch.rand(B2, T2, 3 * sd, dtype=torch.float64, device=dev, generator=gen) + 0.1
        ms = gpu_time(lambda: _hip.forward(m2, v2, WINDOWS, want_status=False), steps=5)
        by2 = 56.0 * sd * B2 * T2
        emit(path="long-T4000-forward", ms=ms, frames_per_s=B2 * T2 / ms * 1e3, alg_bytes=by2, GBps=by2 / ms / 1e6)
        del m2, v2

    # ---- c2h: config 2 end to end from host memory (numpy in -> numpy out through paramgen.mlpg_batch): PCIe-inclusive ----
    if want("c2h"):
        B, T, sd = 256, 1000, 60
        rng = np.random.RandomState(1234)
        mh = rng.randn(B, T, 3 * sd)
        vh = rng.rand(B, T, 3 * sd) + 0.1
        G.mlpg_batch(mh, vh, WINDOWS)          # full-size warm-up: the library's staging buffers grow on first use
        by = 56.0 * sd * B * T

        def host_walls(m_, v_, nrep=6):
            """Wall clock per call, every call into FRESH output pages (the arrays are kept alive, so that neither a reused
            mapping nor the munmap of the previous 123 MB result falls into the timed region: round 4's entry timed
            `y = mlpg_batch(...)` in a loop, i.e. each call plus the release of the previous result -- 20.5 ms against the
            16.1 ms tools/dbg/host_path_time.py measured for the same call)."""
            keep, ts, ts_free = [], [], []
            for _ in range(nrep):
                t0 = time.perf_counter()
                keep.append(G.mlpg_batch(m_, v_, WINDOWS))
                ts.append(time.perf_counter() - t0)
            yprev = keep.pop()
            for _ in range(3):                 # the round-4 form: the previous result is released inside the timed region
                t0 = time.perf_counter()
                yprev = G.mlpg_batch(m_, v_, WINDOWS)
                ts_free.append(time.perf_counter() - t0)
            del keep, yprev
            return float(np.median(ts)), float(np.min(ts)), float(np.mean(ts_free))

        wall, wmin, wfree = host_walls(mh, vh)
        emit(path="c2h-numpy-to-numpy-mlpg_batch", ms=wall * 1e3, ms_min=wmin * 1e3, ms_with_release_of_previous_result=wfree * 1e3,
             frames_per_s=B * T / wall, alg_bytes=by,
             GBps=by / wall / 1e9, note="pageable host arrays through mlpg_hip_forward_host: chunked, staged by copy threads, transfers overlapped with the kernels; median of 6 calls into fresh output pages")
        # the same from pinned host arrays (nnmnkwii_amd._hip.pinned_empty): transferred in place, no staging copies
        mp, vp = _hip.pinned_empty(mh.shape), _hip.pinned_empty(vh.shape)
        mp[...] = mh
        vp[...] = vh
        G.mlpg_batch(mp, vp, WINDOWS)
        wall, wmin, wfree = host_walls(mp, vp)
        emit(path="c2h-numpy-to-numpy-mlpg_batch-pinned-inputs", ms=wall * 1e3, ms_min=wmin * 1e3, ms_with_release_of_previous_result=wfree * 1e3,
             frames_per_s=B * T / wall, alg_bytes=by,
             GBps=by / wall / 1e9, note="pinned inputs, pageable output: PCIe floor 12.9 ms (737 MB up at 57 GB/s, the 123 MB down overlapped); median of 6 calls into fresh output pages")
        yh = None
        del mh, vh, yh, mp, vp

    # ---- lit: the LITERAL drop-in calls -- one numpy -> numpy call per utterance, as a user of the reference writes them ----
    if want("lit") or want("litq"):
        literal_calls(emit, quick=args.quick, long_reference_backward=want("lit"))

    # ---- c2b: backward (mlpg_hip_backward) at config-2 scale, float64 and float32 ----
    if want("c2b"):
        B, T, sd = 256, 1000, 60
        for name, dt, esz in (("f64", torch.float64, 8), ("f32", torch.float32, 4)):
            v = torch.rand(B, T, 3 * sd, dtype=dt, device=dev, generator=gen) + 0.1
            go = torch.randn(B, T, sd, dtype=dt, device=dev, generator=gen)
            ms = gpu_time(lambda: _hip.backward(v, go, WINDOWS, 3 * sd, out_dtype=dt, want_status=False))
            by = float(esz) * (3 + 1 + 3) * sd * B * T     # read 3 variances + grad_out, write 3 grads per (frame, dim)
            emit(path="c2b-backward-" + name, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
            del v, go
        m32 = torch.randn(B, T, 3 * sd, dtype=torch.float32, device=dev, generator=gen)
        v32 = torch.rand(B, T, 3 * sd, dtype=torch.float32, device=dev, generator=gen) + 0.1
        ms = gpu_time(lambda: _hip.forward(m32, v32, WINDOWS, want_status=False))
        by = 4.0 * 7 * sd * B * T
        emit(path="c2-forward-f32", ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
        del m32, v32

    # ---- c2v: gradients w.r.t. the variances (mlpg_hip_backward_var) at config-2 scale; only with --only c2v ----
    if args.only and "c2v" in args.only.split(","):
        B, T, sd = 256, 1000, 60
        for name, dt, esz in (("f64", torch.float64, 8), ("f32", torch.float32, 4)):
            m = torch.randn(B, T, 3 * sd, dtype=dt, device=dev, generator=gen)
            v = torch.rand(B, T, 3 * sd, dtype=dt, device=dev, generator=gen) + 0.1
            go = torch.randn(B, T, sd, dtype=dt, device=dev, generator=gen)
            y, _ = _hip.forward(m, v, WINDOWS, want_status=False)
            ms_b = gpu_time(lambda: _hip.backward(v, go, WINDOWS, 3 * sd, out_dtype=dt), steps=20)
            ms_v = gpu_time(lambda: _hip.backward_var(m, v, y, go, WINDOWS), steps=20)
            by_b = float(esz) * (3 + 1 + 3) * sd * B * T
            by_k = float(esz) * (4 * 3 + 1) * sd * B * T     # the new kernel: read 3 x (grad_mean, var, mean) + y, write 3 grad_var
            share = ms_v - ms_b
            emit(path="c2v-backward-" + name, ms=ms_b, alg_bytes=by_b, GBps=by_b / ms_b / 1e6)
            emit(path="c2v-backward_var-" + name, ms=ms_v, alg_bytes=by_b + by_k, GBps=(by_b + by_k) / ms_v / 1e6)
            emit(path="c2v-var-grad-kernel-share-" + name, ms=share, alg_bytes=by_k, GBps=by_k / share / 1e6 if share > 0 else None,
                 note="HIP-event time of backward_var minus backward alone; rocprofv3 --kernel-trace gives the kernel's own duration")
            mq = m.clone().requires_grad_()
            vq = v.clone().requires_grad_()

            def step():
                mq.grad = None
                vq.grad = None
                (AF.mlpg_batch(mq, vq, WINDOWS) * go).sum().backward()

            ms_s = gpu_time(step, steps=10)
            emit(path="c2v-mlpg_batch-step-" + name, ms=ms_s, frames_per_s=B * T / ms_s * 1e3,
                 note="autograd.mlpg_batch forward + backward, requires_grad on means and variances, CHECK_STATUS on")
            del m, v, go, y, mq, vq

    # ---- msb: forward + backward of the log-MS loss over a padded config-2 sized minibatch; only with --only msb ----
    if args.only and "msb" in args.only.split(","):
        B, T, D, eps = 256, 1000, 60, 1e-10
        lengths = np.random.RandomState(1234).randint(600, 1001, size=B)
        L = torch.from_numpy(lengths.astype(np.int32)).to(dev)
        live = (torch.arange(T, device=dev)[None, :, None] < L[:, None, None])
        for name, dt, esz in (("f32", torch.float32, 4), ("f64", torch.float64, 8)):
            for n in (2048, 4096):
                nb = n // 2 + 1
                traj = lambda: (0.1 * torch.cumsum(torch.randn(B, T, D, dtype=torch.float64, device=dev, generator=gen), dim=1) +  # noqa: E731
                                torch.rand(B, T, D, dtype=torch.float64, device=dev, generator=gen)).to(dt) * live
                y = traj().requires_grad_()
                tm = AF.modspec_batch(traj(), n=n, lengths=L).detach()
                n_elems = float(B * nb * D)

                def loop():             # (a) what the 2-D node allows: one utterance at a time, torch ops for the loss
                    y.grad = None
                    total = 0.0
                    for b in range(B):
                        ms = AF.modspec(y[b, :lengths[b]], n=n)
                        total = total + ((torch.log(ms + eps) - torch.log(tm[b] + eps)) ** 2).sum()
                    (total / n_elems).backward()

                def composed():         # (b) modspec_batch + torch ops
                    y.grad = None
                    ms = AF.modspec_batch(y, n=n, lengths=L)
                    ((torch.log(ms + eps) - torch.log(tm + eps)) ** 2).mean().backward()

                def fused():            # (c) the fused step
                    y.grad = None
                    AF.modspec_mse_loss(y, tm, n=n, lengths=L, eps=eps).backward()

                by = float(esz) * B * D * (2 * T + nb)      # (c): y read, target_ms read, grad_x written
                tag = "%s-n%d" % (name, n)
                ms_a = gpu_time(loop, steps=3, warmup=1, settle_ms=0)
                emit(path="msb-loop-2d-node-" + tag, ms=ms_a, note="(a) Python loop of autograd.modspec over %d utterances + torch ops" % B)
                ms_b = gpu_time(composed, steps=10)
                emit(path="msb-modspec_batch-torch-" + tag, ms=ms_b, note="(b) autograd.modspec_batch + torch ops for the loss")
                ms_c = gpu_time(fused, steps=20)
                emit(path="msb-fused-" + tag, ms=ms_c, alg_bytes=by, GBps=by / ms_c / 1e6, form=_hip.modspec_loss_form(n),
                     note="(c) autograd.modspec_mse_loss, forward + backward")
                del y, tm

    # ---- c5b: multi-stream MLPG forward + backward at config-5 scale, gradients in place; only with --only c5b ----
    if args.only and "c5b" in args.only.split(","):
        B, T = 512, 2000
        sizes, dyn = [180, 3, 15], [True, True, True]                 # mgc 60 | lf0 1 | bap 5, three windows each: 198 columns
        D, nsd = sum(sizes), sum(sizes) // 3
        bounds = np.cumsum([0] + sizes).tolist()
        streams = [(bounds[k], sizes[k] // 3, WINDOWS) for k in range(3)]
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import streamgrad64
        for name, dt, esz in (("f64", torch.float64, 8), ("f32", torch.float32, 4)):
            m = torch.randn(B, T, D, dtype=dt, device=dev, generator=gen)
            vf = torch.rand(B, T, D, dtype=dt, device=dev, generator=gen) + 0.1
            go = torch.randn(B, T, nsd, dtype=dt, device=dev, generator=gen)
            for vname, v in (("frame", vf), ("global", vf[0, 0].clone())):
                mq, vq = m.clone().requires_grad_(), v.clone().requires_grad_()

                def step_inplace():
                    mq.grad = None
                    vq.grad = None
                    AF.multi_stream_mlpg(mq, vq, WINDOWS, sizes, dyn).backward(go)

                def step_composed():          # what a user writes without the in-place call: slices, one mlpg_batch per stream, cat
                    mq.grad = None
                    vq.grad = None
                    ys = [AF.mlpg_batch(mq[:, :, a:b].contiguous(), vq[..., a:b].contiguous(), WINDOWS)
                          for a, b in zip(bounds[:-1], bounds[1:])]
                    torch.cat(ys, dim=2).backward(go)

                tag = "%s-%s" % (vname, name)
                by = float(esz) * B * T * (7 * nsd + 7 * nsd + 13 * nsd)   # forward solve, backward solve, variance-gradient epilogue
                have = hasattr(AF, "multi_stream_mlpg")
                for label, fn in (("inplace", step_inplace), ("composed", step_composed)):
                    if label == "inplace" and not have:
                        continue
                    takes = [gpu_time(fn, steps=5) for _ in range(5)]
                    emit(path="c5b-step-%s-%s" % (label, tag), ms=float(np.median(takes)), ms_min=min(takes), ms_max=max(takes),
                         takes_ms=takes, frames_per_s=B * T / float(np.median(takes)) * 1e3, alg_bytes=by,
                         GBps=by / float(np.median(takes)) / 1e6,
                         note="forward + backward, requires_grad on means and variances, CHECK_STATUS on; 5 takes of the median of 5 steps")
                if not have:
                    continue
                # the epilogue kernel's share: backward_streams with and without the variance gradient (HIP events)
                md, vd = mq.detach(), vq.detach()
                y, _ = _hip.forward_streams(md, vd, streams, want_status=False)
                sh = []
                for _ in range(5):
                    ms_v = gpu_time(lambda: _hip.backward_streams(md, vd, y, go, streams), steps=5)
                    ms_m = gpu_time(lambda: _hip.backward_streams(md, vd, y, go, streams, want_var=False), steps=5)
                    sh.append(ms_v - ms_m)
                by_k = float(esz) * B * T * 13 * nsd     # read 3 x (grad_mean, var, mean) + y, write 3 grad_var per (frame, dim)
                share = float(np.median(sh))
                emit(path="c5b-epilogue-kernel-share-" + tag, ms=share, ms_min=min(sh), ms_max=max(sh), takes_ms=sh, alg_bytes=by_k,
                     GBps=by_k / share / 1e6 if share > 0 else None,
                     note="HIP-event time of backward_streams with grad_var minus without: one launch for the three streams")
                # spot check: the gradients of two utterances against the float64 reference (tests/streamgrad64.py)
                step_inplace()
                torch.cuda.synchronize()
                sel = [0, B - 1]
                sdicts = [dict(in_col=c, out_col=c // 3, static_dim=sd, windows=w) for c, sd, w in streams]
                v_np = vd.cpu().numpy() if vd.dim() == 1 else vd[sel].cpu().numpy()
                _, gm_ref, gv_ref = streamgrad64.multi_stream_grad64(md[sel].cpu().numpy(), v_np, go[sel].cpu().numpy(), sdicts)
                gm_got = mq.grad[sel].double().cpu().numpy()
                tol = 1e-10 if dt == torch.float64 else 3e-6
                e_m = float(np.abs(gm_got - gm_ref).max() / np.abs(gm_ref).max())
                if vd.dim() == 1:
                    # (the sum runs over all 512 utterances on the GPU: compare the two utterances' own contributions instead)
                    _, gv2, _ = _hip.backward_streams(md[sel].contiguous(), vd, y[sel].contiguous(), go[sel].contiguous(), streams)
                    gv_got = gv2.double().cpu().numpy()
                else:
                    gv_got = vq.grad[sel].double().cpu().numpy()
                e_v = float(np.abs(gv_got - gv_ref).max() / np.abs(gv_ref).max())
                emit(path="c5b-spot-check-" + tag, grad_mean_rel_err=e_m, grad_var_rel_err=e_v, tol=tol, ok=bool(e_m <= tol and e_v <= tol),
                     note="utterances 0 and 511 against the float64 reference, error over the largest gradient entry")
                assert e_m <= tol and e_v <= tol, ("c5b spot check", tag, e_m, e_v)
                del mq, vq, md, vd, y
            del m, vf, go

    def config4_joint():
        """The joint matrix one IterativeDTWAligner iteration fits at config 4 (zero padding rows included, as the aligner fits it)."""
        N, D = (16 if args.quick else 128), 25
        rng = np.random.RandomState(1234)
        X = np.zeros((N, 900, D))
        Y = np.zeros((N, 900, D))
        for n in range(N):
            a, b = rng.randint(700, 901, size=2)
            X[n, :a] = np.cumsum(rng.randn(a, D), 0) * 0.1
            Y[n, :b] = np.cumsum(rng.randn(b, D), 0) * 0.1
        Xa, Ya = DTWAligner().transform((X, Y))
        return np.concatenate((Xa, Ya), axis=-1).reshape(-1, 2 * D)

    # ---- gmm: the joint-GMM fit of one IterativeDTWAligner iteration at config 4, host and device; only with --only gmm ----
    if args.only and "gmm" in args.only.split(","):
        import warnings
        from sklearn.mixture import GaussianMixture
        from nnmnkwii_amd.mixture import fit_gaussian_mixture
        K = 16
        joint = config4_joint()
        rows, F = joint.shape
        t0 = time.perf_counter()
        g0 = GaussianMixture(n_components=K, covariance_type="full", max_iter=0, random_state=0).fit(joint)
        init_s = time.perf_counter() - t0
        init = (g0.weights_, g0.means_, g0.covariances_)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fit_gaussian_mixture(joint, K, max_iter=2, init=init)            # warm-up: code objects, allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gd = fit_gaussian_mixture(joint, K, max_iter=100, init=init)
            dev_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            gs = GaussianMixture(n_components=K, covariance_type="full", max_iter=100, weights_init=init[0], means_init=init[1],
                                 precisions_init=g0.precisions_).fit(joint)
            host_s = time.perf_counter() - t0
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
        xd, w, mu, cov = f64(joint), f64(gd.weights_), f64(gd.means_), f64(gd.covariances_)
        ws = _hip.gmm_workspace(dev, rows, F, K)
        U, log_det, _ = _hip.gmm_precisions(cov)
        resp = _hip.gmm_estep(xd, w, mu, U, log_det, want_mean=True, workspace=ws)[0]
        ms_e = gpu_time(lambda: _hip.gmm_estep(xd, w, mu, U, log_det, want_mean=True, workspace=ws), steps=20)
        ms_m = gpu_time(lambda: _hip.gmm_mstep(xd, resp, 1e-6, workspace=ws), steps=20)
        ms_p = gpu_time(lambda: _hip.gmm_precisions(cov), steps=20)
        rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
        res = dict(path="gmm-fit-config4", rows=int(rows), F=int(F), K=K, max_iter=100, tol=1e-3, host_threads=os.environ.get("OMP_NUM_THREADS"),
                   sklearn_init_s=init_s, sklearn_fit_s=host_s, sklearn_iters=int(gs.n_iter_), sklearn_converged=bool(gs.converged_),
                   sklearn_s_per_iter=host_s / max(int(gs.n_iter_), 1),
                   device_fit_s=dev_s, device_iters=int(gd.n_iter_), device_converged=bool(gd.converged_),
                   device_s_per_iter=dev_s / max(int(gd.n_iter_), 1), estep_ms=ms_e, mstep_ms=ms_m, precisions_ms=ms_p,
                   fit_speedup=host_s / dev_s, means_rel_diff=rel(gd.means_, gs.means_),
                   lower_bound_device=float(gd.lower_bound_), lower_bound_sklearn=float(gs.lower_bound_),
                   flops_per_iter=float(rows) * K * F * F * 2 * 2,
                   note="one aligner iteration's fit, both from the same max_iter=0 start; device_fit_s includes the host-to-device copy "
                        "of the joint matrix and the per-iteration read-back; kernel times are HIP-event medians on settled clocks")
        emit(**res)
        out = os.environ.get("NNMNKWII_GMM_PROFILE") or os.path.join(ROOT, "profiles", "gmm_em.json")
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")

    # ---- kmeans: the start of that fit (k-means, then one M-step), host and device, same data and seed; only with --only kmeans ----
    if args.only and "kmeans" in args.only.split(","):
        import warnings
        from sklearn.cluster import KMeans
        from sklearn.mixture import GaussianMixture
        from sklearn.utils import check_random_state
        from nnmnkwii_amd import mixture
        K, seed = 16, 0
        joint = config4_joint()
        rows, F = joint.shape
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            g0 = GaussianMixture(n_components=K, covariance_type="full", max_iter=0, random_state=seed).fit(joint)
            host_s = time.perf_counter() - t0
            km = KMeans(n_clusters=K, n_init=1, random_state=check_random_state(seed)).fit(joint)   # the same draws: its n_iter_
            mixture.fit_gaussian_mixture(joint, K, init="kmeans", max_iter=0, random_state=seed)   # warm-up: code objects, allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gd = mixture.fit_gaussian_mixture(joint, K, init="kmeans", max_iter=0, random_state=seed)
            dev_s = time.perf_counter() - t0
        xd = torch.from_numpy(joint).to(dev)
        t0 = time.perf_counter()
        labels, centers, inertia, n_iter = mixture.kmeans(xd, K, random_state=seed)
        torch.cuda.synchronize()
        resident_s = time.perf_counter() - t0
        shift = xd.mean(dim=0).contiguous()
        ws = _hip.kmeans_workspace(dev, rows, F, K)
        cand = torch.arange(0, 5 * 1000, 1000, dtype=torch.int32, device=dev) % rows      # 2 + int(log 16) = 4 trials; 5 is no faster case
        closest = _hip.kmeans_seed_step(xd, shift, cand[:1], None, workspace=ws)[0][0].contiguous()
        ms_seed = gpu_time(lambda: _hip.kmeans_seed_step(xd, shift, cand[:4], closest, workspace=ws), steps=20)
        cen = (centers - shift).contiguous()
        ms_lloyd = gpu_time(lambda: _hip.kmeans_lloyd_step(xd, shift, cen, labels, workspace=ws), steps=20)
        rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
        res = dict(path="kmeans-start-config4", rows=int(rows), F=int(F), K=K, seed=seed, host_threads=os.environ.get("OMP_NUM_THREADS"),
                   sklearn_start_s=host_s, device_start_s=dev_s, start_speedup=host_s / dev_s, device_kmeans_resident_s=resident_s,
                   sklearn_lloyd_iters=int(km.n_iter_), device_lloyd_iters=int(n_iter),
                   labels_equal=bool(np.array_equal(labels.cpu().numpy(), km.labels_)), seed_step_ms=ms_seed, lloyd_step_ms=ms_lloyd,
                   lloyd_step_gb_s=rows * F * 8 / (ms_lloyd * 1e6), means_rel_diff=rel(gd.means_, g0.means_),
                   covariances_rel_diff=rel(gd.covariances_, g0.covariances_),
                   note="GaussianMixture(max_iter=0).fit on the host against fit_gaussian_mixture(init='kmeans', max_iter=0) from numpy "
                        "input (device_start_s includes the host-to-device copy of the joint matrix and every read-back); "
                        "device_kmeans_resident_s: mixture.kmeans on the matrix already on the device; kernel times are HIP-event "
                        "medians on settled clocks, the seed step with 4 candidates")
        emit(**res)
        out = os.environ.get("NNMNKWII_KMEANS_PROFILE") or os.path.join(ROOT, "profiles", "kmeans.json")
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")

    # ---- postfilter: the Merlin post-filter behind multi-stream MLPG at config-5 scale; only with --only postfilter ----
    if args.only and "postfilter" in args.only.split(","):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import postfilter_model as PM
        from nnmnkwii_amd import postfilters as PF
        B, T, D, alpha, order, fftlen = (64, 500, 60, 0.58, 511, 1024) if args.quick else (512, 2000, 60, 0.58, 511, 1024)
        rng = np.random.RandomState(1234)
        lens = rng.randint(int(0.6 * T), T + 1, size=B).astype(np.int32)
        frames = int(lens.sum())
        flops = float(frames) * 2 * (fftlen // 2 + 1) * D * 2
        lengths = torch.from_numpy(lens).to(dev)
        t0 = time.perf_counter()
        G = _hip.postfilter_table_host(D, alpha, order, fftlen)
        table_ms = (time.perf_counter() - t0) * 1e3
        res = dict(path="postfilter-config5", B=B, T=T, D=D, alpha=alpha, minimum_phase_order=order, fftlen=fftlen, frames=frames,
                   flops=flops, f64_matrix_peak_tflops=F64_MATRIX_PEAK_TFLOPS, table_build_host_ms=table_ms,
                   table_bytes=int(G.nbytes), frame_tile=_hip.POSTFILTER_FRAME_TILE)
        host = (rng.randn(B, T, D) / (1.0 + np.arange(D)))
        host[:, :, 0] += rng.uniform(-8.0, 2.0, (B, T))
        for name, tdt in (("float64", torch.float64), ("float32", torch.float32)):
            x = torch.from_numpy(host).to(dev).to(tdt)
            out = torch.empty_like(x)
            ms = gpu_time(lambda: PF.merlin_post_filter_batch(x, alpha, order, fftlen, lengths=lengths, out=out), steps=20)
            res["%s_ms" % name] = ms
            res["%s_tflops" % name] = flops / (ms * 1e9)
            res["%s_peak_frac" % name] = flops / (ms * 1e9) / F64_MATRIX_PEAK_TFLOPS
            res["%s_us_per_frame" % name] = ms * 1e3 / frames
            pick = np.arange(0, min(int(lens[0]), 200), 37)
            ref = PM.post_filter_literal(x[0, pick].cpu().numpy().astype(np.float64), alpha, order, fftlen)
            res["%s_rel_err" % name] = float(np.abs(out[0, pick].cpu().numpy() - ref).max() / np.abs(ref).max())
        nf = 64
        t0 = time.perf_counter()
        PM.post_filter_literal(host[0, :nf], alpha, order, fftlen)
        res["numpy_model_s_per_frame"] = (time.perf_counter() - t0) / nf
        res["note"] = ("one launch over the padded batch, lengths in [0.6 T, T]; flops = valid frames * 2 products * (fftlen/2 + 1) bins * D "
                       "* 2 (padding frames and the exponentials not counted); the peak is AMD's published float64 matrix rate for the "
                       "MI355X; HIP-event medians on settled clocks; the numpy model (%d frames at once, literal recursion) is context, "
                       "not a baseline: the parent commit has no device path and pysptk is not installed here" % nf)
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_POSTFILTER_PROFILE") or os.path.join(ROOT, "profiles", "postfilter.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- msfilter: the MS post-filter and smoothing on the mgc columns of a config-5 sized batch; only with --only msfilter ----
    if args.only and "msfilter" in args.only.split(","):
        from nnmnkwii_amd import postfilters as PF
        import importlib
        MS = importlib.import_module("nnmnkwii_amd.preprocessing.modspec")   # (by name: the package re-exports a function `modspec`)
        B, T, D, ld, n, modfs, cutoff = (32, 500, 60, 187, 4096, 200, 50) if args.quick else (512, 2000, 60, 187, 4096, 200, 50)
        nb = n // 2 + 1
        rng = np.random.RandomState(1234)
        lens = rng.randint(int(0.6 * T), T + 1, size=B).astype(np.int32)
        lengths = torch.from_numpy(lens).to(dev)
        live = lengths.to(torch.int64)
        limit_bin = MS.limit_bin_of(n, modfs, cutoff)
        A = torch.from_numpy(rng.uniform(0.8, 1.3, (nb, D))).to(dev)
        C = torch.from_numpy(rng.uniform(-0.5, 0.5, (nb, D))).to(dev)
        res = dict(path="msfilter-config5", B=B, T=T, D=D, row_stride=ld, n=n, modfs=modfs, cutoff=cutoff, limit_bin=limit_bin,
                   frames=int(lens.sum()), table_bytes=int(2 * nb * D * 8), hbm_peak_GBps=HBM_PEAK_GBS)
        for name, tdt, item in (("float32", torch.float32, 4), ("float64", torch.float64, 8)):
            wide = (0.1 * torch.cumsum(torch.randn(B, T, ld, dtype=torch.float64, device=dev, generator=gen), dim=1)).to(tdt)
            dst = torch.zeros_like(wide)
            x, out = wide[..., :D], dst[..., :D]
            c0 = _hip.lib().mlpg_hip_launch_count(31)
            ms_a = gpu_time(lambda: PF.modspec_post_filter_batch(x, A, C, n=n, lengths=lengths, modfs=modfs, cutoff=cutoff, out=out),
                            steps=20)
            assert _hip.lib().mlpg_hip_launch_count(31) > c0
            ya = out.to(torch.float64)

            def composed():
                out.copy_(MS._composed_filter(x, live, n, False, A, C, limit_bin, True))

            ms_b = gpu_time(composed, steps=5, warmup=1, settle_ms=0)
            yb = out.to(torch.float64)
            nbytes = 2.0 * B * T * D * item
            floor_ms = nbytes / (HBM_PEAK_GBS * 1e9) * 1e3
            res.update({"%s_launch_ms" % name: ms_a, "%s_composed_ms" % name: ms_b, "%s_composed_over_launch" % name: ms_b / ms_a,
                        "%s_bytes" % name: nbytes, "%s_hbm_floor_ms" % name: floor_ms, "%s_hbm_floor_frac" % name: floor_ms / ms_a,
                        "%s_us_per_column" % name: ms_a * 1e3 / (B * D),
                        "%s_launch_vs_composed_rel" % name: float((ya - yb).abs().max() / yb.abs().max())})
            del wide, dst, x, out, ya, yb
            torch.cuda.empty_cache()
        res["note"] = ("(a) one launch of mlpg_hip_modspec_filter on the column slice, in the stored dtype; (b) the same filter from entry "
                       "points the parent commit has: a masked float64 copy, mlpg_hip_modspec with phase, torch arithmetic on the "
                       "(B, n/2+1, D) spectra, mlpg_hip_inv_modspec, mask, cast and copy into the slice.  Bytes: x read plus result "
                       "written over the padded batch; the floor is those bytes at the 8 TB/s HBM peak.  HIP-event medians; (a) on "
                       "settled clocks over 20 calls, (b) over 5 calls.  Neither time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_MSFILTER_PROFILE") or os.path.join(ROOT, "profiles", "msfilter.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- vc: trajectory GMM voice conversion of a corpus, per utterance and batched; only with --only vc ----
    if args.only and "vc" in args.only.split(","):
        g, utts, X, lens, Xd, Ld, B, sd, M, D, Tmax, frames = vc_corpus(args.quick, dev)
        res = dict(path="gmm-vc-corpus", B=B, Tmax=Tmax, D=D, static_dim=sd, M=M, frames=frames, padded_rows=B * Tmax, posterior="device",
                   row_tile=_hip.GMM_TRAJ_ROW_TILE, hbm_peak_GBps=HBM_PEAK_GBS)
        # (a) the parent route: one MLPG.transform per utterance (every length is a shape of its own: the first loop warms them all)
        ref = [g.transform(u) for u in utts]
        res["a_transform_loop"] = spread(events(lambda: [g.transform(u) for u in utts], 3))
        # (b) transform_batch on the same list
        got = g.transform_batch(utts)
        res["b_vs_a_rel_err"] = float(max(np.abs(y - r).max() for y, r in zip(got, ref)) / max(np.abs(r).max() for r in ref))
        g.transform_batch(utts)
        res["b_transform_batch"] = spread(events(lambda: g.transform_batch(utts), 5))
        # (c) transform_padded on a resident tensor, and its three launches one by one
        from nnmnkwii_amd.paramgen import mlpg_batch as _mlpg_batch
        mu_x, mu_y, A, cvar, px = g._device_model(dev)[:5]
        x2 = Xd.view(B * Tmax, D)
        for _ in range(3):
            g.transform_padded(Xd, Ld)
        res["c_transform_padded"] = spread(events(lambda: g.transform_padded(Xd, Ld), 20))
        labels = _hip.gmm_estep(x2, *px, want_resp=False, want_labels=True)[2]
        mean, var = _hip.gmm_trajectory_stats(Xd, Ld, labels, mu_x, mu_y, A, cvar)
        estep = lambda: _hip.gmm_estep(x2, *px, want_resp=False, want_labels=True)  # noqa: E731
        stats = lambda: _hip.gmm_trajectory_stats(Xd, Ld, labels, mu_x, mu_y, A, cvar, mean=mean, var=var)  # noqa: E731
        traj = lambda: _mlpg_batch(mean, var, WINDOWS, Ld)  # noqa: E731
        for name, fn in (("c_estep", estep), ("c_stats", stats), ("c_mlpg", traj)):
            for _ in range(3):
                fn()
            res[name] = spread(events(fn, 20))
        # (d) the stats kernel against the composition it replaces, alternating in one run
        lab64 = labels.to(torch.int64)

        def composed():
            e = _hip.gmm_convert(x2, None, labels, mu_x, mu_y, A)
            return e, cvar[lab64]

        e, v = composed()
        live = (torch.arange(Tmax, device=dev)[None, :] < Ld[:, None]).view(-1)
        res["d_new_vs_composed_rel"] = float(((mean.view(-1, D) - e)[live].abs().max() / e[live].abs().max()).item())
        assert torch.equal(var.view(-1, D)[live], v[live])
        for _ in range(20):     # settle the clocks on both
            stats()
            composed()
        t_new, t_old = [], []
        for _ in range(24):
            t_new += events(stats, 1)
            t_old += events(composed, 1)
        res["d_stats_kernel"], res["d_composed"] = spread(t_new), spread(t_old)
        res["d_composed_over_new"] = res["d_composed"]["median_ms"] / res["d_stats_kernel"]["median_ms"]
        nbytes = float(frames) * (8 * D + 16 * D + 4)
        res["stats_bytes"] = nbytes
        res["stats_GBps"] = nbytes / (res["d_stats_kernel"]["median_ms"] * 1e6)
        res["stats_hbm_peak_frac"] = res["stats_GBps"] / HBM_PEAK_GBS
        lab_h = labels.view(B * Tmax).cpu().numpy()
        live_h = live.cpu().numpy()
        tiles = [np.unique(lab_h[i:i + 64][live_h[i:i + 64]]).size for i in range(0, B * Tmax, 64)]
        res["distinct_labels_per_tile_mean"] = float(np.mean(tiles))
        res["distinct_labels_per_tile_max"] = int(np.max(tiles))
        res["note"] = ("synthetic corpus: a joint model of M separated components built directly, every utterance a chain of 5-30 frame "
                       "segments drawn from one component each.  HIP-event times around (a) the loop of MLPG.transform over the list "
                       "(numpy in and out, 3 loops), (b) MLPG.transform_batch on the list (5 calls), (c) transform_padded on a resident "
                       "tensor (20 calls) and its three launches alone, (d) mlpg_hip_gmm_trajectory_stats against gmm_convert(mixture=labels) "
                       "plus cvar[labels] by torch over all padded rows, 24 alternating pairs.  Bytes: live rows * (8 D read + 16 D written "
                       "+ 4 label); A, mu and cvar are not counted.  No time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_GMM_VC_PROFILE") or os.path.join(ROOT, "profiles", "gmm_vc.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- gv: the ascent on the likelihood with the gv term, one launch against the iteration composed from torch operations ----
    if args.only and "gv" in args.only.split(","):
        from nnmnkwii_amd.paramgen import mlpg_batch as _mlpg_batch
        g, utts, X, lens, Xd, Ld, B, sd, M, D, Tmax, frames = vc_corpus(args.quick, dev)
        n_iter = 100
        mu_x, mu_y, A, cvar, px = g._device_model(dev)[:5]
        labels = _hip.gmm_estep(Xd.view(B * Tmax, D), *px, want_resp=False, want_labels=True)[2]
        mean, var = _hip.gmm_trajectory_stats(Xd, Ld, labels, mu_x, mu_y, A, cvar)
        y0 = _mlpg_batch(mean, var, WINDOWS, Ld)
        gv0 = _hip.gv(y0, Ld)
        gv_mean = 1.8 * gv0.mean(dim=0)                 # statistics above the gv of the over-smoothed trajectories
        gv_prec = 1.0 / (0.2 * gv_mean) ** 2
        # the composed route's tables, built once outside the timed region: the band columns of P and r by shifted slices
        Tf = Ld.to(torch.float64)[:, None, None]
        tt = torch.arange(Tmax, device=dev)[None, :, None]
        live = (tt < Ld[:, None, None]).to(torch.float64)

        def shift(x, o):                                 # shift(x, o)[f] = x[f - o], 0 outside
            z = torch.zeros_like(x)
            if o == 0:
                z.copy_(x)
            elif o > 0:
                z[:, o:] = x[:, :-o]
            else:
                z[:, :o] = x[:, -o:]
            return z

        pk = [torch.zeros((B, Tmax, sd), dtype=torch.float64, device=dev) for _ in range(3)]
        r = torch.zeros((B, Tmax, sd), dtype=torch.float64, device=dev)
        for w, (l, u, c) in enumerate(WINDOWS):
            tau = live / var[:, :, w * sd:(w + 1) * sd]
            if w:
                tau = tau * ((tt >= 1) & (tt < Ld[:, None, None] - 1)).to(torch.float64)
            mu = mean[:, :, w * sd:(w + 1) * sd]
            for o in range(u, -l - 1, -1):
                a = float(c[l + o]) * shift(tau, o)
                r += a * shift(mu, o)
                for k in range(3):
                    if l + o + k <= l + u:
                        pk[k] += a * float(c[l + o + k]) * shift(live, -k)
        Pd, P1, P2 = pk
        omega = 1.0 / (2.0 * Tf)

        def band(y):
            py = Pd * y
            py[:, :-1] += P1[:, :-1] * y[:, 1:]
            py[:, :-2] += P2[:, :-2] * y[:, 2:]
            py[:, 1:] += P1[:, :-1] * y[:, :-1]
            py[:, 2:] += P2[:, :-2] * y[:, :-2]
            return py

        def mean_var(y):
            m = y.sum(dim=1, keepdim=True) / Tf
            e = (y - m) * live
            return m, (e * e).sum(dim=1, keepdim=True) / Tf

        rows = Pd.abs() + P1.abs() + P2.abs() + shift(P1, 1).abs() + shift(P2, 2).abs()
        Gmax = rows.max(dim=1, keepdim=True)[0]

        def composed():
            y = y0.clone()
            m, v = mean_var(y)
            y = (m + torch.sqrt(gv_mean / v) * (y - m)) * live
            m, v = mean_var(y)
            alpha = 1.0 / (omega * Gmax + 2.0 / Tf * gv_prec * ((v - gv_mean).abs() + 2.0 * torch.maximum(v, gv_mean.expand_as(v))))
            for _ in range(n_iter):
                grad = omega * (r - band(y)) - 2.0 / Tf * gv_prec * (v - gv_mean) * (y - m)
                y = (y + alpha * grad) * live
                m, v = mean_var(y)
            return y

        ybuf = torch.empty_like(y0)

        def kernel():
            return _hip.gv_ascent(mean, var, WINDOWS, y0, gv_mean, gv_prec, Ld, n_iter=n_iter, out=ybuf)

        yk, report, status = kernel()
        yc = composed()
        res = dict(path="gv-ascent-corpus", B=B, Tmax=Tmax, D=D, static_dim=sd, frames=frames, n_iter=n_iter, systems=B * sd,
                   status_nonzero=int((status != 0).sum().item()),
                   kernel_vs_composed_rel=float(((yk - yc).abs().max() / yc.abs().max()).item()),
                   gv_ml_over_mean=float((gv0.mean(dim=0) / gv_mean).mean().item()),
                   gv_final_over_mean=float((report[:, :, 3].mean(dim=0) / gv_mean).mean().item()))
        for _ in range(3):                               # settle the clocks on both
            kernel()
        composed()
        t_new, t_old = [], []
        for _ in range(4 if args.quick else 12):
            t_new += events(kernel, 1)
            t_old += events(composed, 1)
        res["kernel"], res["composed"] = spread(t_new), spread(t_old)
        res["composed_over_kernel"] = res["composed"]["median_ms"] / res["kernel"]["median_ms"]
        res["note"] = ("the corpus of --only vc; mean and var from mlpg_hip_gmm_trajectory_stats, y0 from batched MLPG, the gv statistics "
                       "1.8 x the mean gv of y0 with a standard deviation of 0.2 of that.  HIP-event times, alternating pairs, of ONE launch "
                       "of mlpg_hip_gv_ascent (scaled start, derived step, 100 iterations, out of place) against the same iteration composed "
                       "from torch operations on resident float64 tensors (the band columns of P, r and the row sums built once outside the "
                       "timed region; the banded product by shifted slices).  The composed route is the yardstick: the parent has no such "
                       "capability.  No counters were collected; no time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_GVMLPG_PROFILE") or os.path.join(ROOT, "profiles", "gvmlpg.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- trajcov: the band of the trajectory covariance, log det R, the likelihood and its gradients; only with --only trajcov ----
    if args.only and "trajcov" in args.only.split(","):
        from nnmnkwii_amd import _trajectory_calls as TC
        nw, Q = len(WINDOWS), 2
        res = dict(path="trajcov", hbm_peak_gbs=HBM_PEAK_GBS, dtype="float64", windows="static + delta + delta-delta")

        def timed(fn, steps, warmup=2):
            gpu_time(fn, steps=1, warmup=warmup)                                  # warm-up and settled clocks
            return spread(events(fn, steps))

        def case(B, T, sd, lo):
            rng = np.random.RandomState(1234)
            lens = rng.randint(lo, T + 1, size=B).astype(np.int32)
            g2 = torch.Generator(device=dev).manual_seed(4321)
            m = torch.randn(B, T, nw * sd, dtype=torch.float64, device=dev, generator=g2)
            v = torch.rand(B, T, nw * sd, dtype=torch.float64, device=dev, generator=g2) + 0.5
            c = torch.randn(B, T, sd, dtype=torch.float64, device=dev, generator=g2)
            return lens, torch.from_numpy(lens).to(dev), m, v, c

        def device_route(B, T, sd, L, m, v, c, steps):
            D = nw * sd
            band = torch.empty((Q + 1, B, T, sd), dtype=torch.float64, device=dev)
            logdet = torch.empty((B, sd), dtype=torch.float64, device=dev)
            status = torch.empty((B, sd), dtype=torch.int32, device=dev)
            cbar, _ = _hip.forward(m, v, WINDOWS, L, want_status=False)
            cov = lambda: TC.covariance(v, WINDOWS, L, B, T, D, band=band, logdet=logdet, status=status)  # noqa: E731
            fwd = lambda: TC.covariance(v, WINDOWS, L, B, T, D, want_band=False, logdet=logdet, status=status)  # noqa: E731

            def both():
                cov()
                return TC.nll(m, v, WINDOWS, cbar, c, L, band, logdet)
            r = dict(cov_ms=timed(cov, steps))
            r["logdet_only_ms"] = timed(fwd, steps)
            r["cov_nll_grads_ms"] = timed(both, steps)
            nll, gm, gv = both()
            torch.cuda.synchronize()
            return r, band, logdet, status, nll, gm, gv

        # -- the full shape: against a plain copy of the bytes each must move
        B, T, sd = (16, 200, 60) if args.quick else (256, 1000, 60)
        D = nw * sd
        lens, L, m, v, c = case(B, T, sd, T // 2)
        live = int(lens.sum())
        r, band, logdet, status, nll, gm, gv = device_route(B, T, sd, L, m, v, c, 20)
        cov_bytes = 8.0 * (live * D + (Q + 1) * B * T * sd)                     # the variances in, every row of the band out
        nll_bytes = 8.0 * (2 * live * D + 2 * live * sd + (Q + 1) * live * sd + 2 * B * T * D)   # means, variances, cbar, target, band in; two gradients out
        for key, nbytes in (("cov", cov_bytes), ("cov_nll_grads", cov_bytes + nll_bytes)):
            src = torch.empty(int(nbytes // 16), dtype=torch.float64, device=dev)
            dst = torch.empty_like(src)
            copy_ms = timed(lambda: dst.copy_(src), 20)
            ms = r["%s_ms" % key]["median_ms"]
            r["%s_bytes" % key] = nbytes
            r["%s_copy_ms" % key] = copy_ms
            r["%s_hbm_frac" % key] = nbytes / (ms * 1e6) / HBM_PEAK_GBS
            r["%s_over_copy" % key] = ms / copy_ms["median_ms"]
            del src, dst
        r.update(B=B, T=T, D=D, live_frames=live, bad_systems=int((status != 0).sum()), wavefronts=B * ((sd + 63) // 64))
        res["full"] = r
        del m, v, c, band, gm, gv

        # -- a shape whose dense matrices fit: against the composed route
        B, T, sd = (2, 100, 60) if args.quick else (8, 500, 60)
        D = nw * sd
        lens, L, m, v, c = case(B, T, sd, T)                                     # full lengths: the dense route has no padding rule
        r, band, logdet, status, nll, gm, gv = device_route(B, T, sd, L, m, v, c, 20)
        W = torch.zeros((nw, T, T), dtype=torch.float64, device=dev)
        for w, (l, u, cf) in enumerate(WINDOWS):
            for k in range(-l, u + 1):
                i = torch.arange(max(0, -k), min(T, T - k), device=dev)
                W[w, i, i + k] = float(cf[l + k])
        edge = torch.ones((nw, T), dtype=torch.float64, device=dev)
        edge[1:, 0] = 0.0
        edge[1:, T - 1] = 0.0

        def dense_R(var):
            tau = (1.0 / var).view(B, T, nw, sd).permute(0, 3, 2, 1) * edge       # (B, sd, nw, T)
            return torch.einsum("wts,bdwt,wtu->bdsu", W, tau, W), tau

        lu = dict(chunk=B * sd)     # systems per call of torch.linalg.inv / solve / logdet: all of them, an utterance's, or one

        def chunked(fn, *ts):
            n = ts[0].shape[0]
            outs = [fn(*[t[k:k + lu["chunk"]] for t in ts]) for k in range(0, n, lu["chunk"])]
            return outs[0] if len(outs) == 1 else torch.cat(outs)

        def inv_logdet(R):
            Rf = R.reshape(B * sd, T, T)
            return chunked(torch.linalg.inv, Rf).view(B, sd, T, T), chunked(torch.logdet, Rf).view(B, sd)

        def solve_logdet(R, rhs):
            Rf = R.reshape(B * sd, T, T)
            return chunked(torch.linalg.solve, Rf, rhs.reshape(B * sd, T)).view(B, sd, T), chunked(torch.logdet, Rf).view(B, sd)

        def composed_cov():
            R, _ = dense_R(v)
            return inv_logdet(R)

        def composed_nll():
            mm, vv = m.detach().requires_grad_(), v.detach().requires_grad_()
            R, tau = dense_R(vv)
            mu = mm.view(B, T, nw, sd).permute(0, 3, 2, 1)                         # (B, sd, nw, T)
            rhs = torch.einsum("wts,bdwt->bds", W, tau * mu)
            cb_, ld_ = solve_logdet(R, rhs)
            e = c.permute(0, 2, 1) - cb_
            out = 0.5 * torch.einsum("bds,bdsu,bdu->bd", e, R, e) - 0.5 * ld_ + 0.5 * T * math.log(2 * math.pi)
            out.sum().backward()
            return out.detach(), mm.grad, vv.grad
        for chunk in (B * sd, sd, 1):     # the BLAS library's batched LU and triangular solves can run out of their own workspace
            lu["chunk"] = chunk
            try:
                composed_cov()
                composed_nll()
                torch.cuda.synchronize()
                break
            except RuntimeError as err:
                r["composed_error_at_%d_systems_a_call" % chunk] = str(err).splitlines()[0][:200]
        r["composed_systems_per_call"] = lu["chunk"]
        r["composed_cov_ms"] = timed(composed_cov, 5, warmup=1)
        r["composed_nll_grads_ms"] = timed(composed_nll, 5, warmup=1)
        S, ld = composed_cov()
        cn, cgm, cgv = composed_nll()
        r["band_max_abs_diff_vs_composed"] = float(max((torch.diagonal(S, k, 2, 3).permute(0, 2, 1) - band[k, :, :T - k]).abs().max() for k in range(Q + 1)))
        r["logdet_max_abs_diff_vs_composed"] = float((ld - logdet).abs().max())
        r["nll_max_rel_diff_vs_composed"] = float(((cn - nll).abs() / cn.abs()).max())
        r["grad_means_max_abs_diff_vs_composed"] = float((cgm - gm).abs().max())
        r["grad_vars_max_abs_diff_vs_composed"] = float((cgv - gv).abs().max())
        r["composed_cov_over_cov"] = r["composed_cov_ms"]["median_ms"] / r["cov_ms"]["median_ms"]
        r["composed_nll_over_cov_nll"] = r["composed_nll_grads_ms"]["median_ms"] / r["cov_nll_grads_ms"]["median_ms"]
        r.update(B=B, T=T, D=D, dense_bytes_per_matrix=8.0 * B * sd * T * T)
        res["dense_fits"] = r
        res["note"] = ("HIP-event times of single calls on settled clocks (median, min, max, quartiles of 20; 5 for the composed routes).  "
                       "cov: ONE launch of nnmk_traj_covariance into a caller's band; logdet_only: the same with want_band = 0; cov_nll_grads: "
                       "that launch plus ONE of nnmk_traj_nll with both gradients (cbar is made beforehand by mlpg_hip_forward and not timed).  "
                       "bytes: the variances of the live frames in and every row of the band out; for the likelihood also means, variances, cbar, "
                       "target and band of the live frames in and two full gradients out.  copy: torch's dst.copy_(src) of half those bytes (it "
                       "reads and writes them).  hbm_frac: bytes over time as a fraction of 8 TB/s.  composed: R assembled densely by einsum, "
                       "then inverse and log-determinant over all (B, sd) systems, and autograd of the dense likelihood through a dense "
                       "solve and log-determinant: torch.linalg.inv / solve / logdet over composed_systems_per_call systems a call (all of "
                       "them where the library's batched routines take that); full lengths.  No counters were collected; no time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_TRAJCOV_PROFILE") or os.path.join(ROOT, "profiles", "trajcov.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- trajsample: draws from the trajectory distribution and the whitening map; only with --only trajsample ----
    if args.only and "trajsample" in args.only.split(","):
        from nnmnkwii_amd import _sample_calls as SC, _trajectory_calls as TC
        nw, Q, G = len(WINDOWS), 2, SC.draw_group()
        res = dict(path="trajsample", hbm_peak_gbs=HBM_PEAK_GBS, dtype="float64", windows="static + delta + delta-delta", draw_group=G)

        def timed(fn, steps, warmup=2):
            gpu_time(fn, steps=1, warmup=warmup)                                  # warm-up and settled clocks
            return spread(events(fn, steps))

        def case(B, T, sd, lo, K):
            rng = np.random.RandomState(1234)
            lens = rng.randint(lo, T + 1, size=B).astype(np.int32)
            g2 = torch.Generator(device=dev).manual_seed(4321)
            v = torch.rand(B, T, nw * sd, dtype=torch.float64, device=dev, generator=g2) + 0.5
            c = torch.randn(B, T, sd, dtype=torch.float64, device=dev, generator=g2)
            z = torch.randn(K, B, T, sd, dtype=torch.float64, device=dev, generator=g2)
            return lens, torch.from_numpy(lens).to(dev), v, c, z

        def against_copy(r, key, nbytes):
            src = torch.empty(int(nbytes // 16), dtype=torch.float64, device=dev)
            dst = torch.empty_like(src)
            copy_ms = timed(lambda: dst.copy_(src), 20)
            ms = r["%s_ms" % key]["median_ms"]
            r["%s_bytes" % key] = nbytes
            r["%s_copy_ms" % key] = copy_ms
            r["%s_hbm_frac" % key] = nbytes / (ms * 1e6) / HBM_PEAK_GBS
            r["%s_over_copy" % key] = ms / copy_ms["median_ms"]

        # -- the full shape: against a plain copy of the bytes each must move
        B, T, sd = (16, 200, 60) if args.quick else (256, 1000, 60)
        D = nw * sd
        KS = sorted({1, G, 16})
        lens, L, v, c, z = case(B, T, sd, T // 2, max(KS))
        live = int(lens.sum())
        fac = torch.empty((Q + 1, B, T, sd), dtype=torch.float64, device=dev)
        logdet = torch.empty((B, sd), dtype=torch.float64, device=dev)
        status = torch.empty((B, sd), dtype=torch.int32, device=dev)
        out = torch.empty_like(z)
        r = dict(factor_ms=timed(lambda: SC.factor(v, WINDOWS, L, B, T, D, factor=fac, logdet=logdet, status=status), 20))
        r["traj_covariance_want_band_0_ms"] = timed(lambda: TC.covariance(v, WINDOWS, L, B, T, D, want_band=False, logdet=logdet, status=status), 20)
        r["factor_over_traj_covariance_want_band_0"] = r["factor_ms"]["median_ms"] / r["traj_covariance_want_band_0_ms"]["median_ms"]
        against_copy(r, "factor", 8.0 * (live * D + (Q + 1) * B * T * sd))         # the variances in, every row of the factor out
        SC.factor(v, WINDOWS, L, B, T, D, factor=fac, logdet=logdet, status=status)
        for K in KS:
            key = "sample_K%d" % K
            r[key + "_ms"] = timed(lambda: SC.sample(fac, status, L, z[:K], c, out=out[:K]), 20)
            r[key + "_per_draw_ms"] = r[key + "_ms"]["median_ms"] / K
            against_copy(r, key, 8.0 * ((Q + 1) * live * sd + K * live * sd + live * sd + K * B * T * sd))   # factor, noise, mean in; K draws out
        r["per_draw_K%d_over_K1" % G] = r["sample_K%d_per_draw_ms" % G] / r["sample_K1_per_draw_ms"]
        r["per_draw_K16_over_K1"] = r["sample_K16_per_draw_ms"] / r["sample_K1_per_draw_ms"]
        back = torch.empty_like(z[:1])
        r["whiten_K1_ms"] = timed(lambda: SC.whiten(fac, status, L, out[:1], c, out=back), 20)
        against_copy(r, "whiten_K1", 8.0 * ((Q + 1) * live * sd + live * sd + live * sd + B * T * sd))
        SC.sample(fac, status, L, z[:1], c, out=out[:1])
        SC.whiten(fac, status, L, out[:1], c, out=back)
        torch.cuda.synchronize()
        mask = (torch.arange(T, device=dev)[None, :] < L[:, None])[None, :, :, None]
        r["round_trip_max_abs_diff"] = float(((back - z[:1]) * mask).abs().max())
        r.update(B=B, T=T, D=D, live_frames=live, bad_systems=int((status != 0).sum()), wavefronts=B * ((sd + 63) // 64))
        res["full"] = r
        del v, c, z, out, fac, back

        # -- a shape whose dense matrices fit: against the composed route (R by einsum, Cholesky, a triangular solve)
        B, T, sd = (2, 100, 60) if args.quick else (8, 500, 60)
        D = nw * sd
        K = 1
        lens, L, v, c, z = case(B, T, sd, T, K)                                    # full lengths: the dense route has no padding rule
        fac, logdet, status = SC.factor(v, WINDOWS, L, B, T, D)
        out = torch.empty_like(z)

        def device_route():
            SC.factor(v, WINDOWS, L, B, T, D, factor=fac, logdet=logdet, status=status)
            return SC.sample(fac, status, L, z, c, out=out)
        r = dict(factor_sample_ms=timed(device_route, 20))
        W = torch.zeros((nw, T, T), dtype=torch.float64, device=dev)
        for w, (l, u, cf) in enumerate(WINDOWS):
            for k in range(-l, u + 1):
                i = torch.arange(max(0, -k), min(T, T - k), device=dev)
                W[w, i, i + k] = float(cf[l + k])
        edge = torch.ones((nw, T), dtype=torch.float64, device=dev)
        edge[1:, 0] = 0.0
        edge[1:, T - 1] = 0.0

        def composed():
            tau = (1.0 / v).view(B, T, nw, sd).permute(0, 3, 2, 1) * edge         # (B, sd, nw, T)
            R = torch.einsum("wts,bdwt,wtu->bdsu", W, tau, W)
            C = torch.linalg.cholesky(R)                                          # R = C C^T
            x = torch.linalg.solve_triangular(C.transpose(-1, -2), z[0].permute(0, 2, 1).unsqueeze(-1), upper=True)
            return c + x.squeeze(-1).permute(0, 2, 1)
        try:
            composed()
            torch.cuda.synchronize()
            r["composed_ms"] = timed(composed, 5, warmup=1)
            r["draw_max_abs_diff_vs_composed"] = float((composed() - device_route()[0]).abs().max())
            r["composed_over_factor_sample"] = r["composed_ms"]["median_ms"] / r["factor_sample_ms"]["median_ms"]
        except RuntimeError as err:
            r["composed_error"] = str(err).splitlines()[0][:200]
        r.update(B=B, T=T, D=D, K=K, dense_bytes_per_matrix=8.0 * B * sd * T * T)
        res["dense_fits"] = r
        res["note"] = ("HIP-event times of single calls on settled clocks (median, min, max, quartiles of 20; 5 for the composed route).  "
                       "factor: ONE launch of nnmk_draw_factor into a caller's planes; traj_covariance_want_band_0: nnmk_traj_covariance's "
                       "forward sweep on the same inputs; sample_K*: ONE launch of nnmk_draw_sample for K draws with a mean (draw_group draws "
                       "side by side in a lane); whiten_K1: ONE launch of nnmk_draw_whiten.  bytes: the variances of the live frames in and "
                       "every row of the factor out; for the draws the factor, the noise and the mean of the live frames in and every row of "
                       "the K draws out.  copy: torch's dst.copy_(src) of half those bytes (it reads and writes them).  hbm_frac: bytes over "
                       "time as a fraction of 8 TB/s.  composed: R assembled densely by einsum, torch.linalg.cholesky and "
                       "torch.linalg.solve_triangular over all (B, sd) systems, one draw; factor_sample: the two launches that give the same "
                       "draw; full lengths.  No counters or traces were collected; no time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_TRAJSAMPLE_PROFILE") or os.path.join(ROOT, "profiles", "trajsample.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- norm: corpus normalisation over a config-5 sized padded batch: statistics in one pass, the affine map; only with --only norm ----
    if args.only and "norm" in args.only.split(","):
        B, T, D = (64, 500, 187) if args.quick else (512, 2000, 187)
        rng = np.random.RandomState(1234)
        lens = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
        live = int(lens.sum())
        lengths = torch.from_numpy(lens).to(dev)
        mask = (torch.arange(T, device=dev)[None, :] < lengths[:, None])[:, :, None]
        res = dict(path="norm-config5", B=B, T=T, D=D, live_frames=live, hbm_peak_gbs=HBM_PEAK_GBS,
                   chunk_rows=_hip.COLSTATS_CHUNK_ROWS, block_rows=_hip.COLSTATS_BLOCK_ROWS)
        host = rng.randn(B, T, D) * (0.2 + rng.rand(D)) + 3.0 * rng.randn(D)
        ws = torch.empty(_hip.column_stats_workspace(B, T, D) // 8, dtype=torch.float64, device=dev)
        state = torch.empty((5, D), dtype=torch.float64, device=dev)
        n = float(live)
        inf = float("inf")

        def composed_stats(x):
            xd = x.to(torch.float64)
            mean = (xd * mask).sum(dim=(0, 1)) / n
            var = (((xd - mean) * mask) ** 2).sum(dim=(0, 1)) / n
            return mean, var, torch.where(mask, xd, inf).amin(dim=(0, 1)), torch.where(mask, xd, -inf).amax(dim=(0, 1))

        for name, tdt, size in (("float32", torch.float32, 4), ("float64", torch.float64, 8)):
            x = torch.from_numpy(host).to(dev).to(tdt)
            nbytes = float(size) * live * D
            r = dict(stats_bytes=nbytes, apply_bytes=2 * nbytes)
            r["stats_ms"] = gpu_time(lambda: _hip.column_stats(x, lengths, None, state, ws), steps=20)
            r["stats_composed_ms"] = gpu_time(lambda: composed_stats(x), steps=10)
            mean, var, mn, mx = composed_stats(x)
            st = state.clone()
            std = (st[2] / st[0]).sqrt()
            r["stats_hbm_frac"] = nbytes / (r["stats_ms"] * 1e6) / HBM_PEAK_GBS
            r["stats_mean_rel_err_vs_composed"] = float(((st[1] - mean).abs() / mean.abs()).max())
            r["stats_var_rel_err_vs_composed"] = float(((st[2] / st[0] - var).abs() / var).max())
            r["stats_extrema_equal"] = bool(torch.equal(st[3], mn) and torch.equal(st[4], mx))
            out = torch.empty_like(x)
            a, c = std.contiguous(), st[1].contiguous()
            for mode, word, expr in ((0, "scale", lambda: torch.where(mask, (x - c) / a, 0.0).to(tdt)),
                                     (1, "inv_scale", lambda: torch.where(mask, a * x + c, 0.0).to(tdt))):
                r["%s_ms" % word] = gpu_time(lambda: _hip.column_affine(x, a, c, mode, lengths, out), steps=20)
                r["%s_composed_ms" % word] = gpu_time(expr, steps=10)
                r["%s_hbm_frac" % word] = 2 * nbytes / (r["%s_ms" % word] * 1e6) / HBM_PEAK_GBS
                r["%s_max_abs_diff_vs_composed" % word] = float((out.to(torch.float64) - expr().to(torch.float64)).abs().max())
            res[name] = r
        res["note"] = ("lengths in [T/2, T]; HIP-event medians on settled clocks.  stats: ONE call of mlpg_hip_column_stats (the statistics "
                       "kernel and its finish step, workspace given) against count, mean, variance, min and max composed from masked torch "
                       "reductions in float64; scale / inv_scale: one launch of mlpg_hip_column_affine (modes 0 and 1) against the broadcast "
                       "torch expression plus masking.  hbm_frac: 4 | 8 bytes * live frames * D (twice that for the apply) over the time, as "
                       "a fraction of 8 TB/s.  The composed routes are the yardstick: the parent has no such capability.  No counters "
                       "were collected; no time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_NORM_PROFILE") or os.path.join(ROOT, "profiles", "norm.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- metrics: the four-term Merlin evaluation over a config-5 sized padded batch, one call; only with --only metrics ----
    if args.only and "metrics" in args.only.split(","):
        from nnmnkwii_amd import _metrics_hip as MH
        from nnmnkwii_amd import metrics as MT
        B, T, D = (64, 500, 187) if args.quick else (512, 2000, 187)
        rng = np.random.RandomState(1234)
        lens = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
        live = int(lens.sum())
        lengths = torch.from_numpy(lens).to(dev)
        # Merlin's acoustic feature matrix: mgc 0 .. 59 (MCD without the energy), lf0 60, vuv 61, bap 62 .. 64
        MGC, LF0, VUV, BAP = slice(1, 60), 60, 61, slice(62, 65)
        host_y = rng.randn(B, T, D).astype(np.float32)
        host_y[:, :, LF0] = 5.0 + 0.3 * rng.randn(B, T)
        host_y[:, :, VUV] = rng.rand(B, T) < 0.7
        host_x = host_y + 0.3 * rng.randn(B, T, D).astype(np.float32)
        host_x[:, :, VUV] = np.where(rng.rand(B, T) < 0.9, host_y[:, :, VUV], 1.0 - host_y[:, :, VUV])
        X, Y = torch.from_numpy(host_x).to(dev), torch.from_numpy(host_y).to(dev)
        terms = [MH.term(MH.FRAME_L2, 1, width=59), MH.term(MH.SQUARED, 62, width=3), MH.term(MH.VOICED_SQUARED, LF0, x_mask_col=VUV),
                 MH.term(MH.MISMATCH, VUV)]
        ws = torch.empty(MH.metrics_workspace(B, T, len(terms)) // 8, dtype=torch.float64, device=dev)
        spec = {"mcd": ("melcd", MGC), "bap": ("mse", BAP), "lf0": ("lf0_mse", LF0, VUV), "vuv": ("vuv_error", VUV)}
        lens_list = [int(n) for n in lens]

        def loop():            # the reference's batched forms: a Python loop over the utterances, a float() each (metrics/__init__.py:64-183)
            s = [0.0, 0.0, 0.0, 0.0]
            voiced = 0
            for x, y, n in zip(X, Y, lens_list):
                x, y = x[:n], y[:n]
                z = x[:, MGC] - y[:, MGC]
                s[0] += float((z * z).sum(-1).sqrt().sum())
                z = x[:, BAP] - y[:, BAP]
                s[1] += float((z * z).sum())
                v = (x[:, VUV] + y[:, VUV]) >= 2
                voiced += int(v.sum())
                z = x[:, LF0][v] - y[:, LF0][v]
                s[2] += float((z * z).sum())
                s[3] += float((x[:, VUV] != y[:, VUV]).sum())
            return dict(mcd=float(MT._logdb_const) * s[0] / live, bap=math.sqrt(s[1] / (live * 3)), lf0=math.sqrt(s[2] / voiced), vuv=s[3] / live)

        mask = torch.arange(T, device=dev)[None, :] < lengths[:, None]

        def vectorised():      # masked torch expressions over the whole batch, float64 sums, one copy back
            z = X[:, :, MGC] - Y[:, :, MGC]
            mcd = ((z * z).sum(-1, dtype=torch.float64).sqrt() * mask).sum()
            z = X[:, :, BAP] - Y[:, :, BAP]
            bap = ((z * z).sum(-1, dtype=torch.float64) * mask).sum()
            v = ((X[:, :, VUV] + Y[:, :, VUV]) >= 2) & mask
            z = (X[:, :, LF0] - Y[:, :, LF0]).to(torch.float64)
            lf0 = (z * z * v).sum()
            vuv = ((X[:, :, VUV] != Y[:, :, VUV]) & mask).sum()
            r = torch.stack([mcd, bap, lf0, v.sum().to(torch.float64), vuv.to(torch.float64)]).cpu().numpy()
            return dict(mcd=float(MT._logdb_const) * r[0] / live, bap=math.sqrt(r[1] / (live * 3)), lf0=math.sqrt(r[2] / r[3]), vuv=r[4] / live)

        nbytes = 4.0 * live * 2 * (59 + 3 + 1 + 1)             # the bytes the four terms need: 64 float32 columns of x and of y
        span_bytes = 4.0 * live * 2 * 64                        # the bytes the kernel loads: columns 1 .. 64, the span of the terms
        res = dict(path="metrics-config5", B=B, T=T, D=D, live_frames=live, hbm_peak_gbs=HBM_PEAK_GBS, block_rows=MH.BLOCK_ROWS,
                   needed_bytes=nbytes, span_bytes=span_bytes)
        res["kernel_ms"] = gpu_time(lambda: MH.metrics_batch(X, Y, terms, lengths, workspace=ws), steps=20)
        res["kernel_hbm_frac"] = nbytes / (res["kernel_ms"] * 1e6) / HBM_PEAK_GBS
        # the routes a user sees: wall clock to the floats on the host, everything included
        res["one_call_wall_ms"] = wall_time(lambda: MT.batch_metrics(X, Y, lengths, spec), steps=50, warmup=5)
        res["vectorised_wall_ms"] = wall_time(vectorised, steps=20, warmup=3)
        res["loop_wall_ms"] = wall_time(loop, steps=2, warmup=1, repeats=2)
        res["vectorised_over_one_call"] = res["vectorised_wall_ms"] / res["one_call_wall_ms"]
        res["loop_over_one_call"] = res["loop_wall_ms"] / res["one_call_wall_ms"]
        a, b, c = MT.batch_metrics(X, Y, lengths, spec), vectorised(), loop()
        res["values"] = a
        res["max_rel_diff_vs_vectorised"] = max(abs(a[k] - b[k]) / abs(b[k]) for k in a)
        res["max_rel_diff_vs_loop"] = max(abs(a[k] - c[k]) / abs(c[k]) for k in a)
        res["note"] = ("float32 (B, T, 187) prediction and target, lengths in [T/2, T]; terms: mgc MCD (59 columns), bap distortion (3), lf0 "
                       "RMSE on voiced frames, V/UV error.  kernel_ms: HIP-event median of ONE call of nnmk_metrics_batch (both launches, "
                       "workspace given) on settled clocks; kernel_hbm_frac: the bytes the terms need over that time as a fraction of 8 TB/s.  "
                       "*_wall_ms: wall clock of a whole evaluation down to Python floats -- batch_metrics (the kernel, one copy of 8 doubles), "
                       "masked vectorised torch expressions with float64 sums (one copy), and the reference's per-utterance loop with a "
                       "float() per reduction (float32 sums, as the reference) -- all on the same tensors.  No counters were collected; no "
                       "time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_METRICS_PROFILE") or os.path.join(ROOT, "profiles", "metrics.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- frontend: phone-level linguistic features expanded to frames over a config-5 sized padded batch; only with --only frontend ----
    if args.only and "frontend" in args.only.split(","):
        from nnmnkwii_amd import _frontend_hip as FH
        from nnmnkwii_amd.frontend import merlin as FE
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import frontend_model as FM
        B, Tlo, Thi, Dl, S = (32, 1000, 2000, 416, 5) if args.quick else (512, 1000, 2000, 416, 5)
        rng = np.random.RandomState(1234)
        nph = rng.randint(60, 101, size=B).astype(np.int32)
        Nmax, F = 100, 9
        W = Dl + F
        frames = rng.randint(Tlo, Thi + 1, size=B)
        host_d = np.zeros((B, Nmax, S), dtype=np.int32)
        for b in range(B):                                   # the utterance's frames dealt to its states
            host_d[b, :nph[b]] = rng.multinomial(frames[b], np.ones(nph[b] * S) / (nph[b] * S)).reshape(nph[b], S)
        host_P = ((rng.rand(B, Nmax, Dl) < 0.2) + (rng.rand(B, Nmax, Dl) < 0.05) * rng.randn(B, Nmax, Dl)).astype(np.float32)
        scale_h, min_h = rng.rand(W) + 0.5, rng.randn(W)
        P, d, n = torch.from_numpy(host_P).to(dev), torch.from_numpy(host_d).to(dev), torch.from_numpy(nph).to(dev)
        sc, mn = torch.from_numpy(scale_h).to(dev), torch.from_numpy(min_h).to(dev)
        Tmax = Thi
        out = torch.empty((B, Tmax, W), dtype=torch.float32, device=dev)
        live = int(frames.sum())
        # the composed torch route, on the same tensors: the state of every frame by repeat_interleave, the nine columns by tensor
        # arithmetic in float64, the phone rows gathered, cat, the affine expression, one rounding, the rows placed into the padded batch
        r = d.to(torch.int64) * (torch.arange(Nmax, device=dev)[None, :, None] < n[:, None, None])
        state_ids = torch.arange(B * Nmax * S, device=dev)

        def composed(affine):
            rf = r.reshape(-1)
            idx = torch.repeat_interleave(state_ids, rf, output_size=live)            # the state of every frame of the batch
            ends = torch.cumsum(rf, 0)
            g = torch.arange(live, device=dev)
            i = (g - (ends - rf)[idx]).to(torch.float64)
            fn = rf[idx].to(torch.float64)
            phone = idx // S
            s = (idx % S + 1).to(torch.float64)
            pd = r.sum(-1).reshape(-1)[phone].to(torch.float64)
            base = (torch.cumsum(r, -1) - r).reshape(-1)[idx].to(torch.float64)
            nine = torch.stack([(i + 1) / fn, (fn - i) / fn, fn, s, S + 1 - s, pd, fn / pd, (pd - i - base) / pd, (base + i + 1) / pd], dim=1)
            rows = torch.cat([P.reshape(-1, Dl)[phone].to(torch.float64), nine], dim=1)
            if affine:
                rows = rows * sc + mn
            utt = idx // (Nmax * S)
            first = torch.cumsum(r.sum((1, 2)), 0) - r.sum((1, 2))                     # the batch index of every utterance's frame 0
            res = torch.zeros((B, Tmax, W), dtype=torch.float32, device=dev)
            res.view(-1, W)[utt * Tmax + (g - first[utt])] = rows.to(torch.float32)
            return res

        in_bytes = float(host_P.nbytes + host_d.nbytes + nph.nbytes)
        out_bytes = 4.0 * B * Tmax * W
        res = dict(path="frontend-config5", B=B, Tmax=Tmax, Nmax=Nmax, S=S, Dl=Dl, F=F, live_frames=live, hbm_peak_gbs=HBM_PEAK_GBS,
                   block_rows=FH.BLOCK_ROWS, out_bytes=out_bytes, in_bytes=in_bytes)
        res["fill_ms"] = gpu_time(lambda: out.zero_(), steps=20)     # a yardstick: torch's fill of the same output, stores alone
        res["fill_hbm_frac"] = out_bytes / (res["fill_ms"] * 1e6) / HBM_PEAK_GBS
        for affine, tag in ((False, "plain"), (True, "affine")):
            a, b_ = (sc, mn) if affine else (None, None)
            res["kernel_%s_ms" % tag] = gpu_time(lambda: FH.expand(P, d, n, FH.FULL, 0, None, a, b_, out), steps=20)
            res["kernel_%s_hbm_frac" % tag] = (out_bytes + in_bytes) / (res["kernel_%s_ms" % tag] * 1e6) / HBM_PEAK_GBS
            res["one_call_%s_wall_ms" % tag] = wall_time(lambda: FE.frame_features_batch(P, d, n, "full", min_frames=0, scale_=a, min_=b_, out=out,
                                                                                         strict=False), steps=20, warmup=3)
            res["composed_%s_ms" % tag] = gpu_time(lambda: composed(affine), steps=5, warmup=1)
            res["composed_over_kernel_%s" % tag] = res["composed_%s_ms" % tag] / res["kernel_%s_ms" % tag]
            FH.expand(P, d, n, FH.FULL, 0, None, a, b_, out)
            res["equal_to_composed_%s" % tag] = bool(torch.equal(out, composed(affine)))
        # the specification's per-frame loop (the reference's loop with the regular expressions taken out) on eight utterances, scaled
        t0 = time.perf_counter()
        for b in range(8):
            m = FM.frame_features(host_P[b, :nph[b]], host_d[b, :nph[b]], "full", 0, scale_h, min_h, np.float32)
            assert np.array_equal(m, out[b, :len(m)].cpu().numpy())
        res["model_loop_8_utterances_ms"] = (time.perf_counter() - t0) * 1e3
        res["model_loop_scaled_ms"] = res["model_loop_8_utterances_ms"] * live / float(frames[:8].sum())
        res["note"] = ("float32 (B, 100, 416) phone-level features, 60 .. 100 phones x 5 states per utterance, int32 durations that add up to "
                       "1000 .. 2000 frames, kind full, float32 (B, 2000, 425) out.  kernel_*_ms: HIP-event median of ONE launch of "
                       "nnmk_frontend_expand on settled clocks, without and with the fused affine map; kernel_*_hbm_frac: the bytes of the whole "
                       "padded output plus the inputs over that time as a fraction of 8 TB/s; fill_ms: torch's zero_() of the same output "
                       "tensor, what stores alone reach.  one_call_*_wall_ms: wall clock of "
                       "frame_features_batch(out=, strict=False) in a back-to-back loop.  composed_*_ms: the same padded result from torch "
                       "operations on the same tensors (repeat_interleave with output_size, nine columns in float64, gather, cat, affine, one "
                       "rounding, index_put into zeros); equal_to_composed_*: torch.equal of the two results.  model_loop_*: "
                       "tools/frontend_model.py's per-frame Python loop on the first eight utterances (each compared with the kernel's rows, "
                       "np.array_equal), scaled by live frames to the batch.  No counters were collected; no time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_FRONTEND_PROFILE") or os.path.join(ROOT, "profiles", "frontend.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- f0: the lf0 column of a config-5 sized padded batch filled in place, the flag into the vuv column; only with --only f0 ----
    if args.only and "f0" in args.only.split(","):
        from nnmnkwii_amd import _f0_hip as F0H
        from nnmnkwii_amd import preprocessing as PP
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import f0_model as F0M
        B, Tlo, Thi, W, LF0, VUV = (32, 1000, 2000, 187, 180, 181) if args.quick else (512, 1000, 2000, 187, 180, 181)
        rng = np.random.RandomState(1234)
        Tmax = Thi
        lens_h = rng.randint(Tlo, Thi + 1, size=B).astype(np.int32)
        host_X = rng.randn(B, Tmax, W).astype(np.float32)
        for b in range(B):                                   # log-F0 in voiced runs of about 30 frames, unvoiced runs of about 20
            t, on = 0, rng.rand() < 0.6
            while t < Tmax:
                n = 1 + rng.geometric(1.0 / (30 if on else 20))
                host_X[b, t:t + n, LF0] = (4.5 + rng.rand(min(n, Tmax - t))) if on else -1e10
                t += n
                on = not on
        live = int(lens_h.sum())
        unvoiced_share = float(np.mean([np.mean(host_X[b, :lens_h[b], LF0] <= 0) for b in range(B)]))
        X0 = torch.from_numpy(host_X).to(dev)               # the batch as it arrives (read by every timed call)
        X = X0.clone()                                      # the batch the results go into
        Ld = torch.from_numpy(lens_h).to(dev)
        src, dst, flag = X0[:, :, LF0:LF0 + 1], X[:, :, LF0:LF0 + 1], X[:, :, VUV:VUV + 1]

        def composed():
            """The same result from torch operations on the same tensors: (filled (B, Tmax), flag (B, Tmax))."""
            x = X0[:, :, LF0].to(torch.float64)
            t = torch.arange(Tmax, device=dev)[None]
            L = Ld.to(torch.int64)[:, None]
            alive = t < L
            voiced = (x > 0) & alive
            below = torch.cummax(torch.where(voiced, t, -1), 1).values
            above = torch.flip(torch.cummin(torch.flip(torch.where(voiced, t, Tmax), [1]), 1).values, [1])
            has_p, has_q = below >= 0, above < Tmax
            a, b_ = torch.gather(x, 1, below.clamp(min=0)), torch.gather(x, 1, above.clamp(max=Tmax - 1))
            a, b_ = torch.where(has_p, a, b_), torch.where(has_q, b_, a)
            p, q = torch.where(has_p, below, 0), torch.where(has_q, above, L - 1)
            lin = a + (b_ - a) * ((t - p).to(torch.float64) / (q - p).to(torch.float64))
            keep = voiced | ~(has_p | has_q) | (L < 2)
            y = torch.where(keep, x, torch.where((t == 0) | (t == L - 1), a, torch.where(x <= 0, lin, x)))
            return torch.where(alive, y, 0.0).to(torch.float32), voiced.to(torch.float32)

        def composed_into():
            y, v = composed()
            X[:, :, LF0], X[:, :, VUV] = y, v

        def windows(fn, reps, n=7):
            """Milliseconds per call over `n` windows of `reps` back-to-back calls between two events, after a settled warm-up."""
            gpu_time(fn, steps=3)
            out = []
            for _ in range(n):
                a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b_.record()
                torch.cuda.synchronize()
                out.append(a.elapsed_time(b_) / reps)
            return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)), reps=reps, windows=n)

        alg_bytes = 4.0 * (3 * live + 2 * (B * Tmax - live))          # read x, write y and the flag; two zeros per pad frame
        res = dict(path="f0-config5", B=B, Tmax=Tmax, W=W, live_frames=live, unvoiced_share=unvoiced_share, hbm_peak_gbs=HBM_PEAK_GBS,
                   tile=F0H.TILE, alg_bytes=alg_bytes)
        kern = lambda: F0H.interp(src, Ld, F0H.SLINEAR, dst, flag)    # noqa: E731
        res["kernel"] = windows(kern, 200)
        res["kernel_hbm_frac"] = alg_bytes / (res["kernel"]["median_ms"] * 1e6) / HBM_PEAK_GBS
        # a yardstick: the same bytes moved by torch with no computation (a strided copy of the column, a strided fill of the flag's)
        def plain():
            dst.copy_(src)
            flag.zero_()
        res["plain_copy_and_fill"] = windows(plain, 200)
        res["plain_over_kernel"] = res["plain_copy_and_fill"]["median_ms"] / res["kernel"]["median_ms"]
        res["one_call_wall_ms"] = wall_time(lambda: PP.interp1d_batch(src, Ld, out=dst, vuv=flag), steps=200, warmup=10)
        res["composed"] = windows(composed_into, 10, n=5)
        res["composed_over_kernel"] = res["composed"]["median_ms"] / res["kernel"]["median_ms"]
        kern()
        got_y, got_v = X[:, :, LF0].clone(), X[:, :, VUV].clone()
        want_y, want_v = composed()
        res["equal_to_composed"] = bool(torch.equal(got_y, want_y) and torch.equal(got_v, want_v))
        # in place, as a user calls it (once: a second call would find the gaps filled), against the call above
        Xi = X0.clone()
        PP.interp1d_batch(Xi[:, :, LF0:LF0 + 1], Ld, out=Xi[:, :, LF0:LF0 + 1], vuv=Xi[:, :, VUV:VUV + 1])
        res["in_place_equal"] = bool(torch.equal(Xi[:, :, LF0], got_y) and torch.equal(Xi[:, :, VUV], got_v))
        rest = [c for c in range(W) if c not in (LF0, VUV)]
        res["other_columns_untouched"] = bool(torch.equal(Xi[:, :, rest], X0[:, :, rest]))
        # the reference-style loop: per utterance a copy of the column to the host, SciPy, a copy back, the flag derived separately
        try:
            from scipy import interpolate
        except ImportError:
            interpolate = None
        nloop = min(B, 32)
        Xl = X0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(nloop):
            n = int(lens_h[b])
            f = Xl[b, :n, LF0].cpu().numpy()
            flag_h = (f > 0).astype(np.float32)
            c = f.copy()
            idx = np.where(c > 0)[0]
            if len(idx):
                c[0], c[-1] = c[idx[0]], c[idx[-1]]
                idx = np.where(c > 0)[0]
                gaps = np.where(c <= 0)[0]
                if interpolate is not None:
                    c[gaps] = interpolate.interp1d(idx, c[idx], kind="slinear")(gaps)
                else:
                    c[gaps] = np.interp(gaps, idx, c[idx])
            Xl[b, :n, LF0] = torch.from_numpy(c).to(dev)
            Xl[b, :n, VUV] = torch.from_numpy(flag_h).to(dev)
        torch.cuda.synchronize()
        res["host_loop_utterances"] = nloop
        res["host_loop_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_loop_scaled_ms"] = res["host_loop_ms"] * B / nloop
        res["host_loop_uses_scipy"] = interpolate is not None
        res["host_loop_max_abs_diff"] = max(float((Xl[b, :lens_h[b], LF0] - got_y[b, :lens_h[b]]).abs().max().item()) for b in range(nloop))
        m = F0M.batch(host_X[:4, :, LF0], lens_h[:4])
        res["equal_to_model_4_utterances"] = bool(np.array_equal(m[0], got_y[:4].cpu().numpy()) and np.array_equal(m[1], got_v[:4].cpu().numpy()))
        res["note"] = ("float32 (B, 2000, 187) batch, lengths 1000 .. 2000, the lf0 column (180) in voiced runs of about 30 frames and "
                       "unvoiced runs of about 20 written as -1e10; kind slinear; the filled column goes to column 180 and the flag to "
                       "column 181 of a second tensor of the same layout, so that every timed call finds the same gaps (in place a second "
                       "call would find them filled; in_place_equal: one in-place call gives the same bits).  kernel / "
                       "plain_copy_and_fill / composed: milliseconds per call between two HIP events around `reps` back-to-back calls, "
                       "median, least and most of `windows` such windows on settled clocks.  plain_copy_and_fill: torch's strided copy_ "
                       "of the column plus zero_() of the flag's column, the bytes the kernel must move and no computation; "
                       "kernel_hbm_frac: those algorithmic bytes over the kernel's time as a fraction of 8 TB/s -- with a row stride of "
                       "748 bytes every 4-byte element costs a whole memory transaction, so this fraction says how little of the traffic "
                       "is payload, not how busy the memory system is.  composed: the same result from torch operations on the same "
                       "tensors (cummax, flip / cummin / flip, two gathers, wheres, float64 arithmetic); equal_to_composed: torch.equal.  "
                       "host_loop: per utterance the column copied to the host, SciPy's interp1d over the knots, the result and the flag "
                       "copied back, on the first utterances and scaled to the batch.  No counters were collected; no time is asserted "
                       "anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_F0_PROFILE") or os.path.join(ROOT, "profiles", "f0.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- joint: aligned pairs to the rows a joint GMM is fitted on (deltas, concatenation, zero frames out); only with --only joint ----
    if args.only and "joint" in args.only.split(","):
        from nnmnkwii_amd import _joint_hip as JH
        from nnmnkwii_amd import preprocessing as PP
        B, Tlo, Thi, D0 = (32, 1000, 2000, 60) if args.quick else (512, 1000, 2000, 60)
        rng = np.random.RandomState(1234)
        Tmax = Thi
        lens_h = rng.randint(Tlo, Thi + 1, size=B).astype(np.int32)
        host_X, host_Y = rng.randn(B, Tmax, D0).astype(np.float32), rng.randn(B, Tmax, D0).astype(np.float32)
        for b in range(B):                                   # silences of about 20 frames in both sides, about 5 % of the frames
            t = int(rng.geometric(1.0 / 380))
            while t < Tmax:
                n = 1 + int(rng.geometric(1.0 / 20))
                host_X[b, t:t + n] = 0.0
                host_Y[b, t:t + n] = 0.0
                t += n + int(rng.geometric(1.0 / 380))
        live = int(lens_h.sum())
        zero_share = float(np.mean([np.mean(np.abs(host_X[b, :lens_h[b]]).sum(1) == 0) for b in range(B)]))
        wins = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]
        X0, Y0 = torch.from_numpy(host_X).to(dev), torch.from_numpy(host_Y).to(dev)
        Ld = torch.from_numpy(lens_h).to(dev)
        xs, ys = X0[:, :, 1:], Y0[:, :, 1:]                  # column 0 dropped: slices, used where they lie
        W = 2 * (D0 - 1) * 3
        plan, offsets = JH.count(xs, ys, Ld, Ld, wins, JH.NONZERO, 1e-7, torch.float64)
        N = int(offsets[-1].item())
        out = torch.empty((live, W), dtype=torch.float64, device=dev)       # room for the LIVE mode's rows as well

        def windows(fn, reps, n=7):
            """Milliseconds per call over `n` windows of `reps` back-to-back calls between two events, after a settled warm-up."""
            gpu_time(fn, steps=3)
            res_ = []
            for _ in range(n):
                a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b_.record()
                torch.cuda.synchronize()
                res_.append(a.elapsed_time(b_) / reps)
            return dict(median_ms=float(np.median(res_)), min_ms=float(min(res_)), max_ms=float(max(res_)), reps=reps, windows=n)

        def both():
            plan.count(JH.NONZERO, 1e-7, offsets)
            plan.write(out)

        def both_live():
            plan.count(JH.LIVE, 0.0, offsets)
            plan.write(out)

        def composed():
            """The same rows from the package's delta_features and torch operations (float32 until the final cast)."""
            dx = _hip.delta_features(xs.contiguous(), wins, Ld)
            dy = _hip.delta_features(ys.contiguous(), wins, Ld)
            XY = torch.cat((dx, dy), dim=-1).reshape(-1, W)
            keep = XY.abs().sum(dim=1, dtype=torch.float64) > 1e-7
            return XY[keep]

        in_bytes = 4.0 * 2 * (D0 - 1) * live
        res = dict(path="joint-rows", B=B, Tmax=Tmax, D=D0 - 1, W=W, live_frames=live, kept_rows=N, zero_frame_share=zero_share,
                   hbm_peak_gbs=HBM_PEAK_GBS, tile=JH.TILE, write_bytes=8.0 * W * N, source_bytes=in_bytes)
        res["count"] = windows(lambda: plan.count(JH.NONZERO, 1e-7, offsets), 20)
        plan.count(JH.NONZERO, 1e-7, offsets)
        res["write"] = windows(lambda: plan.write(out), 10)
        res["count_and_write"] = windows(both, 10)
        res["live_count_and_write"] = windows(both_live, 10)
        res["live_rows"] = int(offsets[-1].item())
        res["live_count"] = windows(lambda: plan.count(JH.LIVE, 0.0, offsets), 20)
        both()
        torch.cuda.synchronize()
        res["write_hbm_frac"] = (res["write_bytes"] + in_bytes) / (res["write"]["median_ms"] * 1e6) / HBM_PEAK_GBS
        res["one_call_wall_ms"] = wall_time(lambda: PP.joint_features_batch(xs, ys, Ld, wins), steps=10, warmup=2)
        # floors: torch's plain copy of the rows the write stage must store, from float64 rows and from float32 rows (a conversion)
        src64 = torch.empty((N, W), dtype=torch.float64, device=dev).normal_(generator=gen)
        res["plain_copy_f64"] = windows(lambda: out[:N].copy_(src64), 10)
        src32 = src64.to(torch.float32)
        del src64
        res["plain_convert_f32_to_f64"] = windows(lambda: out[:N].copy_(src32), 10)
        del src32
        res["write_over_plain_copy"] = res["write"]["median_ms"] / res["plain_copy_f64"]["median_ms"]
        res["write_over_plain_convert"] = res["write"]["median_ms"] / res["plain_convert_f32_to_f64"]["median_ms"]
        del out
        torch.cuda.empty_cache()
        res["composed"] = windows(lambda: composed().to(torch.float64), 3, n=5)
        res["composed_over_count_and_write"] = res["composed"]["median_ms"] / res["count_and_write"]["median_ms"]
        got32 = PP.joint_features_batch(xs, ys, Ld, wins, dtype=torch.float32)
        want32 = composed()
        res["equal_to_composed_float32"] = bool(got32.shape == want32.shape and torch.equal(got32, want32))
        del got32, want32
        torch.cuda.empty_cache()
        # the reference-style loop: per utterance on the host, np.correlate per dimension and window, concatenate, remove the zero frames
        nloop = min(B, 8)
        t0 = time.perf_counter()
        host_rows = []
        for b in range(nloop):
            n = int(lens_h[b])
            blocks = []
            for src in (host_X, host_Y):
                x = src[b, :n, 1:]
                blocks.append(np.concatenate([np.stack([np.correlate(x[:, d], w[2], mode="same") for d in range(x.shape[1])], axis=1)
                                              for w in wins], axis=1))
            XY = np.concatenate(blocks, axis=1)
            host_rows.append(XY[np.sum(np.abs(XY), axis=1) > 1e-7])
        res["host_loop_utterances"] = nloop
        res["host_loop_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_loop_scaled_ms"] = res["host_loop_ms"] * B / nloop
        got = PP.joint_features_batch(xs[:nloop], ys[:nloop], Ld[:nloop], wins).cpu().numpy()
        host_rows = np.concatenate(host_rows, axis=0)
        res["host_loop_equal"] = bool(got.shape == host_rows.shape and np.array_equal(got, host_rows))
        res["note"] = ("float32 (B, 2000, 60) aligned pairs with column 0 dropped by slicing, lengths 1000 .. 2000, silences of about 20 "
                       "frames in both sides; static + delta + delta-delta, float64 rows of 354 columns.  count: the mask kernel plus the "
                       "one-workgroup scan; write: the third stage alone on a counted workspace; count_and_write: the three launches; "
                       "live_*: the LIVE keep rule (masks from the lengths).  Milliseconds per call between two HIP events around `reps` "
                       "back-to-back calls, median, least and most of `windows` such windows on settled clocks.  plain_copy_f64 / "
                       "plain_convert_f32_to_f64: torch's copy_ of (kept_rows, 354) float64 / float32 rows into the same output, the "
                       "stores the write stage must make with twice / once its row bytes read on top and no computation.  composed: "
                       "the same rows from two delta_features launches on contiguous copies of the slices, cat, abs-sum in float64, "
                       "boolean indexing and the cast to float64; equal_to_composed_float32: torch.equal of float32 rows.  host_loop: "
                       "per utterance np.correlate per dimension and window, concatenate, remove the zero frames, on the first "
                       "utterances, scaled to the batch.  No counters were collected; no time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_JOINT_PROFILE") or os.path.join(ROOT, "profiles", "joint.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- wave: crops to classes (encode) and classes to waveforms (decode), one launch each, at two shapes; only with --only wave ----
    if args.only and "wave" in args.only.split(","):
        from nnmnkwii_amd import _wave_hip as WH
        from nnmnkwii_amd import preprocessing as PP
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import wave_model as WM
        try:
            from scipy import signal
        except ImportError:
            signal = None
        MU, COEF = 256, 0.97
        c32 = float(np.float32(COEF))

        def windows(fn, reps, n=7):
            """Milliseconds per call over `n` windows of `reps` back-to-back calls between two events, after a settled warm-up."""
            gpu_time(fn, steps=3)
            out = []
            for _ in range(n):
                a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b_.record()
                torch.cuda.synchronize()
                out.append(a.elapsed_time(b_) / reps)
            return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)), reps=reps, windows=n)

        shapes = [(4, 20000)] if args.quick else [(32, 160000), (512, 16000)]
        res = dict(path="wave", mu=MU, coef=COEF, tile=WH.TILE, hbm_peak_gbs=HBM_PEAK_GBS, shapes=[])
        for B, Lmax in shapes:
            rng = np.random.RandomState(1234)
            lens_h = rng.randint(Lmax // 2, Lmax + 1, size=B).astype(np.int32)
            lens_h[0] = Lmax
            host_X = (np.cumsum(rng.randn(B, Lmax).astype(np.float32), 1) * 0.01 + rng.randn(B, Lmax).astype(np.float32) * 0.05)
            host_X = np.clip(host_X * np.abs(np.sin(np.arange(Lmax, dtype=np.float32) / 977.0)), -0.999, 0.999).astype(np.float32)
            live = int(lens_h.sum())
            X = torch.from_numpy(host_X).to(dev)
            Ld = torch.from_numpy(lens_h).to(dev)
            C = torch.empty((B, Lmax), dtype=torch.int16, device=dev)
            Y = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
            table = torch.from_numpy(WM.inv_mulaw_table(MU)).to(dev)
            alive = torch.arange(Lmax, device=dev)[None] < Ld[:, None]
            r = dict(B=B, Lmax=Lmax, live_samples=live)
            # ---- encode: float32 -> pre-emphasis -> mu-law -> int16 classes
            enc_bytes = 4.0 * live + 2.0 * B * Lmax
            enc = lambda: WH.encode(X, Ld, COEF, WH.QUANTIZE, MU, C)      # noqa: E731
            r["encode"] = windows(enc, 100)
            r["encode_alg_bytes"] = enc_bytes
            r["encode_hbm_frac"] = enc_bytes / (r["encode"]["median_ms"] * 1e6) / HBM_PEAK_GBS
            r["encode_one_call_wall_ms"] = wall_time(lambda: PP.wave_encode_batch(X, Ld, COEF, MU, out=C), steps=100, warmup=10)
            src8 = torch.empty(int(enc_bytes // 2), dtype=torch.uint8, device=dev).random_(0, 255)
            dst8 = torch.empty_like(src8)
            r["encode_plain_copy"] = windows(lambda: dst8.copy_(src8), 100)

            def enc_composed():
                nc = torch.tensor(-np.float32(COEF), device=dev)
                p = X.clone()
                p[:, 1:] = X[:, 1:] + nc * X[:, :-1]
                d = p.to(torch.float64)
                v = (torch.sign(d) * torch.log1p(MU * d.abs()) / math.log1p(MU) + 1.0) / 2.0 * MU
                return torch.where(alive, v.to(torch.int16), MU // 2)
            r["encode_composed"] = windows(enc_composed, 5, n=5)
            enc()
            got_c, want_c = C.clone(), enc_composed()
            differ = (got_c != want_c)
            r["encode_differs_from_composed"] = int(differ.sum().item())      # (torch's log1p against the kernel's, at bin edges)
            r["encode_max_class_diff"] = int((got_c.to(torch.int32) - want_c.to(torch.int32)).abs().max().item())
            m = WM.encode_batch(host_X[:1], lens_h[:1], COEF, WM.QUANTIZE, MU, np.int16)
            r["encode_first_utterance_differs_from_model"] = int((m != got_c[:1].cpu().numpy()).sum())
            # ---- decode: int16 classes -> table -> de-emphasis -> float32, at the segment settings
            dec_bytes = 2.0 * live + 4.0 * B * Lmax
            r["decode_alg_bytes"] = dec_bytes
            r["decode_plan_auto"] = list(WH.plan(Lmax, c32, 0))
            for name, seg in (("auto", 0), ("S16384", 16384), ("S65536", 65536), ("unsplit", Lmax)):
                if 0 < seg < Lmax or name in ("auto", "unsplit"):
                    r["decode_" + name] = windows(lambda: WH.decode(got_c, Ld, WH.QUANTIZE, MU, table, c32, seg, Y), 100 if name != "unsplit" else 20)
                    r["decode_" + name]["nseg"] = WH.plan(Lmax, c32, seg)[2]
            r["decode_hbm_frac_auto"] = dec_bytes / (r["decode_auto"]["median_ms"] * 1e6) / HBM_PEAK_GBS
            r["decode_one_call_wall_ms"] = wall_time(lambda: PP.wave_decode_batch(got_c, Ld, MU, COEF, out=Y), steps=100, warmup=10)
            src8 = torch.empty(int(dec_bytes // 2), dtype=torch.uint8, device=dev).random_(0, 255)
            dst8 = torch.empty_like(src8)
            r["decode_plain_copy"] = windows(lambda: dst8.copy_(src8), 100)

            def dec_composed():
                y = torch.where(alive, table[got_c.to(torch.int64).clamp(0, MU)].to(torch.float64), 0.0)
                d, cd = 1, c32
                while d < Lmax and cd != 0.0:                 # a log-step scan: y[n] += c^d y[n - d]
                    y = torch.cat([y[:, :d], y[:, d:] + cd * y[:, :-d]], 1)
                    d, cd = 2 * d, cd * cd
                return torch.where(alive, y, 0.0).to(torch.float32)
            r["decode_composed"] = windows(dec_composed, 3, n=5)
            WH.decode(got_c, Ld, WH.QUANTIZE, MU, table, c32, 0, Y)
            got_y = Y.clone()
            r["decode_max_abs_diff_from_composed"] = float((got_y - dec_composed()).abs().max().item())
            WH.decode(got_c, Ld, WH.QUANTIZE, MU, table, c32, Lmax, Y)
            r["decode_max_abs_diff_auto_from_unsplit"] = float((got_y - Y).abs().max().item())
            m = WM.decode_batch(got_c[:1].cpu().numpy(), lens_h[:1], WM.QUANTIZE, MU, c32, 0, np.float32)
            r["decode_first_utterance_equals_model"] = bool(np.array_equal(m.view(np.int32), got_y[:1].cpu().numpy().view(np.int32)))
            # ---- the reference-style loop: per utterance a copy to the host, the reference's expressions, a copy back
            nloop = min(B, 8)
            if signal is not None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b in range(nloop):
                    n = int(lens_h[b])
                    x = X[b, :n].cpu().numpy()
                    p = signal.lfilter(np.array([1.0, -COEF], x.dtype), np.array([1.0], x.dtype), x)
                    yq = np.sign(p) * np.log1p(MU * np.abs(p)) / np.log1p(MU)
                    C[b, :n] = torch.from_numpy(((yq + 1) / 2 * MU).astype(int).astype(np.int16)).to(dev)
                torch.cuda.synchronize()
                r["encode_host_loop_scaled_ms"] = (time.perf_counter() - t0) * 1e3 * B / nloop
                t0 = time.perf_counter()
                for b in range(nloop):
                    n = int(lens_h[b])
                    q = got_c[b, :n].cpu().numpy()
                    yf = 2 * q.astype(np.float32) / MU - 1
                    w = np.sign(yf) * (1.0 / MU) * ((1.0 + MU) ** np.abs(yf) - 1.0)
                    Y[b, :n] = torch.from_numpy(signal.lfilter(np.array([1.0], w.dtype), np.array([1.0, -COEF], w.dtype), w)).to(dev)
                torch.cuda.synchronize()
                r["decode_host_loop_scaled_ms"] = (time.perf_counter() - t0) * 1e3 * B / nloop
                r["host_loop_utterances"] = nloop
                r["decode_host_loop_max_abs_diff"] = max(float((Y[b, :lens_h[b]] - got_y[b, :lens_h[b]]).abs().max().item()) for b in range(nloop))
            res["shapes"].append(r)
        res["note"] = ("float32 waveforms, lengths Lmax / 2 .. Lmax, mu 256, coef 0.97.  encode: pre-emphasis -> mu-law -> int16 classes in one "
                       "nnmk_wave_encode launch; decode: int16 classes -> table -> de-emphasis -> float32 in one nnmk_wave_decode launch, at "
                       "segment 0 (the built-in choice), 16384, 65536 and Lmax (one workgroup per utterance).  Milliseconds per call between two "
                       "HIP events around `reps` back-to-back calls: median, least and most of `windows` such windows on settled clocks.  "
                       "plain_copy: torch's copy_ of a uint8 buffer of half the launch's algorithmic bytes (so it moves the same bytes and "
                       "computes nothing); hbm_frac: algorithmic bytes over time as a fraction of 8 TB/s.  composed: the same result from "
                       "torch operations (encode: shifted multiply-add, float64 log1p, truncation; decode: a gather and a log-step scan of "
                       "torch.cat passes in float64).  host_loop: per utterance a copy to the host, the reference's numpy expressions and "
                       "scipy.signal.lfilter, a copy back, on the first utterances and scaled to the batch.  No counters were collected; "
                       "no time is asserted anywhere")
        emit(**res)
        if not args.quick:
            out_path = os.environ.get("NNMNKWII_WAVE_PROFILE") or os.path.join(ROOT, "profiles", "wave.json")
            with open(out_path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")

    # ---- c3: unit-variance autograd fwd+bwd ----
    if want("c3"):
        B, T, D = 64, 500, 180
        R = torch.from_numpy(G.unit_variance_mlpg_matrix(WINDOWS, T)).to(dev)
        means = torch.rand(B, T, D, device=dev, requires_grad=True)
        target = torch.rand(B, T, D // 3, device=dev)
        loss_fn = torch.nn.MSELoss()

        def step():
            means.grad = None
            y = AF.unit_variance_mlpg(R, means)
            loss_fn(y, target).backward()

        ms = gpu_time(step)
        nwall = 200 if args.quick else 1000
        ms_wall = wall_time(step, steps=nwall)

        def step_plain():      # the same loop with a trivial node in place of MLPG: what the framework itself costs per step
            means.grad = None
            loss_fn(means[..., :D // 3] * 1.0, target).backward()

        ms_wall_plain = wall_time(step_plain, steps=nwall)
        by = 1920.0 * B * T    # 960 B/frame forward + 960 B/frame backward
        # the same training step captured once into a HIP graph and replayed (eager mode is host-bound: a dozen
        # framework launches of a few microseconds each around two short kernels)
        ms_graph = None
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            means.grad = None
            with torch.cuda.graph(graph):
                y_ = AF.unit_variance_mlpg(R, means)
                loss_ = loss_fn(y_, target)
                loss_.backward()
            ms_graph = gpu_time(graph.replay, steps=20)
        except Exception as e:  # noqa: BLE001
            ms_graph = "capture failed: %s" % str(e)[:120]
        # the two kernels alone (unit variances, float32), wave-per-system vs strip
        md = means.detach()
        god = torch.rand(B, T, D // 3, device=dev)
        for name, algo in (("wave", 2), ("strip", 3), ("fir", 7)):
            kf = gpu_time(lambda: _hip.forward(md, None, WINDOWS, algo=algo, want_status=False), steps=20)
            kb = gpu_time(lambda: _hip.backward(None, god, WINDOWS, D, out_dtype=torch.float32, algo=algo, want_status=False), steps=20)
            emit(path="c3-kernels-" + name, ms_forward=kf, ms_backward=kb, ms=kf + kb, alg_bytes=by, GBps=by / (kf + kb) / 1e6)
        # reference CPU form: dense R @ means on torch CPU (autograd/_impl/mlpg.py:138,158), 1 thread
        torch.set_num_threads(1)
        Rc, mc = R.cpu(), means.detach().cpu().requires_grad_()
        tc = target.cpu()
        t0 = time.perf_counter()
        nrep = 1 if args.quick else 3
        for _ in range(nrep):
            mc.grad = None
            rm = mc.view(B, T, 3, -1).transpose(1, 2).contiguous().view(B, -1, D // 3)
            loss_fn(torch.matmul(Rc, rm), tc).backward()
        cpu_s = (time.perf_counter() - t0) / nrep
        # the same step as ONE fused launch (autograd.unit_variance_mlpg_mse_loss -> mlpg_hip_unit_mse_step)
        def step_fused():
            means.grad = None
            AF.unit_variance_mlpg_mse_loss(R, means, target).backward()

        ms_fused = gpu_time(step_fused, steps=20)
        ms_fused_wall = wall_time(step_fused, steps=nwall)
        ms_fused_kernel = gpu_time(lambda: _hip.unit_mse_step(md, target, WINDOWS), steps=20)
        full = torch.full((B,), T, dtype=torch.int32, device=dev)     # (a lengths vector keeps the call on the one-launch kernel)
        ms_one_launch = gpu_time(lambda: _hip.unit_mse_step(md, target, WINDOWS, lengths=full), steps=20)
        ms_fused_graph = None
        try:
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            means.grad = None
            side2 = torch.cuda.Stream()
            side2.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side2):
                for _ in range(3):
                    step_fused()
            torch.cuda.current_stream().wait_stream(side2)
            torch.cuda.synchronize()
            means.grad = None
            with torch.cuda.graph(g2, stream=side2):   # (the stream that was warmed up: the step's workspace is per stream and is
                AF.unit_variance_mlpg_mse_loss(R, means, target).backward()     # never created inside a capture, _hip._mse_workspace)
            ms_fused_graph = gpu_time(g2.replay, steps=20)
        except Exception as e:  # noqa: BLE001
            ms_fused_graph = "capture failed: %s" % str(e)[:120]
        emit(path="c3-fused-unit-mse-step", ms=ms_fused_kernel, ms_one_launch_kernel=ms_one_launch, ms_autograd_eager=ms_fused,
             ms_autograd_eager_wall_loop=ms_fused_wall, ms_hip_graph_replay=ms_fused_graph,
             frames_per_s=B * T / ms_fused_kernel * 1e3, alg_bytes=by + 4.0 * 60 * B * T, GBps=(by + 4.0 * 60 * B * T) / ms_fused_kernel / 1e6,
             note="ms = one mlpg_hip_unit_mse_step call (float32 without lengths: the FIR form, two launches, nothing allocated; "
                  "ms_one_launch_kernel: the wave-per-system kernel that takes the call when lengths are given): forward + MSE loss + backward of config 3; "
                  "ms_autograd_eager / ms_hip_graph_replay = the same through autograd.unit_variance_mlpg_mse_loss(...).backward(); "
                  "ms_autograd_eager_wall_loop: wall clock per step of %d back-to-back eager steps, one synchronize at the end" % nwall)
        emit(path="c3-unit-variance-autograd-fwd+bwd", ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by,
             GBps=by / ms / 1e6, ms_wall_loop=ms_wall, ms_wall_loop_plain_torch_ops_no_mlpg_node=ms_wall_plain, ms_hip_graph_replay=ms_graph,
             note="ms: median HIP-event pair around ONE eager step (host-bound: the pair reads the host's issue time of a step that starts on an idle "
                  "device); ms_wall_loop: wall clock per step of %d back-to-back eager steps with one synchronize at the end -- how the reference "
                  "times this loop (perf/autograd_mlpg_perf.py:56-86); ..._plain_torch_ops_no_mlpg_node: the same loop with `means[..., :60] * 1.0` "
                  "in place of the MLPG node" % nwall,
             GBps_hip_graph_replay=(by / ms_graph / 1e6 if isinstance(ms_graph, float) else None),
             cpu_dense_matmul_1thread_frames_per_s=B * T / cpu_s)

    # ---- c3m: generic autograd.mlpg fwd+bwd (one utterance, like the reference's MLPG) ----
    if want("c3m"):
        T, D = 500, 180
        m1 = torch.rand(T, D, device=dev, requires_grad=True)
        v1 = torch.rand(T, D, device=dev) + 0.1
        tg = torch.rand(T, D // 3, device=dev)
        AF._mlpg.CHECK_STATUS = False

        def step1():
            m1.grad = None
            torch.nn.MSELoss()(AF.mlpg(m1, v1, WINDOWS), tg).backward()

        ms = gpu_time(step1)
        AF._mlpg.CHECK_STATUS = True
        t0 = time.perf_counter()
        O.mlpg(m1.detach().cpu().numpy(), v1.cpu().numpy(), WINDOWS)
        cpu_fwd = time.perf_counter() - t0
        emit(path="c3m-autograd.mlpg-fwd+bwd-1utt", ms=ms, frames_per_s=T / ms * 1e3,
             cpu_oracle_forward_only_frames_per_s=T / cpu_fwd,
             note="reference backward is O(T^2) dense solve_banded: 12.7 ms per static dim at T=500 (SURVEY 6)")

    # ---- c4: DTW (c4q: the kernel on one GPU's share only -- the per-rank leg of bench.py --gpus N) ----
    if want("c4") or want("c4q"):
        share_only = want("c4q") and not want("c4")
        N = 32 if args.quick else 128
        rng = np.random.RandomState(1234)
        Tx = Ty = 900
        X = np.zeros((N, Tx, 25))
        Y = np.zeros((N, Ty, 25))
        for n in range(N):
            a, b = rng.randint(700, 901, size=2)
            X[n, :a] = np.cumsum(rng.randn(a, 25), 0) * 0.1
            Y[n, :b] = np.cumsum(rng.randn(b, 25), 0) * 0.1
        Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
        lenx, leny = _hip.trim_lengths(Xd), _hip.trim_lengths(Yd)
        ms = gpu_time(lambda: _hip.fastdtw_l2(Xd, Yd, lenx, leny, 1))
        pi, pj, pl, cost = _hip.fastdtw_l2(Xd, Yd, lenx, leny, 1)
        plen = pl.cpu().numpy()
        by = float(((lenx + leny).sum().item()) * 25 * 8 + 8 * plen.sum())
        ncpu = 2 if share_only else (8 if args.quick else 32)
        t0 = time.perf_counter()
        for n in range(ncpu):
            OD.fastdtw(X[n, :int(lenx[n])], Y[n, :int(leny[n])], 1)
        cpu_s = (time.perf_counter() - t0) / ncpu
        ms_full = None if share_only else gpu_time(lambda: DTWAligner().transform((X, Y)), steps=8, warmup=3)
        # DP cells over all pyramid levels (mean of 8 pairs): the kernel is latency-bound, cells/s is its work rate
        cells_per_pair = float(np.mean([fastdtw_window_cells(X[n, :int(lenx[n])], Y[n, :int(leny[n])], 1) for n in range(8)]))
        if not args.quick and not share_only:
            # all 1024 pairs of config 4 on one GPU (the pairs repeated 8 times)
            X8, Y8 = Xd.repeat(8, 1, 1).contiguous(), Yd.repeat(8, 1, 1).contiguous()
            lx8, ly8 = lenx.repeat(8).contiguous(), leny.repeat(8).contiguous()
            ms8 = gpu_time(lambda: _hip.fastdtw_l2(X8, Y8, lx8, ly8, 1), steps=5)
            emit(path="c4-fastdtw-kernel-1024pairs", pairs=8 * N, ms=ms8, pairs_per_s=8 * N / ms8 * 1e3, alg_bytes=8 * by,
                 GBps=8 * by / ms8 / 1e6, dp_cells_per_pair=cells_per_pair, dp_cells_per_s=cells_per_pair * 8 * N / ms8 * 1e3)
            del X8, Y8
            # the same 1024 pairs from HOST memory through mlpg_hip_fastdtw_host (device-side trim, chunks of pairs
            # on two streams, PCIe-inclusive wall clock), pageable and pinned inputs
            host_legs = (not args.only) or "c4h" in args.only.split(",")
            Xh, Yh = (np.tile(X, (8, 1, 1)), np.tile(Y, (8, 1, 1))) if host_legs else (None, None)
            for nm, (a_, b_) in () if not host_legs else (("pageable", (Xh, Yh)), ("pinned", (_hip.pinned_empty(Xh.shape), _hip.pinned_empty(Yh.shape)))):
                if nm == "pinned":
                    a_[...] = Xh
                    b_[...] = Yh
                _hip.fastdtw_host(a_, b_, 1)
                t0 = time.perf_counter()
                for _ in range(3):
                    _hip.fastdtw_host(a_, b_, 1)
                wall = (time.perf_counter() - t0) / 3 * 1e3
                emit(path="c4h-fastdtw-host-1024pairs-" + nm, pairs=8 * N, ms=wall, pairs_per_s=8 * N / wall * 1e3,
                     host_bytes=float(Xh.nbytes + Yh.nbytes))
        emit(path="c4-fastdtw-kernel", pairs=N, ms=ms, pairs_per_s=N / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6,
             dp_cells_per_pair=cells_per_pair, dp_cells_per_s=cells_per_pair * N / ms * 1e3,
             cpu_oracle_c_pairs_per_s=1.0 / cpu_s, transform_numpy_to_numpy_ms=ms_full,
             note="paths bit-exact vs the oracle's restatement of third-party fastdtw (parity unpinned: the package is absent)")

    # ---- ms: modulation-spectrum smoothing of the config-2 output batch (the step after MLPG) ----
    if want("ms"):
        B, T, sd, n = 256, 1000, 60, 4096
        x = torch.randn(B, T, sd, dtype=torch.float64, device=dev, generator=gen)
        ms = gpu_time(lambda: _hip.modspec_smoothing(x, n, 500, True), steps=5)
        by = 16.0 * B * T * sd                      # read + write the trajectory once
        # FFT arithmetic: 2 transforms x 5 n log2 n flops per column
        fl = 2 * 5.0 * n * 12 * B * sd
        xc = x[:4].cpu().numpy()
        t0 = time.perf_counter()
        for b_ in range(4):
            s_ = np.fft.rfft(xc[b_], n=n, axis=0)
            a_ = np.abs(s_)
            a_[500:] = 1.0
            np.fft.irfft(a_ * np.exp(1j * np.angle(s_)), n=n, axis=0)[:T]
        cpu_s = (time.perf_counter() - t0) / 4
        emit(path="ms-modspec_smoothing-n4096", ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6,
             fft_GFLOPs=fl / ms / 1e6, cpu_numpy_fft_frames_per_s=T / cpu_s)
        ms2 = gpu_time(lambda: _hip.modspec(x, n), steps=5)
        emit(path="ms-modspec-n4096", ms=ms2, frames_per_s=B * T / ms2 * 1e3)
        # a DFT length outside the in-LDS FFT: the direct transform (modspec_dft.hip)
        nd = 5000
        ms3 = gpu_time(lambda: _hip.modspec_smoothing(x, nd, 600, True), steps=3, warmup=1)
        t0 = time.perf_counter()
        for b_ in range(2):
            s_ = np.fft.rfft(xc[b_], n=nd, axis=0)
            np.fft.irfft(np.abs(s_) * np.exp(1j * np.angle(s_)), n=nd, axis=0)[:T]
        cpu3 = (time.perf_counter() - t0) / 2
        emit(path="ms-modspec_smoothing-n5000-direct", ms=ms3, frames_per_s=B * T / ms3 * 1e3, alg_bytes=by, GBps=by / ms3 / 1e6,
             cpu_numpy_fft_frames_per_s=T / cpu3)
        del x

    # ---- c5: Merlin-style multi-stream (c5q: the one-call form only) ----
    if want("c5") or want("c5q"):
        B, T = (128 if args.quick else 512), 2000
        tot_ms, tot_by = 0.0, sum(56.0 * sd_ * B * T for sd_ in (60, 1, 5))
        tot_by0, tot_by = tot_by, 0.0
        for name, sd in (("mgc", 60), ("lf0", 1), ("bap", 5)) if want("c5") else ():
            m = torch.randn(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen)
            v = torch.rand(B, T, 3 * sd, dtype=torch.float64, device=dev, generator=gen) + 0.1
            ms = gpu_time(lambda: _hip.forward(m, v, WINDOWS, want_status=False), steps=5)
            by = 56.0 * sd * B * T
            emit(path="c5-" + name, batch=B, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by, GBps=by / ms / 1e6)
            tot_ms += ms
            tot_by += by
            del m, v
        if want("c5"):
            emit(path="c5-all-streams", batch=B, ms=tot_ms, frames_per_s=B * T / tot_ms * 1e3, alg_bytes=tot_by,
                 GBps=tot_by / tot_ms / 1e6)
        tot_by = tot_by0
        # the same three streams consumed in place from ONE (B, T, 198) batch: mlpg_hip_forward_streams
        m = torch.randn(B, T, 198, dtype=torch.float64, device=dev, generator=gen)
        v = torch.rand(B, T, 198, dtype=torch.float64, device=dev, generator=gen) + 0.1
        streams = [(0, 60, WINDOWS), (180, 1, WINDOWS), (183, 5, WINDOWS)]
        ms = gpu_time(lambda: _hip.forward_streams(m, v, streams, want_status=False), steps=5)
        emit(path="c5-forward_streams-one-call", batch=B, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=tot_by,
             GBps=tot_by / ms / 1e6)
        del v
        # the same call with GLOBAL (D,) variances -- what a Merlin-style pipeline passes (util/files.py:90-115: one variance
        # vector per stream for the whole corpus): 32 B per (frame, dim); the streams merged on the constant-coefficient kernel
        vg5 = torch.rand(198, dtype=torch.float64, device=dev, generator=gen) + 0.1
        by_g = 32.0 * 66 * B * T
        ms = gpu_time(lambda: _hip.forward_streams(m, vg5, streams, want_status=False), steps=5)
        n0 = [int(_hip.lib().mlpg_hip_launch_count(k)) for k in range(9)]
        _hip.forward_streams(m, vg5, streams, want_status=False)
        n1 = [int(_hip.lib().mlpg_hip_launch_count(k)) for k in range(9)]
        emit(path="c5g-forward_streams-one-call-global-variances", batch=B, ms=ms, frames_per_s=B * T / ms * 1e3, alg_bytes=by_g,
             GBps=by_g / ms / 1e6, launches={k: b - a for k, (a, b) in enumerate(zip(n0, n1)) if b != a},
             note="launches: kernel family -> launches of one call (8 = merged constant-coefficient, 1 = wave-per-system for the 2 dims left over)")
        ms_sep = 0.0
        for in_col, sd_, _w in streams:       # the three streams as three calls on dense tensors, for comparison
            md = m[:, :, in_col:in_col + 3 * sd_].contiguous()
            vd = vg5[in_col:in_col + 3 * sd_].contiguous()
            ms_sep += gpu_time(lambda: _hip.forward(md, vd, WINDOWS, want_status=False), steps=5)
            del md
        emit(path="c5g-three-calls-global-variances", batch=B, ms=ms_sep, frames_per_s=B * T / ms_sep * 1e3, alg_bytes=by_g, GBps=by_g / ms_sep / 1e6,
             note="dense copies of the three streams' columns, one mlpg_hip_forward each")
        # ... and as three calls IN PLACE (one stream per forward_streams call: nothing to merge) -- what the one-call form competes with
        ms_inplace = sum(gpu_time(lambda: _hip.forward_streams(m, vg5, [st_]), steps=5) for st_ in streams)
        emit(path="c5g-three-calls-in-place-global-variances", batch=B, ms=ms_inplace, frames_per_s=B * T / ms_inplace * 1e3, alg_bytes=by_g,
             GBps=by_g / ms_inplace / 1e6)
        del m


if __name__ == "__main__":
    main()
