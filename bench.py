#!/usr/bin/env python
"""bench.py -- MLPG frames/sec on BASELINE.json configs[1] (per GPU: 256 utterances
x T=1000 x 60-dim mgc static+delta+delta-delta = 180 columns, float64, per-frame
variances, standard 3 windows), weak-scaled over N GPUs (one process per GPU,
independent shards, no data-path collective).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

With --gpus N > 1 and no WORLD_SIZE in the environment the script launches its own N ranks (it
re-executes itself under torch.distributed.run on 127.0.0.1) and fails loudly if the node has
fewer than N GPUs.  A "step" is one pass of the hot path (one mlpg_hip_forward launch through the
C ABI) over the rank's resident batch.  Rank 0 prints ONE JSON line.

A plain run does what the headline figure needs: it generates the inputs, runs the preconditioning
leg and the W warm-up steps, times exactly K steps, checks their status array, writes the outputs
of the last timed step if --dump-outputs is given, and prints the line.  --full adds everything
else: the in-run copy-rate peak, the cold protocol, the steady and repeat regions, the oracle
parity checks, the live PMC traffic pass, `secondary`, `cpu_baseline` and (N > 1) the in-run
single-GPU leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
DUMP_LIMIT = 48 << 20          # bytes of trajectories --dump-outputs writes at most
WINDOWS = [
    (0, 0, np.array([1.0])),
    (1, 1, np.array([-0.5, 0.0, 0.5])),
    (1, 1, np.array([1.0, -2.0, 1.0])),
]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="utterances per GPU")
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--static-dim", type=int, default=60)
    ap.add_argument("--algo", type=int, default=0, help="0 auto, 1 generic, 2 wave-per-system, 3 strip, 5 constant-coefficient (global / unit variances)")
    ap.add_argument("--dry-run-cpu", action="store_true",
                    help="plumbing test only (no GPU, gloo): the launch / barrier / reduction / JSON path with a no-op step")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-check", action="store_true", help="profiling/ablation only: skip status and parity checks")
    ap.add_argument("--gather", action="store_true", help="also time an RCCL all-gather of the outputs (reported separately)")
    ap.add_argument("--no-traffic", action="store_true", help="skip the live PMC pass (two rocprofv3 child runs, ~40 s)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the `secondary` object (the other BASELINE configs and kernel variants, timed after the metric)")
    ap.add_argument("--precondition", type=int, default=200,
                    help="steps of the same workload run BEFORE the --warmup steps and the timed region (event-timed, reported as "
                         "roofline.kernel_ms_steady): the device's clocks take tens of milliseconds of THIS kernel to settle -- the "
                         "copy-rate measurement in front of them does not do it -- and a batch job runs thousands of steps; 0: none")
    ap.add_argument("--regions", type=int, default=9,
                    help="extra timed regions of --steps launches after the official one; their median is reported beside it")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure (copy-rate peak, cold protocol, steady and "
                         "repeat regions, oracle parity, live PMC traffic, `secondary`, cpu_baseline, N > 1: the single-GPU leg); "
                         "the --no-* options and --regions select among these")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float64; rank 0's "
                         "shard; a fixed, seeded sample of whole utterances where the batch's output exceeds %d MiB)" % (DUMP_LIMIT >> 20))
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.dry_run_cpu:
        ap.error("--dump-outputs needs a GPU run (a --dry-run-cpu step computes nothing)")
    return args


def dump_outputs(d, out, status):
    """What the timed path returned in its last step: `mlpg_out` (the trajectories, (k, T, static_dim) float64, utterances
    `mlpg_out_utterances` of the batch) and `status` (one int32 per system, as float64).  The inputs are seeded, so two
    builds run with the same arguments can be compared array for array."""
    import torch
    os.makedirs(d, exist_ok=True)
    B = out.shape[0]
    per = out[0].numel() * 8                    # bytes of one utterance's trajectories, written as float64
    k = max(1, min(B, DUMP_LIMIT // max(per, 1)))
    idx = np.arange(B) if k == B else np.sort(np.random.RandomState(0).choice(B, k, replace=False))
    y = out.index_select(0, torch.from_numpy(idx).to(out.device)).to(torch.float64).cpu().numpy()
    if y.nbytes > DUMP_LIMIT:          # one utterance alone is larger than the limit: its leading frames
        y = y[:, :max(1, DUMP_LIMIT // (y.shape[2] * 8))]
    np.save(os.path.join(d, "mlpg_out.npy"), y)
    np.save(os.path.join(d, "mlpg_out_utterances.npy"), idx.astype(np.float64))
    if status is not None:
        np.save(os.path.join(d, "status.npy"), status.cpu().numpy().astype(np.float64))


_REF_WORKER = r"""
import sys, time, numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import ref
G = ref.load()
n, T, D, seed = (int(a) for a in sys.argv[2:6])
W = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]
rng = np.random.RandomState(seed)
utts = [(rng.randn(T, D), rng.rand(T, D) + 0.1) for _ in range(n)]      # distinct utterances
G.mlpg(*utts[0], W)
sys.stdin.readline()              # start gun
t0 = time.perf_counter()
for m, v in utts:
    G.mlpg(m, v, W)
print(time.perf_counter() - t0)
"""


def _reference_pool(n_per_proc, T, D, cores, timeout):
    """The reference's mlpg on `cores` independent processes (it has no threading of its own).
    Plain subprocesses with a hard timeout: this leg must never be able to hang the bench."""
    import subprocess
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, "-c", _REF_WORKER, ROOT, str(n_per_proc), str(T), str(D), str(100 + i)],
                              stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, text=True)
             for i in range(cores)]
    try:
        time.sleep(min(15.0, 2.0 + 0.1 * cores))          # let every process import and generate its utterances
        t0 = time.perf_counter()
        for p in procs:
            p.stdin.write("go\n")
            p.stdin.flush()
        outs = [p.communicate(timeout=timeout)[0] for p in procs]
        wall = time.perf_counter() - t0
        busy = [float(o.strip().splitlines()[-1]) for o in outs]
        return cores * n_per_proc * T / max(max(busy), 1e-9), wall
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()


def cpu_baseline(T, D, seconds):
    """CPU path timed on the GPU box's host, bounded sample of the same workload.

    kind "reference": the reference's OWN numpy/bandmat/Cython code (oracle/_ref: its sources
    compiled unmodified by oracle/build_ref_so.sh), called the way the reference batches -- a
    Python loop of paramgen.mlpg over utterances (util/__init__.py:44-66) -- on ONE core (the
    reference is single-threaded).  The sample is a pool of DISTINCT utterances (5.8 MB each,
    cycled if the time budget outlasts the pool), so the working set does not sit in the core's
    cache.  kind "port": the C restatement oracle/mlpg_oracle.c, if the compiled reference is absent."""
    from oracle import mlpg as O
    from oracle import ref
    O.build()
    rng = np.random.RandomState(1234)
    if ref.available():
        G = ref.load()
        pool = [(rng.randn(T, D), rng.rand(T, D) + 0.1) for _ in range(64)]
        y = G.mlpg(*pool[0], WINDOWS)
        assert np.array_equal(y, O.mlpg(*pool[0], WINDOWS)), "C oracle and compiled reference disagree"
        t0 = time.perf_counter()
        G.mlpg(*pool[1], WINDOWS)
        per = time.perf_counter() - t0
        n = int(max(8, min(4096, seconds / max(per, 1e-6))))
        t0 = time.perf_counter()
        for k in range(n):
            G.mlpg(*pool[k % len(pool)], WINDOWS)
        dt = time.perf_counter() - t0
        res = {
            "value": n * T / dt, "unit": "frames/s", "cores": 1, "kind": "reference",
            "sample": "%d calls of the reference's own paramgen.mlpg (numpy + bandmat Cython, compiled unmodified into "
                      "oracle/_ref) over a pool of %d distinct utterances of T=%d x D=%d float64, Python loop over "
                      "utterances, %.1f s on 1 core of %d" % (n, len(pool), T, D, dt, os.cpu_count()),
        }
        # the same on many cores (independent processes; the reference itself has no threading)
        try:
            cores = max(1, min(os.cpu_count() or 1, 64))
            per_proc = max(2, min(24, int(0.2 * n)))
            rate, wall = _reference_pool(per_proc, T, D, cores, timeout=max(60.0, 6 * seconds))
            res["pool"] = {"value": rate, "unit": "frames/s", "cores": cores,
                           "sample": "%d processes x %d distinct utterances each, %.1f s wall" % (cores, per_proc, wall)}
        except Exception as e:  # the single-core figure is the reported baseline
            res["pool"] = {"error": str(e)[:200]}
        return res
    m = rng.randn(16, T, D)
    v = rng.rand(16, T, D) + 0.1
    t0 = time.perf_counter()
    O.mlpg_batch(m[:4], v[:4], WINDOWS)
    per4 = time.perf_counter() - t0
    n = int(max(16, min(4096, seconds / max(per4 / 4, 1e-6))))
    n -= n % 16
    reps = n // 16
    t0 = time.perf_counter()
    for _ in range(reps):
        O.mlpg_batch(m, v, WINDOWS)
    dt = time.perf_counter() - t0
    return {
        "value": n * T / dt,
        "unit": "frames/s",
        "cores": 1,
        "kind": "port",
        "sample": "%d calls over 16 distinct utterances of T=%d x D=%d float64 through oracle/mlpg_oracle.c (C restatement "
                  "of paramgen.mlpg, bit-exact vs the reference), %.1f s on 1 core of %d" % (n, T, D, dt, os.cpu_count()),
    }


def live_traffic(B, T, sd, algo, timeout_s=90.0):
    """HBM bytes per launch of the dominant kernel, measured NOW: two child runs of this script (the metric's workload
    only, 5 launches) under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` -- counters in their own
    passes, as the MI355X guide prescribes -- read back from the rocpd database.  gfx950: FETCH_SIZE counts half of a
    16 B/lane streaming read, hence 2 x FETCH_SIZE + WRITE_SIZE (both in KiB).  Returns (bytes or None, note)."""
    import glob
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if prof is None:
        return None, "rocprofv3 not found"
    kib = {}
    t0 = time.perf_counter()
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
        try:
            cmd = [prof, "--kernel-trace", "--pmc", counter, "-d", d, "-o", "run", "--", sys.executable,   # a plain run (no --full)
                   os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "1", "--algo", str(algo), "--batch", str(B),
                   "--frames", str(T), "--static-dim", str(sd)]
            env = dict(os.environ, TMPDIR="/tmp")
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
                env.pop(k, None)
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout_s)
            dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
            if r.returncode != 0 or not dbs:
                return None, "rocprofv3 --pmc %s failed (rc %d)" % (counter, r.returncode)
            cur = sqlite3.connect(dbs[0]).cursor()
            rows = cur.execute("select kernel_name, avg(value), count(*) from counters_collection where counter_name = ? "
                               "group by kernel_name order by sum(value) desc", (counter,)).fetchall()
            rows = [x for x in rows if "strip_kernel" in x[0] or "pipe_kernel" in x[0] or "wave_kernel" in x[0] or "generic" in x[0]]
            if not rows:
                return None, "no %s rows for the MLPG kernel" % counter
            kib[counter] = (float(rows[0][1]), int(rows[0][2]), rows[0][0])
        except (subprocess.TimeoutExpired, OSError, sqlite3.Error) as e:
            return None, "%s pass: %s" % (counter, type(e).__name__)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    nbytes = (2.0 * kib["FETCH_SIZE"][0] + kib["WRITE_SIZE"][0]) * 1024.0
    return nbytes, ("measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate child passes of this "
                    "workload, mean of %d dispatches of %s, %.0f s): 2 x %.1f + %.1f KiB"
                    % (kib["FETCH_SIZE"][1], kib["FETCH_SIZE"][2].split("(")[0].replace("void ", ""), time.perf_counter() - t0,
                       kib["FETCH_SIZE"][0], kib["WRITE_SIZE"][0]))


def measured_traffic(B, T, sd, algo):
    """HBM bytes per launch of the dominant kernel from the committed PMC profile (profiles/traffic.json),
    if it was taken on this exact workload and kernel: the fall-back when the live pass (live_traffic) is not possible."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            t = json.load(f)
        w = t["workload"]
        if (w["batch_per_gpu"], w["frames"], w["static_dim"]) == (B, T, sd):
            if algo in t.get("algos", (0, 3)):
                return float(t["traffic_bytes_per_launch"])
            if algo == t.get("other", {}).get("algo"):
                return float(t["other"]["traffic_bytes_per_launch"])
    except (OSError, KeyError, ValueError):
        pass
    return None


def collect_secondary(rank, world, local_rank, copy_gbs, dry=False):
    """The other BASELINE configs and kernel variants, one entry per path: ms (HIP events on the launch stream, median),
    the rate in the path's own unit, algorithmic bytes and their fraction of the 8 TB/s peak (`frac`) and of
    the copy rate measured in this run (`frac_of_measured`).  N = 1: every path on rank 0.  N > 1: the per-GPU shares of
    configs 4 and 5 on every rank, whole-job rates from the slowest rank."""
    import torch
    import torch.distributed as dist
    from tools import bench_paths
    lines = []
    keys = "litq,c2b,c2g,c2t,c3,c4,c5" if world == 1 else "c4q,c5q"
    if dry:
        # plumbing run (no GPU): stand-in entries with a rank-dependent time, so that the reduction below -- slowest rank, whole-job
        # rates -- has run once on CPU (gloo) before an 8-GPU node sees it
        lines = [{"path": "c4-fastdtw-kernel", "ms": 1.0 + rank, "pairs_per_s": 128e3 / (1.0 + rank), "GBps": 1.0, "roofline_frac": 1.0 / 8000},
                 {"path": "c5-forward_streams-one-call", "ms": 2.0 * (1.0 + rank), "frames_per_s": 512 * 2000e3 / (2.0 * (1.0 + rank)), "GBps": 2.0,
                  "roofline_frac": 2.0 / 8000}]
    else:
        try:
            bench_paths.run(only=keys, quick=False, sink=lines, device_index=local_rank)
        except Exception as e:  # noqa: BLE001 -- the metric line must still be printed
            lines.append({"path": "error", "error": "%s: %s" % (type(e).__name__, str(e)[:300])})
    out = {}
    for ln in lines:
        name = ln.pop("path")
        if "roofline_frac" in ln:
            ln["frac"] = ln.pop("roofline_frac")
            if copy_gbs:
                ln["frac_of_measured"] = ln["GBps"] / copy_gbs
        out[name] = ln
    if world > 1:
        # whole-job figures: every rank ran the same per-GPU share; the job is as fast as its slowest rank
        names = sorted(k for k in out if "ms" in out[k])
        mine = torch.tensor([out[k]["ms"] for k in names], dtype=torch.float64, device=torch.device("cpu") if dry else torch.device("cuda", local_rank))
        allms = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allms, mine)
        worst = torch.stack(allms).max(dim=0).values.tolist()
        for k, w in zip(names, worst):
            e = out[k]
            scale = e["ms"] / w
            e["ms_slowest_rank"] = w
            for f in ("frames_per_s", "pairs_per_s", "dp_cells_per_s", "GBps"):
                if f in e and e[f] is not None:
                    e[f + "_whole_job"] = e[f] * scale * world
    return out if rank == 0 else None


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher: start the N ranks ourselves."""
    import subprocess
    if not args.dry_run_cpu:
        import torch
        have = torch.cuda.device_count()
        if have < args.gpus:
            sys.exit("bench.py: --gpus %d requested but this node has %d GPU(s); refusing to run a smaller job "
                     "under that label" % (args.gpus, have))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_launch(args)
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d: launch exactly one rank per GPU" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    import torch.distributed as dist
    dry = args.dry_run_cpu
    # the process group (and with it every barrier, reduction and gather below) also at world size 1 when the launcher's environment is
    # there and NNMNKWII_BENCH_FORCE_DIST=1: how a one-GPU box runs the RCCL path of the N > 1 legs (tests/test_host_multi_gpu.py)
    use_dist = world > 1 or (os.environ.get("NNMNKWII_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    B, T, sd = args.batch, args.frames, args.static_dim
    D = 3 * sd
    if dry:
        dev = torch.device("cpu")
        if use_dist:
            dist.init_process_group("gloo")
        out = status = None

        def step():
            return None, None

        def sync():
            pass
    else:
        from nnmnkwii_amd import _hip
        if torch.cuda.device_count() <= local_rank:
            sys.exit("bench.py: rank %d has no GPU (device_count = %d)" % (rank, torch.cuda.device_count()))
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        if use_dist:
            dist.init_process_group("nccl", device_id=dev)
        gen = torch.Generator(device=dev).manual_seed(1234 + rank)
        means = torch.randn(B, T, D, dtype=torch.float64, device=dev, generator=gen)
        variances = torch.rand(B, T, D, dtype=torch.float64, device=dev, generator=gen) + 0.1

        def step():
            return _hip.forward(means, variances, WINDOWS, None, algo=args.algo, want_status=True)

        def sync():
            torch.cuda.synchronize(dev)

    def barrier():
        if use_dist:
            if dry:
                dist.barrier()
            else:
                dist.barrier(device_ids=[local_rank])

    def timed(nsteps):
        """(wall seconds, ms per launch from one HIP-event pair on the launch stream) for nsteps back-to-back steps."""
        o = st = None
        if dry:
            t0 = time.perf_counter()
            for _ in range(nsteps):
                o, st = step()
            return time.perf_counter() - t0, 0.0, o, st
        ev0, ev1 = events
        t0 = time.perf_counter()
        ev0.record()
        for _ in range(nsteps):
            o, st = step()
        ev1.record()
        sync()
        return time.perf_counter() - t0, float(ev0.elapsed_time(ev1)) / nsteps, o, st

    events = None
    if not dry:
        # the timing events exist and have been used once before the timed region (their first use initialises
        # runtime state: 0.3 ms that belongs to no step)
        events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        events[0].record()
        events[1].record()
        sync()
        events[0].elapsed_time(events[1])

    # What a plain copy kernel reaches on this box, in this run (the library's own streaming copy, 16 B per lane): the
    # measured peak beside the nominal 8 TB/s: best of 16 groups of 50 copies.  Taken BEFORE the warm-up steps (about
    # 0.15 s of copies; the clocks of an idle MI355X settle over roughly 0.1 s of work -- see `repeat_regions`): the timed
    # region then starts on a GPU that has been busy for a while, as it is in any batch job, not 3 launches after idle.
    # --full only: the headline figure does not need it (the preconditioning leg below settles the clocks).
    copy_gbs = None
    if rank == 0 and not dry and args.full:
        nb = 512 << 20
        src = torch.empty(nb // 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        for _ in range(3):
            _hip.stream_copy(src, dst)
        sync()
        best = None
        for _ in range(16):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                _hip.stream_copy(src, dst)
            e1.record()
            sync()
            t = float(e0.elapsed_time(e1)) / 50
            best = t if best is None else min(best, t)
        assert torch.equal(src, dst)
        copy_gbs = 2.0 * nb / (best * 1e-3) / 1e9
        del src, dst


    # The driver's protocol TO THE LETTER first -- W untimed steps, then exactly K timed ones, nothing in front -- reported as
    # `cold_protocol` / roofline.kernel_ms_cold: what a short job sees, on clocks that are still ramping (profiles/r05_notes.md
    # section 18).  `value` is the same region taken again behind the preconditioning leg below, on settled clocks.  --full only.
    cold = None
    if not dry and args.full:
        for _ in range(args.warmup):
            step()
        sync()
        barrier()
        c_el, c_km, _, _ = timed(args.steps)
        barrier()
        tc = torch.tensor([c_el], dtype=torch.float64, device=dev)
        if use_dist:
            allc = [torch.zeros_like(tc) for _ in range(world)]
            dist.all_gather(allc, tc)
            c_el = max(float(x.item()) for x in allc)
        cold = (c_el, c_km)

    # The device's clocks settle over tens of milliseconds of this kernel (`repeat_regions` below showed regions of 20 steps at
    # 0.2093-0.2116 ms once a few hundred steps had run, against 0.221-0.237 ms for the same region 5 steps after the copy
    # measurement): a leg of the same steps in front of the official warm-up, event-timed and reported (kernel_ms_steady).
    # Plain runs too: `value` is the settled-clock figure.
    steady_ms = None
    if not dry and args.precondition > 0:
        timed(args.precondition - args.precondition // 2)
        _, steady_ms, _, _ = timed(max(args.precondition // 2, 1))   # (the second half: past most of the ramp)

    for _ in range(args.warmup):
        out, status = step()
    sync()

    # in-run single-GPU leg (N > 1 and --full only): rank 0 alone, the others idle, same kernel and batch
    solo = None
    if world > 1 and args.full:
        barrier()
        if rank == 0:
            el, _, _, _ = timed(args.steps)
            solo = B * T * args.steps / el
        barrier()

    barrier()
    sync()
    elapsed, kern_ms, out, status = timed(args.steps)
    barrier()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out, status)

    if not dry:
        if not args.no_check:
            assert int(status.abs().max().item()) == 0, "a system was not positive definite (or an internal wait timed out)"
        elif os.environ.get("MLPG_DUMP_STATUS"):
            if os.environ.get("MLPG_DUMP_STATUS") == "trace":
                tr = status.cpu().numpy()[:3840 * 4].reshape(-1, 4).astype(np.int64)
                t0 = tr[:, 0]
                t0 = (t0 - t0.min()) & 0x3FFFFFFF
                asm, arr = tr[:, 1] & 0xFFFF, tr[:, 1] >> 16
                l3, end = tr[:, 2], tr[:, 3] & 0xFFFFFF
                ph = (tr[:, 3] >> 28) & 1
                print("strip trace (100 MHz ticks = 10 ns)", file=sys.stderr)
                for nm, v in (("loads-done", asm), ("arrived", arr), ("level3", l3), ("end", end)):
                    print("  to %-10s median %d  p10 %d  p90 %d  max %d" % (nm, np.median(v), np.percentile(v, 10), np.percentile(v, 90), v.max()), file=sys.stderr)
                # how many workgroups are loading / in the chain / at all active, per 2 us
                span = int((t0 + end).max()) + 1
                loading = np.zeros(span + 1); active = np.zeros(span + 1)
                np.add.at(loading, t0, 1); np.add.at(loading, t0 + asm, -1)
                np.add.at(active, t0, 1); np.add.at(active, t0 + end, -1)
                loading, active = np.cumsum(loading)[:span], np.cumsum(active)[:span]
                nb = span // 200
                print("  kernel span %d ticks; mean workgroups loading %.0f, active %.0f" % (span, loading.mean(), active.mean()), file=sys.stderr)
                print("  loading per 2 us:", [int(x) for x in loading[:nb * 200].reshape(nb, 200).mean(1)][:160], file=sys.stderr)
                print("  active  per 2 us:", [int(x) for x in active[:nb * 200].reshape(nb, 200).mean(1)][:160], file=sys.stderr)
                print("  phase-1 items: %d; their first start %d" % (int(ph.sum()), int(t0[ph == 1].min()) if ph.any() else -1), file=sys.stderr)
            elif os.environ.get("MLPG_DUMP_STATUS") == "strip":
                st = status.cpu().numpy()[:8 * 16 * 16].reshape(8, 16, 16)
                names = "claim assemble eliminate barrier level2 publish poll barrier l3-stage l3-sweep l2-back barrier backsub store l3-first-read l3-row-loop".split()
                mean = st.reshape(-1, 16).mean(0)
                print("strip phase cycles of wavefront 0, mean over 8 utterances x 16 strips:",
                      {n: int(x) for n, x in zip(names, mean)}, "sum", int(mean[:14].sum()), file=sys.stderr)
                print("  poll cycles by strip index:", [int(x) for x in st[:, :, 6].mean(0)], file=sys.stderr)
                for k, n in enumerate(names):
                    print("  %-10s by strip: %s" % (n, [int(x) for x in st[:, :, k].mean(0)]), file=sys.stderr)

            else:
                st = status.cpu().numpy()[:64 * 8].reshape(64, 8)
                print("phase cycles (setup, wait-tiles, lds->regs, dma-issue, assembly, solve, status, output), mean over 64 WGs:",
                      [int(x) for x in st.mean(0)], "sum", int(st.mean(0).sum()), file=sys.stderr)

    per_rank = [elapsed]
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if use_dist:
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank = [float(x.item()) for x in allt]
    elapsed = max(per_rank)

    gather_ms = None
    if args.gather and use_dist and not dry:
        full = torch.empty((world,) + tuple(out.shape), dtype=out.dtype, device=dev)
        dist.all_gather_into_tensor(full, out)
        sync()
        barrier()
        g0 = time.perf_counter()
        dist.all_gather_into_tensor(full, out)
        sync()
        gather_ms = (time.perf_counter() - g0) * 1e3

    # a longer steady-state leg (informational): the driver's --steps 20 is a ~4 ms region
    if steady_ms is None and rank == 0 and not dry and args.full:
        _, steady_ms, _, _ = timed(max(200, args.steps))

    # the official region is short at the driver's --steps (a few ms): repeat it and report the spread beside it
    regions = None
    if not dry and args.full and args.regions > 0:
        rs = []
        for _ in range(args.regions):
            barrier()
            el, km, _, _ = timed(args.steps)
            rs.append((el / args.steps * 1e3, km))
        regions = {"k": len(rs), "ms_per_step_median": float(np.median([r[0] for r in rs])),
                   "ms_per_step_min": float(min(r[0] for r in rs)), "ms_per_step_max": float(max(r[0] for r in rs)),
                   "kernel_ms_median": float(np.median([r[1] for r in rs])),
                   "ms_per_step_all": [round(r[0], 5) for r in rs], "kernel_ms_all": [round(r[1], 5) for r in rs]}

    # the other BASELINE configs and kernel variants (after the metric; never part of `value`)
    secondary = None
    if args.full and not args.no_secondary and (not dry or world > 1):
        secondary = collect_secondary(rank, world, local_rank, copy_gbs, dry=dry)

    if rank == 0:
        err = err_tight = None
        if not dry and args.full:
            # parity spot checks outside the timed region (oracle = checker only): the first 4 utterances of the timed batch
            #  and the last one, then the same batch with the dynamic variances 100 x / 1000 x tighter -- the strip
            # kernel's other level-3 rungs, which the timed data never takes -- utterances 0 and B - 1
            from oracle import mlpg as O
            O.build()

            def rel(y, m_, v_):
                yo = O.mlpg(m_.cpu().numpy(), v_.cpu().numpy(), WINDOWS)
                return float(np.abs(y.cpu().numpy() - yo).max() / np.abs(yo).max())

            err = max(rel(out[b], means[b], variances[b]) for b in sorted(set([0, 1, 2, 3, B - 1]) & set(range(B))))
            vt = variances.clone()
            vt[:, :, sd:2 * sd] *= 1e-2
            vt[:, :, 2 * sd:] *= 1e-3
            yt, stt = _hip.forward(means, vt, WINDOWS, None, algo=args.algo, want_status=True)
            err_tight = max(rel(yt[b], means[b], vt[b]) for b in sorted(set([0, B - 1])))
            assert int(stt.abs().max().item()) == 0
            del vt, yt, stt
            if not args.no_check:
                assert err < 1e-9, err
                assert err_tight < 1e-9, err_tight

        # HBM traffic of the dominant kernel: measured now (N = 1), else the committed PMC pass of this command
        traffic, traffic_note = None, "not measured" if args.full else "not measured (bench.py --full measures it)"
        if not dry and args.full:
            why = "skipped (--no-traffic)" if args.no_traffic else "N > 1"
            if world == 1 and not args.no_traffic:
                traffic, why = live_traffic(B, T, sd, args.algo)
            traffic_note = why
            if traffic is None:
                traffic = measured_traffic(B, T, sd, args.algo)
                traffic_note = ("taken from the committed rocprofv3 pass profiles/traffic.json of this command (live pass: %s)" % why
                                if traffic is not None else "none (live pass: %s)" % why)

        frames = world * B * T * args.steps
        alg_bytes = 56.0 * sd * B * T            # 56 B per (frame, static dim) per launch
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9 if kern_ms else None
        algo_names = {0: "auto", 1: "generic", 2: "wave-per-system", 3: "strip", 4: "strip (algo 4 retired)", 5: "constant-coefficient"}
        res = {
            "metric": "MLPG frames/sec (batch, 60-dim mgc x3 windows)",
            "value": frames / elapsed,
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "preconditioning": ("%d steps of the same workload (the second half event-timed: roofline.kernel_ms_steady) ran before the %d warm-up steps: "
                                "the device's clocks settle over tens of ms of this kernel; see repeat_regions" % (args.precondition, args.warmup))
                               if (args.precondition > 0 and not dry) else None,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "full": args.full,
            "config": {
                "workload": "BASELINE configs[1]: %d utterances/GPU x T=%d x %d-dim mgc static+delta+delta-delta "
                            "(%d columns), float64, per-frame variances, std 3 windows; mlpg_hip_forward via C ABI"
                            % (B, T, sd, D),
                "inputs": "means ~ N(0,1), variances ~ U(0.1, 1.1), generated in HBM by torch.Generator(seed 1234 + rank) "
                          "(the distributions of SURVEY 8(d); not numpy RandomState(1234), which would mean a host copy)",
                "batch_per_gpu": B, "frames": T, "static_dim": sd, "algo": args.algo,
                "kernel": algo_names.get(args.algo, "?") + (" (= strip at this shape: mlpg::strip::strip_kernel)" if args.algo == 0 else ""),
                "parallelism": "batch-sharded x%d, no data-path collective" % world,
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS if achieved else None,
                "peak_measured": copy_gbs,
                "peak_measured_kernel": "mlpg_hip_stream_copy, 512 MiB -> 512 MiB, (read + written bytes) / best of 16 x 50 launches, same run",
                "frac_of_measured": (achieved / copy_gbs) if (achieved and copy_gbs) else None,
                "traffic": traffic,
                "traffic_unit": "bytes/launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE); " + traffic_note,
                "kernel_ms": kern_ms,
                "kernel_ms_cold": cold[1] if cold else None,
                "frac_cold": (alg_bytes / (cold[1] * 1e-3) / 1e9 / HBM_PEAK_GBS) if (cold and cold[1]) else None,
                "kernel_ms_steady": steady_ms,
                "algorithmic_bytes": alg_bytes,
            },
            "cold_protocol": ({"value": frames / cold[0], "unit": "frames/s", "ms_per_step": cold[0] / args.steps * 1e3,
                               "note": "the driver's protocol to the letter, taken first: %d untimed steps behind the copy-rate measurement, then "
                                       "these %d timed steps, no preconditioning; `value` is the same region on settled clocks" % (args.warmup, args.steps)}
                              if cold else None),
            "parity_rel_err_vs_oracle": err,
            "parity_checked": "utterances 0-3 and the last of the timed batch; rel err max|y - y_oracle| / max|y_oracle| per utterance" if err is not None else None,
            "parity_rel_err_vs_oracle_tight_dynamic_variances": err_tight,
            "per_rank_ms_per_step": [x / args.steps * 1e3 for x in per_rank],
        }
        if dry:
            res["dry_run"] = True
        if solo is not None:
            res["in_run_single_gpu"] = {"value": solo, "unit": "frames/s",
                                        "weak_scaling_efficiency": (frames / elapsed) / (world * solo)}
        if gather_ms is not None:
            res["allgather_ms"] = gather_ms
        if regions is not None:
            res["repeat_regions"] = regions
        if secondary is not None:
            res["secondary"] = secondary
        if world == 1 and args.full and not args.no_cpu_baseline and not dry:
            res["cpu_baseline"] = cpu_baseline(T, D, args.cpu_seconds)
        print(json.dumps(res), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
