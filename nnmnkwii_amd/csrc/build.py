"""Build nnmnkwii_amd/csrc/libmlpg_hip.so for gfx950 with hipcc (in-tree)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["capi.hip", "streams_api.hip", "host_api.hip", "mlpg_generic.hip", "mlpg_wave.hip", "mlpg_wave_fwd_f64.hip", "mlpg_wave_fwd_f32.hip",
           "mlpg_wave_bwd_f64.hip", "mlpg_wave_bwd_f32.hip", "mlpg_wave_fused.hip", "mlpg_strip.hip", "mlpg_strip_fwd_f64.hip",
           "mlpg_strip_fwd_f32.hip", "mlpg_strip_bwd_f64.hip", "mlpg_strip_bwd_f32.hip", "mlpg_strip_std_fwd_f64.hip", "mlpg_strip_std_fwd_f32.hip", "mlpg_strip_std_bwd_f64.hip", "mlpg_strip_std_bwd_f32.hip", "mlpg_strip_multi_f64.hip", "mlpg_strip_multi_f32.hip", "mlpg_const.hip", "mlpg_const_fwd_f64.hip", "mlpg_const_fwd_f32.hip", "mlpg_const_bwd_f64.hip", "mlpg_const_bwd_f32.hip", "mlpg_const_multi_f64.hip", "mlpg_const_multi_f32.hip", "mlpg_chunk.hip", "mlpg_chunk_fwd_f64.hip", "mlpg_chunk_fwd_f32.hip", "mlpg_chunk_bwd_f64.hip", "mlpg_chunk_bwd_f32.hip", "mlpg_fir.hip", "mlpg_vargrad.hip", "mlpg_streams_bwd.hip", "dtw.hip", "dtw_fast.hip", "dtw_costs.hip", "modspec.hip", "modspec_chirp.hip", "modspec_filter.hip", "modspec_dft.hip", "modspec_api.hip", "gmm_em.hip", "kmeans.hip", "postfilter.hip", "gmm_traj.hip", "mlpg_gv.hip", "colstats.hip", "frame_metrics.hip", "frame_expand.hip", "f0_interp.hip", "wave_codec.hip", "joint_rows.hip", "frame_keep.hip", "mlpg_trajcov.hip", "mlpg_trajsample.hip"]
HEADERS = ["common.h", "device_prims.h", "mlpg_strip_geom.h", "assemble.h", "vargrad_element.h", "mlpg_wave_impl.h", "mlpg_strip_impl.h", "mlpg_const_impl.h", "mlpg_chunk_impl.h", "modspec_fft.h", "postfilter_table.h", os.path.join("..", "..", "include", "mlpg_hip.h"),
           os.path.join("..", "..", "include", "nnmnkwii_metrics.h"), os.path.join("..", "..", "include", "nnmnkwii_frontend.h"),
           os.path.join("..", "..", "include", "nnmnkwii_f0.h"), os.path.join("..", "..", "include", "nnmnkwii_wave.h"),
           os.path.join("..", "..", "include", "nnmnkwii_joint.h"), os.path.join("..", "..", "include", "nnmnkwii_silence.h"),
           os.path.join("..", "..", "include", "nnmnkwii_trajectory.h"), os.path.join("..", "..", "include", "nnmnkwii_sample.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]
# The DTW kernels must round exactly like the CPU oracle (separate multiply and add); the MLPG
# kernels are free to fuse multiply-adds.
# mlpg_chunk_*.hip: their per-chunk loop (24 frame slots, a few hundred instructions each) must be unrolled completely -- every array
# index a constant -- and is larger than the optimiser's default limit for "#pragma unroll" (left at the default the loop stays
# and the arrays land in scratch).
FILE_FLAGS = {"mlpg_fir.hip": ["-ffp-contract=fast", "-mllvm", "-pragma-unroll-threshold=200000", "-mllvm", "-unroll-threshold=200000"],
              **{"mlpg_chunk_%s_%s.hip" % (d, t): ["-ffp-contract=fast", "-mllvm", "-pragma-unroll-threshold=200000", "-mllvm", "-unroll-threshold=200000"]
                 for d in ("fwd", "bwd") for t in ("f64", "f32")},
              "dtw_fast.hip": ["-ffp-contract=off"], "dtw.hip": ["-ffp-contract=off"], "dtw_costs.hip": ["-ffp-contract=off"], "modspec.hip": ["-ffp-contract=off"], "modspec_chirp.hip": ["-ffp-contract=off"], "modspec_filter.hip": ["-ffp-contract=off"], "modspec_dft.hip": ["-ffp-contract=off"], "gmm_em.hip": ["-ffp-contract=off"], "kmeans.hip": ["-ffp-contract=off"], "postfilter.hip": ["-ffp-contract=off"], "gmm_traj.hip": ["-ffp-contract=off"], "mlpg_gv.hip": ["-ffp-contract=off"], "colstats.hip": ["-ffp-contract=off"], "frame_metrics.hip": ["-ffp-contract=off"], "frame_expand.hip": ["-ffp-contract=off"], "f0_interp.hip": ["-ffp-contract=off"],
              "wave_codec.hip": ["-ffp-contract=off"], "joint_rows.hip": ["-ffp-contract=off"],
              "frame_keep.hip": ["-ffp-contract=off"], "mlpg_trajcov.hip": ["-ffp-contract=off"],
              "mlpg_trajsample.hip": ["-ffp-contract=off"]}
COST = {"mlpg_wave_bwd_f64.hip": 29, "mlpg_wave_bwd_f32.hip": 27, "mlpg_chunk_bwd_f64.hip": 26, "mlpg_chunk_bwd_f32.hip": 26, "mlpg_strip_bwd_f64.hip": 23,
        "mlpg_strip_bwd_f32.hip": 23, "mlpg_chunk_fwd_f64.hip": 20, "mlpg_chunk_fwd_f32.hip": 20, "mlpg_fir.hip": 18, "mlpg_wave_fwd_f64.hip": 18,
        "mlpg_wave_fwd_f32.hip": 15, "mlpg_generic.hip": 14, "mlpg_strip_fwd_f32.hip": 13, "mlpg_strip_fwd_f64.hip": 12, "mlpg_const_bwd_f32.hip": 12,
        "mlpg_const_bwd_f64.hip": 12, "mlpg_strip_multi_f64.hip": 9, "mlpg_wave_fused.hip": 9, "mlpg_strip_multi_f32.hip": 8}
EXTRA = [f for f in os.environ.get("MLPG_HIP_EXTRA_FLAGS", "").split() if f]
SO = os.path.join(HERE, "libmlpg_hip.so")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _headers_of(src):
    """Headers a source depends on (the two big kernel headers only matter to their own instantiation files)."""
    hs = [h for h in HEADERS if h not in ("mlpg_wave_impl.h", "mlpg_strip_impl.h", "mlpg_const_impl.h", "mlpg_chunk_impl.h", "modspec_fft.h", "postfilter_table.h")
          and not h.endswith("nnmnkwii_metrics.h") and not h.endswith("nnmnkwii_frontend.h") and not h.endswith("nnmnkwii_f0.h")
          and not h.endswith("nnmnkwii_wave.h") and not h.endswith("nnmnkwii_joint.h") and not h.endswith("nnmnkwii_silence.h")
          and not h.endswith("nnmnkwii_trajectory.h") and not h.endswith("nnmnkwii_sample.h")]
    if src == "frame_metrics.hip":
        hs.append(os.path.join("..", "..", "include", "nnmnkwii_metrics.h"))
    if src == "frame_expand.hip":
        hs.append(os.path.join("..", "..", "include", "nnmnkwii_frontend.h"))
    if src == "f0_interp.hip":
        hs.append(os.path.join("..", "..", "include", "nnmnkwii_f0.h"))
    if src == "wave_codec.hip":
        hs.append(os.path.join("..", "..", "include", "nnmnkwii_wave.h"))
    if src == "joint_rows.hip":
        hs.append(os.path.join("..", "..", "include", "nnmnkwii_joint.h"))
    if src == "frame_keep.hip":   # (its header includes the frontend's for the dtype and kind codes)
        hs += [os.path.join("..", "..", "include", "nnmnkwii_silence.h"), os.path.join("..", "..", "include", "nnmnkwii_frontend.h")]
    if src == "mlpg_trajcov.hip":
        hs.append(os.path.join("..", "..", "include", "nnmnkwii_trajectory.h"))
    if src == "mlpg_trajsample.hip":
        hs.append(os.path.join("..", "..", "include", "nnmnkwii_sample.h"))
    if src == "postfilter.hip":
        hs.append("postfilter_table.h")
    if src in ("modspec.hip", "modspec_chirp.hip", "modspec_filter.hip"):
        hs.append("modspec_fft.h")
    if src.startswith("mlpg_wave_"):
        hs.append("mlpg_wave_impl.h")
    if src.startswith("mlpg_strip_"):
        hs.append("mlpg_strip_impl.h")
    if src.startswith("mlpg_const_"):
        hs.append("mlpg_const_impl.h")
    if src.startswith("mlpg_chunk"):
        hs.append("mlpg_chunk_impl.h")
    return [os.path.join(HERE, h) for h in hs] + [os.path.abspath(__file__)]


def build(force=False, verbose=False, only=None):
    """only: iterable of source-name prefixes to force-rebuild (kernel experiments with MLPG_HIP_EXTRA_FLAGS)."""
    hipcc = _hipcc()
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(HERE, src)
        o = os.path.join(HERE, src.replace(".hip", ".o"))
        objs.append(o)
        forced = force or (only is not None and any(src.startswith(pfx) for pfx in only))
        if forced or _stale(o, [s] + _headers_of(src)):
            jobs.append([hipcc, "-x", "hip", *FLAGS, *FILE_FLAGS.get(src, ["-ffp-contract=fast"]), *EXTRA, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
        return r.stderr

    if jobs:
        # longest first (seconds of one hipcc run, measured in round 6): the pool finishes when its longest-running job does
        jobs.sort(key=lambda cmd: -COST.get(os.path.basename(cmd[-3]), 5))
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 8, 16)) as ex:
            for err in ex.map(run, jobs):
                if verbose and err.strip():
                    print(err)
    if force or jobs or _stale(SO, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO, *objs])
    return SO


if __name__ == "__main__":
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--only=")]
    print(build(force="--force" in sys.argv, verbose="--quiet" not in sys.argv, only=only or None))
