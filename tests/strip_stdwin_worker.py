"""Child process of test_strip_stdwin_gpu.py: runs a fixed list of strip-kernel launches and writes every output and
status array to an .npz file.  The parent runs it twice -- MLPG_STRIP_STDWIN unset (the instantiations compiled for the
standard windows) and MLPG_STRIP_STDWIN=0 (the general ones; the switch is read once per process, hence the child) --
and compares the two files.  Not a test module.

    python tests/strip_stdwin_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from cases import WINDOW_SETS, c2_utterance  # noqa: E402

STD3 = WINDOW_SETS["std3"]
# window sets one step away from the standard one: all must take the general kernel
NEAR = {
    "near_half": [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5000001, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))],
    "scaled": [(0, 0, np.array([1.0])), (1, 1, np.array([-1.0, 0.0, 1.0])), (1, 1, np.array([1.0, -2.0, 1.0]))],
    "reordered": [(0, 0, np.array([1.0])), (1, 1, np.array([1.0, -2.0, 1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))],
}
SD = 60


def c2_slice(B=32, T=1000):
    m = np.empty((B, T, 3 * SD))
    v = np.empty((B, T, 3 * SD))
    for b in range(B):
        m[b], v[b] = c2_utterance(b, T, SD)
    return m, v


def ragged_case():
    """Tmax = 300 (not a multiple of 64), lengths down to 1: whole strips of padding, last strips of every fill, T < 64."""
    rng = np.random.RandomState(901)
    lengths = np.array([300, 299, 257, 256, 193, 191, 130, 129, 128, 65, 64, 63, 33, 17, 16, 15, 3, 2, 1, 300], dtype=np.int32)
    B, T = len(lengths), 300
    m = rng.randn(B, T, 3 * SD)
    v = rng.rand(B, T, 3 * SD) + 0.1
    return m, v, lengths


def tight_case():
    """Dynamic variances 100 x / 1000 x tighter than the static ones: the 3-strip and 5-strip windows of level 3 are rejected
    (as in test_strip_tight_dynamic_variances_every_window_rejected), changing regime along the utterance."""
    rng = np.random.RandomState(902)
    B, T = 6, 1536
    m = rng.randn(B, T, 3 * SD)
    v = rng.rand(B, T, 3 * SD) + 0.1
    for b in range(B):
        for s0 in range(0, T, 128):
            f1, f2 = ((1.0, 1.0), (0.1, 0.01), (0.01, 0.001))[(s0 // 128 + b) % 3 if b else 2]
            v[b, s0:s0 + 128, SD:2 * SD] *= f1
            v[b, s0:s0 + 128, 2 * SD:] *= f2
    lengths = np.array([T, T - 1, 1000, 65, 700, T], dtype=np.int32)
    return m, v, lengths


def failure_case():
    """The c2 slice with variances that are negative, 0, Inf or NaN scattered over utterances, dims, windows and frames -- random
    places plus every position of a 64-frame strip that matters to the blocked elimination (first / last rows of a chunk,
    the chunk's separator rows 14 and 15, the strip's last separator, the utterance's first and last frames)."""
    rng = np.random.RandomState(903)
    m, v = c2_slice()
    B, T = v.shape[:2]
    vals = [-1e-3, 0.0, np.inf, np.nan, -0.0, -np.inf]
    places = []
    for k in range(96):
        places.append((rng.randint(B), rng.randint(T), rng.randint(3), rng.randint(SD)))
    special_t = [0, 1, 2, 13, 14, 15, 16, 17, 30, 31, 46, 47, 61, 62, 63, 64, 65, 126, 127, 128, 959, 960, 997, 998, 999]
    for k, (b, t, w, d) in enumerate(places):
        v[b, t, w * SD + d] = vals[k % len(vals)]
    for t in special_t:                                   # every value in every window at every special frame
        for w in range(3):
            for val in vals:
                v[rng.randint(B), t, w * SD + rng.randint(SD)] = val
    return m, v


def main(out_path):
    import torch
    from nnmnkwii_amd import _hip
    from oracle import mlpg as O

    res = {}
    counts = {}

    def count():
        return int(_hip.lib().mlpg_hip_launch_count(2))  # strip kernel launches (all instantiations)

    def run(name, m, v, lengths, windows=STD3, dtypes=(np.float64, np.float32), seed=7):
        rng = np.random.RandomState(seed)
        B, T = m.shape[:2]
        go64 = rng.randn(B, T, SD)
        L = None if lengths is None else torch.from_numpy(lengths).cuda()
        for dt in dtypes:
            tag = "%s/%s" % (name, np.dtype(dt).name)
            mg, vg = torch.from_numpy(m.astype(dt)).cuda(), torch.from_numpy(v.astype(dt)).cuda()
            go = torch.from_numpy(go64.astype(dt)).cuda()
            n0 = count()
            y, st = _hip.forward(mg, vg, windows, L, algo=_hip.ALGO_STRIP)
            res[tag + "/fwd"], res[tag + "/fwd_status"] = y.cpu().numpy(), st.cpu().numpy()
            for od in (torch.float64, torch.float32):
                g, st = _hip.backward(vg, go, windows, 3 * SD, L, out_dtype=od, algo=_hip.ALGO_STRIP)
                key = tag + "/bwd_" + str(od).split(".")[-1]
                res[key], res[key + "_status"] = g.cpu().numpy(), st.cpu().numpy()
            torch.cuda.synchronize()
            counts[tag] = count() - n0

    m, v = c2_slice()
    run("c2", m, v, None)
    m, v, lengths = ragged_case()
    run("ragged", m, v, lengths)
    m, v, lengths = tight_case()
    run("tight", m, v, lengths)
    m, v = failure_case()
    run("fail", m, v, None)
    # near-standard windows: the general kernel, checked against the oracle here (float64)
    m, v, lengths = ragged_case()
    for wname, wins in NEAR.items():
        run("near_" + wname, m, v, lengths, windows=wins, dtypes=(np.float64,))
        ref, _, rc = O.mlpg_batch(m, v, wins, lengths)
        assert rc == 0
        y = res["near_%s/float64/fwd" % wname]
        res["near_%s/oracle_err" % wname] = np.array(np.abs(y - ref).max() / np.abs(ref).max())
        # ... and what the standard set would have given: far outside that tolerance, so the error shows which kernel ran
        ref_std, _, _ = O.mlpg_batch(m, v, STD3, lengths)
        res["near_%s/distance_to_std" % wname] = np.array(np.abs(ref_std - ref).max() / np.abs(ref).max())
    for k, n in counts.items():
        res["count/" + k] = np.array(n)
    np.savez(out_path, **res)
    print("wrote %d arrays to %s" % (len(res), out_path))


if __name__ == "__main__":
    main(sys.argv[1])
