"""GPU tests (-m gpu): the stream contract of include/nnmnkwii_trajectory.h -- every launch on the caller's stream, no
synchronisation, no allocation, no default-stream work -- with the checks of tests/stream_contract.py that
tests/test_stream_contract_gpu.py applies to the other families: captured on a side stream and replayed on new data behind the
same pointers, two streams interleaved, and behind a late producer.  The wrappers that hand the stream on live in
nnmnkwii_amd/_trajectory_calls.py; the walk at the end finds every function there that asks for the stream and wants a cell for it
(it needs no device, but sits here beside the table it checks)."""
import ast
import os

import numpy as np
import pytest
import torch

import stream_contract as SC
import trajcov_cases as C
from trajcov_cases import TM

B, TMAX, SD, WNAME = 3, 70, 65, "std3"
WIN = C.WINDOWS[WNAME]
D = len(WIN) * SD
LENGTHS = {1: [70, 0, 33], 2: [5, 70, 64]}


def bit_fails(*triples):
    return ["%s differs from the model" % name for name, t, want in triples if not C.same_bits(t.cpu().numpy(), want)]


def make_cov(seed):
    return dict(var=C.variances(seed, B, TMAX, SD, WNAME, TM.VAR_FRAME), lengths=np.array(LENGTHS[seed], dtype=np.int32))


def want_cov(c):
    key = "_want"
    if key not in c:
        c[key] = TM.covariance_batch(c["var"], WIN, c["lengths"], B, TMAX, SD)
    return c[key]


def load_cov(b, c):
    SC.put(b, "in_var", c["var"])
    SC.put(b, "in_idx_lengths", c["lengths"])
    SC.out(b, "out_band", (3, B, TMAX, SD), torch.float64)
    SC.out(b, "out_logdet", (B, SD), torch.float64)
    SC.out(b, "out_status", (B, SD), torch.int32)


def call_cov(b):
    from nnmnkwii_amd import _trajectory_calls as TC
    TC.covariance(b["in_var"], WIN, b["in_idx_lengths"], B, TMAX, D, band=b["out_band"], logdet=b["out_logdet"], status=b["out_status"])


def verdict_cov(c, b):
    band, logdet, status = want_cov(c)
    fails = bit_fails(("band", b["out_band"], band), ("status", b["out_status"], status))
    got = b["out_logdet"].cpu().numpy()
    live = TM.live_frames(c["lengths"], B, TMAX)
    for u in range(B):
        if not (np.abs(got[u] - logdet[u]) <= C.logdet_bound(c["var"][u], WNAME, int(live[u]), SD)).all():
            fails.append("logdet of utterance %d is outside the bound" % u)
    return fails


def make_nll(seed):
    """Global variances: the likelihood launch, its workspace and the finish launch."""
    var = C.variances(seed, B, TMAX, SD, WNAME, TM.VAR_GLOBAL)
    lengths = np.array(LENGTHS[seed], dtype=np.int32)
    mean, target = C.features(seed + 10, B, TMAX, D), C.features(seed + 20, B, TMAX, SD)
    band, logdet, _ = TM.covariance_batch(var, WIN, lengths, B, TMAX, SD)
    cbar = np.zeros((B, TMAX, SD))
    for u in range(B):
        cbar[u, :lengths[u]] = TM.mean_trajectory(mean[u], var, WIN, int(lengths[u]), SD)
    return dict(var=var, lengths=lengths, mean=mean, target=target, band=band, logdet=logdet, cbar=cbar)


def want_nll(c):
    if "_want" not in c:
        c["_want"] = TM.nll_batch(c["mean"], c["var"], WIN, c["cbar"], c["target"], c["lengths"], c["band"], c["logdet"])
    return c["_want"]


def load_nll(b, c):
    for k in ("var", "mean", "target", "band", "logdet", "cbar"):
        SC.put(b, "in_" + k, c[k])
    SC.put(b, "in_idx_lengths", c["lengths"])


def call_nll(b):
    from nnmnkwii_amd import _trajectory_calls as TC
    b["out_nll"], b["out_gm"], b["out_gv"] = TC.nll(b["in_mean"], b["in_var"], WIN, b["in_cbar"], b["in_target"], b["in_idx_lengths"],
                                                    b["in_band"], b["in_logdet"])


def verdict_nll(c, b):
    nll, gm, gv = want_nll(c)
    return bit_fails(("nll", b["out_nll"], nll), ("grad_means", b["out_gm"], gm), ("grad_vars", b["out_gv"], gv))


CELLS = [SC.Cell("trajectory.covariance", ["_trajectory_calls.covariance"], make_cov, load_cov, call_cov, verdict_cov,
                 expected=lambda c: list(want_cov(c)[:2])),      # (the status is 0 in both cases)
         SC.Cell("trajectory.nll", ["_trajectory_calls.nll"], make_nll, load_nll, call_nll, verdict_nll, expected=lambda c: list(want_nll(c)))]


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_replayed_on_new_data(cell):
    SC.replayed_on_new_data(cell)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_two_streams_interleaved(cell):
    SC.two_streams_interleaved(cell)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_behind_a_late_producer(cell):
    SC.behind_a_late_producer(cell)


@pytest.mark.gpu
def test_both_entries_back_to_back_on_one_stream():
    SC.one_stream_shared(CELLS)


# ---- completeness and sharpness (no device) ---------------------------------------------------------------------------------------

def test_every_wrapper_that_takes_the_stream_has_a_cell():
    path = os.path.join(C.ROOT, "nnmnkwii_amd", "_trajectory_calls.py")
    tree = ast.parse(open(path).read(), path)
    users = set()
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            for node in ast.walk(fn):
                f = getattr(node, "func", None)
                if isinstance(node, ast.Call) and ((isinstance(f, ast.Name) and f.id == "_stream") or (isinstance(f, ast.Attribute) and f.attr == "_stream")):
                    users.add("_trajectory_calls." + fn.name)
    assert users == {e for c in CELLS for e in c.entries} and len(users) == 2
    # ... and the binding module itself asks for no stream (tests/test_stream_contract_cpu.py walks it)
    src = open(os.path.join(C.ROOT, "nnmnkwii_amd", "_trajectory_hip.py")).read()
    assert "_stream" not in src


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_case_pairs_tell_a_stale_replay_from_a_fresh_one(cell):
    assert SC.pair_conditions(cell) == []
