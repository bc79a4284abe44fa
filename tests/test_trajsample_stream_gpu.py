"""GPU tests (-m gpu): the stream contract of include/nnmnkwii_sample.h -- every launch on the caller's stream, no
synchronisation, no allocation, no default-stream work -- with the checks of tests/stream_contract.py that
tests/test_stream_contract_gpu.py applies to the other families: captured on a side stream and replayed on new data behind the
same pointers, two streams interleaved, and behind a late producer.  The wrappers that hand the stream on live in
nnmnkwii_amd/_sample_calls.py; the walk at the end finds every function there that asks for the stream and wants a cell for it
(it needs no device, but sits here beside the table it checks)."""
import ast
import os

import numpy as np
import pytest
import torch

import stream_contract as SC
import trajcov_cases as C
import trajsample_cases as S
from trajcov_cases import TM
from trajsample_cases import SM

K, B, TMAX, SD, WNAME = 5, 3, 70, 65, "std3"
WIN = C.WINDOWS[WNAME]
D = len(WIN) * SD
LENGTHS = {1: [70, 0, 33], 2: [5, 70, 64]}


def make(seed):
    lengths = LENGTHS[seed]
    var, noise, mean = S.inputs(seed, K, B, TMAX, SD, WNAME, TM.VAR_FRAME, np.float64, lengths)
    return dict(var=np.nan_to_num(var, nan=1.0), noise=np.nan_to_num(noise), mean=np.nan_to_num(mean), lengths=np.array(lengths, dtype=np.int32))


def want(c):
    """(factor, logdet, status, draws, whitened draws) of the model, and 2^-53 cond_2(R) per system."""
    if "_want" not in c:
        fac, logdet, status = SM.factor_batch(c["var"], WIN, c["lengths"], B, TMAX, SD)
        x = SM.sample_batch(fac, status, c["lengths"], c["noise"], c["mean"])
        z = SM.whiten_batch(fac, status, c["lengths"], x, c["mean"])
        c["_want"] = (fac, logdet, status, x, z)
        c["_unit"] = S.units(c["var"], WNAME, c["lengths"], B, TMAX, SD)
    return c["_want"]


def bound_fails(c, name, t, ref):
    want(c)
    try:
        S.within_bound(t.cpu().numpy(), ref, c["_unit"], c["lengths"], False)
    except AssertionError as e:
        return ["%s is outside the bound of the model: %s" % (name, e)]
    return []


def load_factor(b, c):
    SC.put(b, "in_var", c["var"])
    SC.put(b, "in_idx_lengths", c["lengths"])
    SC.out(b, "out_factor", (3, B, TMAX, SD), torch.float64)
    SC.out(b, "out_logdet", (B, SD), torch.float64)
    SC.out(b, "out_status", (B, SD), torch.int32)


def call_factor(b):
    from nnmnkwii_amd import _sample_calls as calls
    calls.factor(b["in_var"], WIN, b["in_idx_lengths"], B, TMAX, D, factor=b["out_factor"], logdet=b["out_logdet"], status=b["out_status"])


def verdict_factor(c, b):
    fac, logdet, status = want(c)[:3]
    fails = ["%s differs from the model" % n for n, t, w in (("factor", b["out_factor"], fac), ("status", b["out_status"], status))
             if not C.same_bits(t.cpu().numpy(), w)]
    got = b["out_logdet"].cpu().numpy()
    live = TM.live_frames(c["lengths"], B, TMAX)
    for u in range(B):
        if not (np.abs(got[u] - logdet[u]) <= C.logdet_bound(c["var"][u], WNAME, int(live[u]), SD)).all():
            fails.append("logdet of utterance %d is outside the bound" % u)
    return fails


def load_draw(src):
    def load(b, c):
        w = want(c)
        SC.put(b, "in_factor", w[0])
        SC.put(b, "in_status", w[2])
        SC.put(b, "in_idx_lengths", c["lengths"])
        SC.put(b, "in_src", c["noise"] if src == "noise" else w[3])
        SC.put(b, "in_mean", c["mean"])
        SC.out(b, "out_draws", (K, B, TMAX, SD), torch.float64)
    return load


def call_sample(b):
    from nnmnkwii_amd import _sample_calls as calls
    calls.sample(b["in_factor"], b["in_status"], b["in_idx_lengths"], b["in_src"], b["in_mean"], out=b["out_draws"])


def call_whiten(b):
    from nnmnkwii_amd import _sample_calls as calls
    calls.whiten(b["in_factor"], b["in_status"], b["in_idx_lengths"], b["in_src"], b["in_mean"], out=b["out_draws"])


CELLS = [SC.Cell("sample.factor", ["_sample_calls.factor"], make, load_factor, call_factor, verdict_factor,
                 expected=lambda c: list(want(c)[:2])),          # (the status is 0 in both cases)
         SC.Cell("sample.sample", ["_sample_calls.sample"], make, load_draw("noise"), call_sample,
                 lambda c, b: bound_fails(c, "draws", b["out_draws"], want(c)[3]), expected=lambda c: [want(c)[3]]),
         SC.Cell("sample.whiten", ["_sample_calls.whiten"], make, load_draw("x"), call_whiten,
                 lambda c, b: bound_fails(c, "whitened rows", b["out_draws"], want(c)[4]), expected=lambda c: [want(c)[4]])]


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
def test_all_entries_back_to_back_on_one_stream():
    SC.one_stream_shared(CELLS)


# ---- completeness and sharpness (no device) ---------------------------------------------------------------------------------------

def test_every_wrapper_that_takes_the_stream_has_a_cell():
    path = os.path.join(C.ROOT, "nnmnkwii_amd", "_sample_calls.py")
    tree = ast.parse(open(path).read(), path)
    users = set()
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            for node in ast.walk(fn):
                f = getattr(node, "func", None)
                if isinstance(node, ast.Call) and ((isinstance(f, ast.Name) and f.id == "_stream") or (isinstance(f, ast.Attribute) and f.attr == "_stream")):
                    users.add("_sample_calls." + fn.name)
    assert users == {e for c in CELLS for e in c.entries} and len(users) == 3
    # ... and the binding module itself asks for no stream (tests/test_stream_contract_cpu.py walks it)
    src = open(os.path.join(C.ROOT, "nnmnkwii_amd", "_sample_hip.py")).read()
    assert "_stream" not in src


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_case_pairs_tell_a_stale_replay_from_a_fresh_one(cell):
    assert SC.pair_conditions(cell) == []
