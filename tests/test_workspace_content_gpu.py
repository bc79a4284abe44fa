"""The content of a caller's workspace is irrelevant (-m gpu): every entry that takes one -- the joint rows (count + write),
metrics_batch, column_stats, gmm_estep with its mean, gmm_mstep, kmeans_seed_step, kmeans_lloyd_step -- gives the same bytes on

(a) a fresh zeroed workspace,  (b) one of 0xFF bytes,  (c) one of float64 NaN,
(d) one a previous call of a LARGER case left behind,  (e) one a SMALLER case left behind, allocated for this case,

and passes its family's verdict on each.  An entry that reads a word it did not write in this call is right on (a) and wrong on the
others; ``mixture.py`` keeps one workspace across every iteration and shape of a fit.  The workspace is never larger than what the
entry's ``*_workspace*`` query asks for at the case's shape, so the query is exercised at that shape too."""
import numpy as np
import pytest
import torch

import stream_contract as SC
import test_stream_contract_gpu as T

pytestmark = pytest.mark.gpu

MAIN, LARGER, SMALLER = 1, 3, 4            # the seeds of a family's cases: its stream cell's case A, a larger batch, a smaller one


class Entry(object):
    """One entry with a workspace: make / load / call / verdict as in a stream cell, and ``need(case)``: the query's bytes."""

    def __init__(self, name, make, load, call, verdict, need):
        self.name, self.make, self.load, self.call, self.verdict, self.need = name, make, load, call, verdict, need


def _joint_need(c):
    from nnmnkwii_amd import _joint_hip as JH
    return int(JH.lib().nnmk_joint_workspace_bytes(c["X"].shape[0], c["X"].shape[1]))


def _metrics_need(c):
    from nnmnkwii_amd import _metrics_hip as M
    return M.metrics_workspace(c["X"].shape[0], c["X"].shape[1], len(c["terms"]))


def _gmm_need(c):
    from nnmnkwii_amd import _hip
    return int(_hip.lib().mlpg_hip_gmm_workspace_bytes(c["X"].shape[0], c["X"].shape[1], c["means"].shape[0]))


def _kmeans_need(K):
    def need(c):
        from nnmnkwii_amd import _hip
        return int(_hip.lib().mlpg_hip_kmeans_workspace_bytes(c["X"].shape[0], c["X"].shape[1], K or c["centers"].shape[0]))
    return need


GMM_N = {MAIN: 131, LARGER: 300, SMALLER: 70}


# ---- column_stats: bits of the model's state, and tests/norm_cases.py's stats_ok against the exact statistics ---------------------------

def colstats_case(seed):
    import norm_cases as C
    from norm_cases import NM
    BLOCK = NM.BLOCK_ROWS
    lens = {MAIN: [2 * BLOCK + 3, 0, BLOCK + 1], LARGER: [3 * BLOCK + 4, 1, BLOCK, 2 * BLOCK + 3, 17], SMALLER: [100, 17]}[seed]
    X, L = C.padded(600 + seed, lens, 65)
    return dict(X=X, L=L, state=NM.kernel_state(X, L), truth=NM.exact(X, L))


def colstats_load(b, c):
    SC.put(b, "in_x", c["X"])
    SC.put(b, "in_lengths", c["L"])
    SC.out(b, "out_state", (5, c["X"].shape[2]), torch.float64)


def colstats_call(b):
    from nnmnkwii_amd import _hip
    _hip.column_stats(b["in_x"], b["in_lengths"], None, b["out_state"], b["ws"])


def colstats_verdict(c, b):
    import norm_cases as C
    state = T.host(b["out_state"])
    return ([] if T.same_bits(state, c["state"]) else ["the model's bits"]) + ([] if C.stats_ok(state, c["truth"]) else ["stats_ok"])


def _colstats_need(c):
    from nnmnkwii_amd import _hip
    return _hip.column_stats_workspace(*c["X"].shape)


ENTRIES = [
    Entry("joint.count+write", T.joint_case, T.joint_load, T.joint_call, T.joint_verdict, _joint_need),
    Entry("metrics_batch", T.metrics_case, T.metrics_load, T.metrics_call, T.metrics_verdict, _metrics_need),
    Entry("column_stats", colstats_case, colstats_load, colstats_call, colstats_verdict, _colstats_need),
    Entry("gmm_estep", lambda s: T.gmm_case(s, GMM_N[s]), T.gmm_estep_load, T.gmm_estep_call, T.gmm_estep_verdict, _gmm_need),
    Entry("gmm_mstep", lambda s: T.gmm_case(s, GMM_N[s]), T.gmm_mstep_load, T.gmm_mstep_call, T.gmm_mstep_verdict, _gmm_need),
    Entry("kmeans_seed_step", lambda s: T.kmeans_case(s, GMM_N[s]), T.kmeans_load, T.kmeans_seed_call, T.kmeans_seed_verdict, _kmeans_need(1)),
    Entry("kmeans_lloyd_step", lambda s: T.kmeans_case(s, GMM_N[s]), T.kmeans_load, T.kmeans_lloyd_call, T.kmeans_lloyd_verdict, _kmeans_need(0)),
]


def run(entry, case, ws, what):
    """One call of the entry on `case` with the workspace `ws`; the verdict; the bytes of every input and output."""
    bufs = {"ws": ws}
    entry.load(bufs, case)
    for _, t in SC._tensors(bufs, "out_"):
        SC.fill_bytes(t, SC.POISON)
    entry.call(bufs)
    torch.cuda.synchronize()
    assert bufs["ws"] is ws
    fails = entry.verdict(case, bufs)
    assert not fails, (entry.name, what, fails)
    return SC.snapshot(bufs)


def fresh(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_the_content_of_the_workspace_is_irrelevant(entry):
    main, larger, smaller = entry.make(MAIN), entry.make(LARGER), entry.make(SMALLER)
    need, need_larger, need_smaller = entry.need(main), entry.need(larger), entry.need(smaller)
    assert need_smaller <= need <= need_larger and need > 0 and need % 8 == 0, (need_smaller, need, need_larger)
    results = {"zeroed": run(entry, main, fresh(need), "zeroed")}
    ws = fresh(need)
    ws.fill_(0xFF)
    results["0xFF"] = run(entry, main, ws, "0xFF")
    ws = fresh(need)
    ws.view(torch.float64).fill_(float("nan"))
    results["NaN"] = run(entry, main, ws, "NaN")
    big = fresh(need_larger)
    run(entry, larger, big, "the larger case itself")
    results["after a larger case"] = run(entry, main, big[:need], "after a larger case")
    ws = fresh(need)
    run(entry, smaller, ws, "the smaller case itself")
    results["after a smaller case"] = run(entry, main, ws, "after a smaller case")
    for name, snap in results.items():
        assert SC.differing(snap, results["zeroed"]) == [], (entry.name, name, SC.differing(snap, results["zeroed"]))


def test_a_planted_entry_that_trusts_its_workspace_is_caught():
    """A stand-in whose second stage adds to a workspace word the first stage never cleared: right on a zeroed workspace, caught on
    the first dirty one."""
    def make(seed):
        x = np.random.RandomState(300 + seed).randn({MAIN: 64, LARGER: 96, SMALLER: 16}[seed], 8)
        return dict(x=x, ref=x.sum(axis=0))

    def load(b, c):
        SC.put(b, "in_x", c["x"])
        SC.out(b, "out_sum", (8,), torch.float64)

    def call(b):
        acc = b["ws"].view(torch.float64)[:8]
        acc += b["in_x"].sum(dim=0)                     # (the planted bug: no acc.zero_() in front)
        b["out_sum"].copy_(acc)
        acc.zero_()

    def verdict(c, b):
        return [] if np.allclose(T.host(b["out_sum"]), c["ref"], rtol=1e-12, atol=1e-12) else ["sum"]

    entry = Entry("planted", make, load, call, verdict, lambda c: 8 * c["x"].shape[0])
    with pytest.raises(AssertionError, match="0xFF"):
        test_the_content_of_the_workspace_is_irrelevant(entry)
