"""Objective metrics on the device: nnmk_metrics_batch (csrc/frame_metrics.hip) against the numpy specification
tools/metrics_model.py through the C entry on guarded buffers -- payloads at odd element offsets, inputs snapshotted, workspaces
of exact size, pad frames and the columns no term reads holding NaN -- then the four functions of ``nnmnkwii_amd.metrics`` and
``batch_metrics`` on CUDA tensors against what the reference gave (tests/golden/metrics_ref.npz).

Bounds (tools/metrics_model.py).  Counts: equal.  Sums against the model's kernel order: the same bits (every operation is a
separately rounded IEEE operation in the same order; terms with the EXP flag: within the two exponentials' share of the bound).
Against the truth: (longest addition chain of the shape + 4) 2^-53, plus 2 * 21 * 2 units for EXP.  Against the reference's
values: twice that for float64 inputs, the reference's own float32 error for float32 inputs (tests/metrics_cases.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import metrics_cases as C
from embed import Embedded, Workspace, embedded, failed
from metrics_cases import MM

pytestmark = pytest.mark.gpu

BLOCK = C.BLOCK
G = C.golden()
DTYPES = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)]
SHAPES = [(B, Tmax) for B in (1, 3, 5) for Tmax in (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3)]

p = lambda b: None if b is None else ctypes.c_void_p(b.ptr())  # noqa: E731


def _lib():
    from nnmnkwii_amd import _metrics_hip
    return _metrics_hip.lib()


def _counts():
    L = _lib()
    return [L.mlpg_hip_launch_count(k) for k in range(44)] + [L.nnmk_metrics_launch_count()]


def run_batch(X, Y, lengths, terms, off=1, per_utt=True):
    """One call of nnmk_metrics_batch on guarded buffers; X's and Y's last dimensions are the row strides.  Returns (totals,
    per_utt) as numpy; checks the return code, the guards, that the inputs are unchanged and that the call was counted once."""
    from nnmnkwii_amd import _hip, _metrics_hip as M
    L = _lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, Tmax = X.shape[:2]
    n = len(terms)
    ins = dict(x=embedded(X, off), y=embedded(Y, off + 2))
    if lengths is not None:
        ins["lengths"] = embedded(np.asarray(lengths, dtype=np.int32), off)
    totals = Embedded((n, 2), np.float64, off)
    per = Embedded((B, n, 2), np.float64, off) if per_utt else None
    nbytes = L.nnmk_metrics_workspace(B, Tmax, n)
    ws = Workspace(nbytes)
    arr = (M.Term * n)(*[M.term(**{k: (None if k == "threshold" and v != v else v) for k, v in t.items()}) for t in terms])
    c0 = _counts()
    rc = L.nnmk_metrics_batch(dev.index, _hip._stream(dev), int(X.dtype == np.float64), p(ins["x"]), X.shape[2], int(Y.dtype == np.float64),
                              p(ins["y"]), Y.shape[2], p(ins.get("lengths")), B, Tmax, arr, n, p(per), p(totals), p(ws), nbytes)
    torch.cuda.synchronize()
    d = [b - a for a, b in zip(c0, _counts())]
    assert rc == 0, (rc, L.mlpg_hip_last_error())
    assert d[-1] == 1 and sum(d) == 1, d
    bad = failed(ins, dict(totals=totals, per_utt=per), dict(workspace=ws))
    assert not bad, bad
    return totals.host(), (per.host() if per_utt else None)


def lengths_of(B, Tmax):
    return {1: None, 3: [Tmax, 0, 1], 5: [1, Tmax, 0, Tmax // 2 + 1, max(Tmax - 1, 0)]}[B]


@functools.lru_cache(maxsize=None)
def case(B, Tmax, k):
    """Eight terms inside 187-wide rows of x and 190-wide rows of y; the model's kernel order, computed once."""
    dtype_x, dtype_y = DTYPES[k]
    terms = C.eight_terms()
    lengths = lengths_of(B, Tmax)
    X, Y, L = C.kernel_case(100 * B + Tmax, lengths if lengths is not None else [Tmax] * B, Tmax, 187, dtype_x, dtype_y, terms)
    Y = np.concatenate([Y, np.full(Y.shape[:2] + (3,), np.nan, dtype=Y.dtype)], axis=2)
    L = None if lengths is None else L
    return X, Y, L, terms, MM.kernel_order(X, Y, L, terms)


@pytest.mark.parametrize("B,Tmax", SHAPES)
def test_kernel_against_the_model_and_the_truth(B, Tmax):
    k = SHAPES.index((B, Tmax)) % 3                  # every dtype pair meets every B and one-block and many-block shapes
    X, Y, L, terms, model = case(B, Tmax, k)
    totals, per_utt = run_batch(X, Y, L, terms, off=1 + 2 * (B % 2))
    worst = C.check_against_model(totals, per_utt, X, Y, L, terms, model)
    print("against the truth: worst error / bound %.3f" % worst)
    if L is not None:
        assert not per_utt[np.asarray(L) == 0].any()             # the empty utterance: zeros


@pytest.mark.parametrize("k", [0, 1, 2])
def test_same_bits_on_every_call(k):
    X, Y, L, terms, model = case(5, 2 * BLOCK + 3, k)
    first = run_batch(X, Y, L, terms, off=1)
    other = case(3, BLOCK, (k + 1) % 3)
    run_batch(*other[:4])
    again = run_batch(X, Y, L, terms, off=3)
    assert np.array_equal(first[0].view(np.int64), again[0].view(np.int64)) and np.array_equal(first[1].view(np.int64), again[1].view(np.int64))
    only_totals, none = run_batch(X, Y, L, terms, per_utt=False)
    assert none is None and np.array_equal(only_totals.view(np.int64), first[0].view(np.int64))


def test_an_utterance_alone_and_inside_a_batch():
    X, Y, L, terms, _ = case(5, 2 * BLOCK + 3, 1)
    _, per_utt = run_batch(X, Y, L, terms)
    for b in (0, 1, 3):
        n = int(L[b])
        totals, alone = run_batch(np.ascontiguousarray(X[b:b + 1, :n]), np.ascontiguousarray(Y[b:b + 1, :n]), None, terms, off=3)
        assert np.array_equal(alone[0].view(np.int64), per_utt[b].view(np.int64)), b
        assert np.array_equal(totals.view(np.int64), alone[0].view(np.int64))


def test_empty_batches_and_utterances():
    X, Y, L, terms, _ = case(3, BLOCK + 1, 0)
    totals, per_utt = run_batch(X, Y, np.array([0, -5, 0], dtype=np.int32), terms)
    assert not totals.any() and not per_utt.any()
    totals, per_utt = run_batch(X[:0], Y[:0], L[:0], terms)                     # B == 0 still writes the totals
    assert totals.shape == (8, 2) and not totals.any() and per_utt.size == 0
    totals, per_utt = run_batch(X[:, :0], Y[:, :0], None, terms)                # Tmax == 0
    assert not totals.any() and per_utt.shape == (3, 8, 2) and not per_utt.any()
    beyond, _ = run_batch(X, Y, np.array([BLOCK + 1000, 0, 1], dtype=np.int32), terms)     # lengths above Tmax count as Tmax
    want, _ = run_batch(X, Y, L, terms)
    assert np.array_equal(beyond.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("name", sorted(C.G_CASES))
def test_the_reference_s_values_through_the_c_entry(name):
    X, Y, L = G[name + "/X"], G[name + "/Y"], G[name + "/lengths"]
    terms = C.golden_terms()
    live = MM.live_frames(L, len(L), X.shape[1])
    totals, per_utt = run_batch(C.pad_with(X, live), C.pad_with(Y, live), L, list(terms.values()))
    C.check_against_model(totals, per_utt, X, Y, L, list(terms.values()))
    for i, (key, t) in enumerate(terms.items()):
        want = float(G["%s/%s" % (name, key)])
        rel = C.reference_bound(len(L), X.shape[1], t, X.dtype) + 3 * C.U       # the figure's own division, root and scaling
        assert C.close(C.figure(key, totals[i]), want, rel), (key, C.figure(key, totals[i]), want)


def _figure_bound(key, B, Tmax, dtype, width):
    kind = {"melcd": MM.FRAME_L2, "mse": MM.SQUARED, "lf0": MM.VOICED_SQUARED, "vuv": MM.MISMATCH}[key.split("/")[0]]
    t = MM.term(kind, 0, width=width, flags=MM.FLAG_EXP if key.endswith("linear") else 0)
    return C.reference_bound(B, Tmax, t, dtype) + 3 * C.U


@pytest.mark.parametrize("name", sorted(C.G_CASES))
def test_public_functions_on_cuda_tensors(name):
    from nnmnkwii_amd import metrics
    L = _lib()
    Xh, Yh, lengths = G[name + "/X"], G[name + "/Y"], G[name + "/lengths"]
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    c0 = L.nnmk_metrics_launch_count()
    got = C.golden_calls(metrics, X, Y, lengths)
    assert L.nnmk_metrics_launch_count() - c0 == len(got)              # one call each, the lf0 ones included
    for key, value in got.items():
        want = float(G["%s/%s" % (name, key)])
        width = {"melcd/lengths": 11, "melcd/utterance": 11, "melcd/frame": 11, "mse/batch": 11}.get(key, 3 if key.startswith("mse") else 1)
        assert isinstance(value, float) and C.close(value, want, _figure_bound(key, len(lengths), Xh.shape[1], Xh.dtype, width)), (key, value, want)
    # lengths on the device, as a tensor; f0 and vuv from separate tensors (stacked) against columns of one tensor (addressed in place)
    Ld = torch.from_numpy(lengths).cuda()
    f0x, vx, f0y, vy = (t[:, :, c].contiguous() for t, c in ((X, C.G_LF0), (X, C.G_VUV), (Y, C.G_LF0), (Y, C.G_VUV)))
    assert metrics.lf0_mean_squared_error(f0x, vx, f0y, vy, Ld) == got["lf0/lengths"]
    assert metrics.lf0_mean_squared_error(X[:, :, C.G_VUV - 1], X[:, :, C.G_VUV], Y[:, :, C.G_LF0], Y[:, :, C.G_LF0 + 1], Ld, True) == got["lf0/lengths_linear"]
    # the whole evaluation in one call
    terms = {"mcd": ("melcd", C.G_MGC), "bap": ("mse", C.G_BAP), "lf0": ("lf0_mse", C.G_LF0, C.G_VUV), "lf0_hz": ("lf0_mse", C.G_LF0, C.G_VUV, True),
             "vuv": ("vuv_error", C.G_VUV)}
    c0 = L.nnmk_metrics_launch_count()
    one = metrics.batch_metrics(X, Y, Ld, terms)
    per = metrics.batch_metrics(X, Y, lengths, terms, per_utterance=True)
    assert L.nnmk_metrics_launch_count() - c0 == 2
    host = metrics.batch_metrics(Xh, Yh, lengths, terms)
    host_per = metrics.batch_metrics(Xh, Yh, lengths, terms, per_utterance=True)
    for k, key in (("mcd", "melcd/lengths"), ("bap", "mse/lengths"), ("lf0", "lf0/lengths"), ("lf0_hz", "lf0/lengths_linear"), ("vuv", "vuv/lengths")):
        t = list(C.golden_terms().values())[["melcd/lengths", "melcd/one_feature", "mse/lengths", "lf0/lengths", "lf0/lengths_linear", "vuv/lengths"].index(key)]
        rel = 2 * MM.bound(len(lengths), Xh.shape[1], t) + 3 * C.U       # device order against the host's numpy order
        assert one[k] == got[key], k                                       # the same term alone and among five: the same bits
        assert C.close(one[k], host[k], rel), (k, one[k], host[k])
        assert per[k].shape == (len(lengths),) and C.close(per[k], host_per[k], rel), (k, per[k], host_per[k])


def test_threshold_rules_on_cuda_tensors():
    from nnmnkwii_amd import metrics
    x = torch.tensor([[[5.0, 0.9], [5.1, 0.4], [5.2, 0.8]]], device="cuda")
    y = torch.tensor([[[5.5, 0.7], [5.0, 0.6], [5.0, 0.2]]], device="cuda", dtype=torch.float64)
    r = metrics.batch_metrics(x, y, None, {"lf0": ("lf0_mse", 0, 1), "vuv": ("vuv_error", 1)}, vuv_threshold=0.5)
    assert r["lf0"] == 0.5 and r["vuv"] == 2.0 / 3.0
    r = metrics.batch_metrics(x, y, None, {"lf0": ("lf0_mse", 0, 1), "vuv": ("vuv_error", 1)})
    assert np.isnan(r["lf0"]) and r["vuv"] == 1.0
    assert np.isnan(metrics.mean_squared_error(x, y.float(), [0]))


@pytest.mark.parametrize("width,dtype", [(1000, np.float64), (128, np.float64), (2000, np.float32)])
def test_the_widest_spans_the_entry_accepts(width, dtype):
    """1000 float64 (2000 float32) columns of x and of y are NNMK_METRICS_MAX_ROW_BYTES: one frame staged per wave, all of the
    workgroup's LDS; 128 float64 columns: a slab of 2 KB, seven frames staged."""
    terms = [MM.term(MM.FRAME_L2, 0, width=width), MM.term(MM.SQUARED, 0, width=width), MM.term(MM.MISMATCH, 0, width=width)]
    X, Y = C.pair(width, 2, 9, width, dtype)
    L = np.array([9, 6], dtype=np.int32)
    X, Y = C.pad_with(X, L), C.pad_with(Y, L)
    Y[0, 3, 5::7] = X[0, 3, 5::7]                      # some equal elements for the mismatch count
    totals, per_utt = run_batch(X, Y, L, terms)
    C.check_against_model(totals, per_utt, X, Y, L, terms)
    assert 0 < totals[2, 0] < totals[2, 1] == 15 * width
