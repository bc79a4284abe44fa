"""GPU tests (-m gpu) of the modulation-spectrum filter (csrc/modspec_filter.hip, postfilters.modspec_post_filter_batch,
preprocessing.modspec_smoothing_batch) against the numpy model tools/msfilter_model.py -- the literal definition; the model is
never compared against the kernel.  Bounds, relative to the reference array's maximum: those of the two-transform route of the
padded-minibatch modulation spectrum (tests/test_modspec_batch_gpu.py), 1e-10 in float64 and 5e-6 in float32, where the reference
is evaluated in float64 on the float32-rounded inputs.  Two conditions on the inputs are asserted on the reference: over the
removed bins |S| is at least 1e-6 of the column's largest |S| (so that the phase the log domain keeps is well conditioned), and the
gains exp(C / 2) lie within [1/16, 16]."""
import os
import sys

import numpy as np
import pytest
import torch

import modspec_batch64 as R
from embed import Embedded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import msfilter_model as MM  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
BOUND = {F64: 1e-10, F32: 5e-6}
TORCH_DT = {F32: torch.float32, F64: torch.float64}
KIND = 31
B = 4


def _counts():
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return [L.mlpg_hip_launch_count(k) for k in range(32)]


def _moved(c0):
    return {k: b - a for k, (a, b) in enumerate(zip(c0, _counts())) if a != b}


def _lengths(n, Tmax):
    return [n, 1, 0, n - 1] if n <= 4 else [Tmax, n // 2 + 1, 0, (3 * n) // 4]


def _tables(rng, nb, D):
    """A in [0.43, 2.7] (sigma_N / sigma_G between 1/3 and 3 at k = 0.85); gains exp(C / 2) within [1/16, 16]."""
    A, C = rng.uniform(0.43, 2.7, (nb, D)), rng.uniform(-2 * np.log(16.0), 2 * np.log(16.0), (nb, D))
    g = np.exp(0.5 * C)
    assert g.min() >= 1 / 16.0 and g.max() <= 16.0
    return A, C


def _modes(nb):
    """(tables?, limit_bin, log_domain): tables only, removal only and both in either domain at every limit_bin, neither."""
    modes = [(True, nb, True), (False, nb, True)]
    for tabs in (False, True):
        for log_domain in (True, False):
            modes += [(tabs, lb, log_domain) for lb in sorted({0, 1, nb - 1})]
    return modes


def _phase_condition(x, live, n):
    """min over every bin of |S| / the column's largest |S|, over the live utterances (the removed bins are a subset)."""
    worst = 1.0
    for b in range(len(live)):
        if live[b]:
            mag = np.abs(np.fft.rfft(x[b, :live[b]].astype(F64), n=n, axis=0))
            worst = min(worst, float((mag.min(axis=0) / mag.max(axis=0)).min()))
    return worst


def _err(got, ref):
    return float(np.abs(np.asarray(got, dtype=F64) - ref).max() / np.abs(ref).max())


def _check_rows(got, live):
    for b in range(len(live)):
        assert not got[b, live[b]:].any() and not np.signbit(got[b, live[b]:]).any(), b   # exact (positive) zeros from live_b on


@pytest.mark.parametrize("dt", (F64, F32))
@pytest.mark.parametrize("n", (2, 4, 16, 64, 256, 4096))
def test_parity_grid(n, dt):
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda")
    nb = n // 2 + 1
    rng = np.random.RandomState(1000 + n)
    worst, worst_cond, calls = 0.0, 1.0, 0
    c0 = _counts()
    for Tmax in ((n, n - 3) if n >= 16 else (n,)):
        for D in (1, 4, 5):
            A, C = _tables(rng, nb, D)
            At, Ct = torch.from_numpy(A).to(dev), torch.from_numpy(C).to(dev)
            for lengths in (_lengths(n, Tmax), None):
                x = R.make_batch(rng, B, Tmax, D, lengths).astype(dt)          # NaN from each length on
                live = MM.live_frames(lengths, B, Tmax)
                cond = _phase_condition(x, live, n)
                worst_cond = min(worst_cond, cond)
                assert cond >= 1e-6, (n, Tmax, D, lengths, cond)
                xt = torch.from_numpy(x).to(dev)
                lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
                for norm in (None, "ortho"):
                    for tabs, limit_bin, log_domain in _modes(nb):
                        a, c = (A, C) if tabs else (None, None)
                        ref = MM.filter_batch(x, n, norm, lengths, a, c, limit_bin, log_domain)
                        got = _hip.modspec_filter(xt, n, At if tabs else None, Ct if tabs else None, limit_bin, log_domain,
                                                  norm == "ortho", lengths=lt)
                        calls += 1
                        assert got.dtype == TORCH_DT[dt] and got.shape == (B, Tmax, D) and got.is_cuda
                        got = got.cpu().numpy()
                        what = (n, Tmax, D, lengths is not None, norm, tabs, limit_bin, log_domain)
                        assert np.isfinite(got).all(), what
                        _check_rows(got, live)
                        if lengths is not None:
                            assert not got[2].any(), what                     # the utterance of length 0
                        if not np.abs(ref).max():
                            assert not got.any(), what                        # every bin removed outside the log domain
                            continue
                        e = _err(got, ref)
                        worst = max(worst, e)
                        assert e <= BOUND[dt], what + (e,)
    assert _moved(c0) == {KIND: calls}
    print("msfilter n=%d %s: worst %.2e of the maximum over %d calls; min|S|/max|S| >= %.1e" % (n, dt.__name__, worst, calls, worst_cond))


def test_neither_is_the_identity_and_one_call_is_one_launch():
    from nnmnkwii_amd import _hip, postfilters as PF
    dev = torch.device("cuda")
    rng = np.random.RandomState(5)
    n, Tmax, D = 64, 61, 5
    lengths = _lengths(n, Tmax)
    x = R.make_batch(rng, B, Tmax, D, lengths)
    for dt in (F64, F32):
        xt = torch.from_numpy(x.astype(dt)).to(dev)
        c0 = _counts()
        y = PF.modspec_post_filter_batch(xt, None, None, n=n, lengths=lengths)
        assert _moved(c0) == {KIND: 1}
        assert torch.is_tensor(y) and y.is_cuda and y.dtype == TORCH_DT[dt] and y.data_ptr() != xt.data_ptr()
        want = np.nan_to_num(x.astype(dt)).astype(F64)
        assert _err(y.cpu().numpy(), want) <= BOUND[dt]
        # two calls: the same bits
        assert torch.equal(y, PF.modspec_post_filter_batch(xt, None, None, n=n, lengths=lengths))
    assert _hip.modspec_filter_form(n) == 1 and _hip.modspec_filter_form(100) == 0


@pytest.mark.parametrize("dt", (F64, F32))
def test_in_place_on_a_column_slice_between_guards(dt):
    """The D = 5 columns [3, 8) of an 11-column tensor, filtered where they lie: the other columns and the guard bands keep their
    bits, and the result is the out-of-place result bit for bit."""
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda")
    rng = np.random.RandomState(11)
    n, Tmax, D, ld, col = 256, 253, 5, 11, 3
    nb = n // 2 + 1
    lengths = _lengths(n, Tmax)
    live = MM.live_frames(lengths, B, Tmax)
    A, C = _tables(rng, nb, D)
    At, Ct = torch.from_numpy(A).to(dev), torch.from_numpy(C).to(dev)
    lt = torch.tensor(lengths, dtype=torch.int32, device=dev)
    x = R.make_batch(rng, B, Tmax, D, lengths).astype(dt)
    wide = rng.randn(B, Tmax, ld).astype(dt)
    wide[:, ::7, 0] = np.nan                                   # NaN next to the slice reaches nothing either
    wide[..., col:col + D] = x
    limit_bin = 40
    ref = MM.filter_batch(x, n, "ortho", lengths, A, C, limit_bin, True)
    iview = torch.int64 if dt == F64 else torch.int32
    for offset in (0, 1):                                      # the payload on and off a 256-byte boundary
        buf = Embedded((B, Tmax, ld), dt, offset_elems=offset, device=dev).put(wide)
        before = buf.payload().clone()
        view = buf.payload()[..., col:col + D]
        apart = _hip.modspec_filter(view, n, At, Ct, limit_bin, True, True, lengths=lt)
        assert buf.unchanged() and buf.guards_ok()             # out of place: the input keeps its bits
        c0 = _counts()
        r = _hip.modspec_filter(view, n, At, Ct, limit_bin, True, True, lengths=lt, out=view)
        assert _moved(c0) == {KIND: 1}
        assert r.data_ptr() == view.data_ptr() and buf.guards_ok()
        after = buf.payload()
        for sl in (slice(0, col), slice(col + D, ld)):
            assert torch.equal(after[..., sl].contiguous().view(iview), before[..., sl].contiguous().view(iview))
        assert torch.equal(after[..., col:col + D].contiguous().view(iview), apart.contiguous().view(iview))
        got = apart.cpu().numpy()
        assert _err(got, ref) <= BOUND[dt]
        _check_rows(got, live)


@pytest.mark.parametrize("route", ("n=100", "n=1000", "direct"))
def test_the_composed_route(route):
    """Lengths the launch does not take go through modspec / inv_modspec in float64: the same values, no launch of kind 31."""
    from nnmnkwii_amd import _hip, postfilters as PF, preprocessing as PP
    dev = torch.device("cuda")
    rng = np.random.RandomState(21)
    L = _hip.lib()
    n = {"n=100": 100, "n=1000": 1000, "direct": 64}[route]
    nb = n // 2 + 1
    Tmax, D, modfs = n - 3, 5, 200
    lengths = _lengths(n, Tmax)
    live = MM.live_frames(lengths, B, Tmax)
    A, C = _tables(rng, nb, D)
    if route == "direct":
        L.mlpg_hip_modspec_set_direct(1)
    try:
        assert _hip.modspec_filter_form(n) == 0
        c0 = _counts()
        for dt in (F64, F32):
            x = R.make_batch(rng, B, Tmax, D, lengths).astype(dt)
            assert _phase_condition(x, live, n) >= 1e-6
            xt = torch.from_numpy(x).to(dev)
            for norm in (None, "ortho"):
                for a, c, cutoff, log_domain in ((A, C, None, True), (None, None, 30, True), (None, None, 30, False), (A, C, 30, True),
                                                 (A, C, 30, False), (None, None, None, True)):
                    limit_bin = MM.limit_bin_of(n, modfs, cutoff)
                    ref = MM.filter_batch(x, n, norm, lengths, a, c, limit_bin, log_domain)
                    got = PF.modspec_post_filter_batch(xt, a, c, n=n, norm=norm, lengths=lengths, modfs=modfs, cutoff=cutoff,
                                                       log_domain=log_domain)
                    assert got.dtype == TORCH_DT[dt] and got.is_cuda
                    got = got.cpu().numpy()
                    assert _err(got, ref) <= BOUND[dt], (route, dt.__name__, norm, cutoff, log_domain, _err(got, ref))
                    _check_rows(got, live)
                    assert not got[2].any()
            ref = MM.filter_batch(x, n, None, lengths, None, None, MM.limit_bin_of(n, modfs, 30), True)
            got = PP.modspec_smoothing_batch(xt, modfs, n=n, cutoff=30, lengths=lengths).cpu().numpy()
            assert _err(got, ref) <= BOUND[dt]
        assert KIND not in _moved(c0)
    finally:
        L.mlpg_hip_modspec_set_direct(0)
    assert _hip.modspec_filter_form(64) == 1


def test_smoothing_batch_agrees_with_the_existing_smoothing_and_the_padded_loop_is_one_launch():
    from nnmnkwii_amd import preprocessing as PP, util
    rng = np.random.RandomState(31)
    modfs = 200
    for n, Tmax, D in ((64, 64, 4), (256, 200, 5), (4096, 4000, 3)):
        x = R.make_batch(rng, B, Tmax, D)
        for norm in (None, "ortho"):
            for cutoff, log_domain in ((50, True), (20, False), (100, True)):
                old = PP.modspec_smoothing(x, modfs, n=n, norm=norm, cutoff=cutoff, log_domain=log_domain)
                new = PP.modspec_smoothing_batch(x, modfs, n=n, norm=norm, cutoff=cutoff, log_domain=log_domain)
                assert new.dtype == F64 and new.shape == old.shape
                assert _err(new, old) <= 1e-12, (n, norm, cutoff, log_domain, _err(new, old))
        lengths = np.array(_lengths(n, Tmax))
        lengths[2] = 5                                          # (the per-utterance loop has no empty utterance to offer)
        xp = R.make_batch(rng, B, Tmax, D, lengths, pad=0.0)
        loop = np.zeros_like(xp)
        for b in range(B):
            loop[b, :lengths[b]] = PP.modspec_smoothing(xp[b, :lengths[b]], modfs, n=n, norm="ortho", cutoff=25, log_domain=True)
        c0 = _counts()
        got = util.apply_each2d_padded(PP.modspec_smoothing, xp, lengths, modfs, n=n, norm="ortho", cutoff=25)
        assert _moved(c0) == {KIND: 1}
        assert got.dtype == F64 and _err(got, loop) <= 1e-12, (n, _err(got, loop))
        got = util.apply_each2d_padded(PP.modspec_smoothing, xp, lengths, modfs, n, "ortho", 25, True)      # positional
        assert _err(got, loop) <= 1e-12


def test_post_filter_through_the_public_functions():
    """numpy in -> numpy out with the dtype kept, tensor in -> tensor out, the (T, D) form, apply_each2d_padded in one launch,
    and the statistics the tables are built from."""
    from nnmnkwii_amd import postfilters as PF, util
    dev = torch.device("cuda")
    rng = np.random.RandomState(41)
    n, Tmax, D, modfs = 256, 256, 5, 200
    nb = n // 2 + 1
    gen = R.make_batch(rng, 6, Tmax, D)
    nat = 1.7 * R.make_batch(rng, 5, Tmax, D) + 0.3 * rng.randn(5, Tmax, D)
    lengths_g = [256, 200, 0, 131, 256, 17]
    # statistics: log P inherits the relative error of |S|, at most eps * log2(n) * max|S| / min|S| -- with the condition asserted
    # here (>= 1e-5) that is 2.2e-16 * 8 * 1e5 = 1.8e-10 per utterance and bin, doubled in log |S|^2: bound 1e-9
    live = MM.live_frames(lengths_g, 6, Tmax)
    assert _phase_condition(gen, live, n) >= 1e-5 and _phase_condition(nat, [Tmax] * 5, n) >= 1e-5
    for norm in (None, "ortho"):
        mg, sg = PF.modspec_log_stats(gen, lengths_g, n=n, norm=norm)
        mgr, sgr = MM.log_stats(gen, n, norm, lengths_g)
        assert mg.shape == sg.shape == (nb, D) and mg.dtype == sg.dtype == F64
        assert np.abs(mg - mgr).max() <= 1e-9 and np.abs(sg - sgr).max() <= 1e-9
    mt, st = PF.modspec_log_stats(torch.from_numpy(nat.astype(F32)).to(dev), n=n)
    mnr, snr = MM.log_stats(nat.astype(F32), n)
    assert mt.is_cuda and mt.dtype == torch.float64 and np.abs(mt.cpu().numpy() - mnr).max() <= 1e-9
    assert np.abs(st.cpu().numpy() - snr).max() <= 1e-9
    A, C = PF.modspec_post_filter_tables(mgr, sgr, mnr, snr, k=0.85)
    Ar, Cr = MM.tables(mgr, sgr, mnr, snr, 0.85)
    assert (A == Ar).all() and (C == Cr).all()
    limit_bin = MM.limit_bin_of(n, modfs, 60)
    ref = MM.filter_batch(np.nan_to_num(gen), n, None, lengths_g, A, C, limit_bin, True)
    for dt in (F64, F32):
        xin = gen.astype(dt)
        refd = ref if dt == F64 else MM.filter_batch(xin, n, None, lengths_g, A, C, limit_bin, True)
        y = PF.modspec_post_filter_batch(xin, A, C, n=n, lengths=lengths_g, modfs=modfs, cutoff=60)
        assert isinstance(y, np.ndarray) and y.dtype == dt and _err(y, refd) <= BOUND[dt]
        yt = PF.modspec_post_filter_batch(torch.from_numpy(xin).to(dev), torch.from_numpy(A).to(dev), torch.from_numpy(C).to(dev), n=n,
                                          lengths=torch.tensor(lengths_g), modfs=modfs, cutoff=60)
        assert yt.is_cuda and yt.dtype == TORCH_DT[dt] and (yt.cpu().numpy() == y).all()
        # the (T, D) form: numpy out of place, a CUDA tensor in place
        one = PF.modspec_post_filter(xin[3, :131], A, C, n=n, modfs=modfs, cutoff=60)
        assert one.dtype == dt and one.shape == (131, D) and _err(one, refd[3, :131]) <= BOUND[dt]
        t = torch.from_numpy(xin[3, :131].copy()).to(dev)
        assert PF.modspec_post_filter(t, A, C, n=n, modfs=modfs, cutoff=60) is t and (t.cpu().numpy() == one).all()
    # the padded loop of the reference's util, in one launch, keyword arguments honoured
    lengths = np.array([256, 200, 9, 131, 256, 17])
    c0 = _counts()
    got = util.apply_each2d_padded(PF.modspec_post_filter, np.nan_to_num(gen), lengths, A, C, n=n, modfs=modfs, cutoff=60)
    assert _moved(c0) == {KIND: 1}
    want = MM.filter_batch(np.nan_to_num(gen), n, None, lengths, A, C, limit_bin, True)
    assert got.dtype == F64 and _err(got, want) <= BOUND[F64]


def test_python_level_errors():
    from nnmnkwii_amd import postfilters as PF, preprocessing as PP
    dev = torch.device("cuda")
    x = torch.zeros((2, 20, 3), dtype=torch.float64, device=dev)
    A = torch.ones((9, 3), dtype=torch.float64, device=dev)
    c0 = _counts()
    with pytest.raises(RuntimeError, match="DFT length 16 must be larger than time length 20"):
        PF.modspec_post_filter_batch(x, A, A, n=16)
    with pytest.raises(RuntimeError, match="DFT length 16 must be larger than time length 20"):
        PP.modspec_smoothing_batch(x, 200, n=16)
    with pytest.raises(ValueError, match="Nyquist"):
        PF.modspec_post_filter_batch(x, None, None, n=32, modfs=200, cutoff=101)
    with pytest.raises(ValueError, match="Nyquist"):
        PP.modspec_smoothing_batch(x, 200, n=32, cutoff=101)
    with pytest.raises(ValueError, match="even"):
        PF.modspec_post_filter_batch(x, None, None, n=33)
    for a, c in ((A, None), (None, A)):
        with pytest.raises(ValueError, match="both or neither"):
            PF.modspec_post_filter_batch(x, a, c, n=32)
    with pytest.raises(ValueError, match="tables"):
        PF.modspec_post_filter_batch(x, A, A, n=32)                       # (9, 3) tables at nb = 17
    with pytest.raises(ValueError, match="lengths"):
        PF.modspec_post_filter_batch(x, None, None, n=32, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match="float32 or float64"):
        PF.modspec_post_filter_batch(x.to(torch.float16), None, None, n=32)
    assert not _moved(c0)
    # an odd DFT length: smoothing keeps the 2-D function's rule (the inverse at n - 1)
    rng = np.random.RandomState(3)
    xs = R.make_batch(rng, 2, 20, 3)
    old = PP.modspec_smoothing(xs, 200, n=33, cutoff=30)
    new = PP.modspec_smoothing_batch(xs, 200, n=33, cutoff=30)
    assert _err(new, old) <= 1e-12
