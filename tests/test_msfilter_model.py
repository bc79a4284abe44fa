"""CPU checks of tools/msfilter_model.py, the executable specification of the modulation-spectrum filter (-m "not gpu"): the
literal definition against the gain form the kernel uses, against oracle/modspec.py's smoothing, and against the properties the
post-filter is defined by (round trip, pure gain, the statistics it is built to produce, the identity entries of its tables, zero
bins, the padded-batch rules)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import msfilter_model as MM  # noqa: E402
from modspec_batch64 import make_batch  # noqa: E402
from oracle import modspec as oracle_ms  # noqa: E402

NS = (4, 16, 64, 256, 4096)
NORMS = (None, "ortho")


def _rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def _tables(rng, nb, D):
    """A in [0.43, 2.7], gains exp(C / 2) within [1/16, 16]."""
    return rng.uniform(0.43, 2.7, (nb, D)), rng.uniform(-2 * np.log(16.0), 2 * np.log(16.0), (nb, D))


@pytest.mark.parametrize("norm", NORMS)
def test_round_trip(norm):
    rng = np.random.RandomState(0)
    for n in NS:
        for live in sorted({n, n // 2 + 1, max(n - 3, 1), 1}):
            x = make_batch(rng, 1, live, 3)[0]
            for form in (MM.filter_literal, MM.filter_gain):
                y = form(x, n, norm)
                assert y.shape == x.shape and _rel(y, x) <= 1e-12, (n, live, form.__name__)


@pytest.mark.parametrize("norm", NORMS)
def test_the_literal_and_the_gain_form_agree(norm):
    rng = np.random.RandomState(1)
    worst = 0.0
    for n in NS:
        nb = n // 2 + 1
        A, C = _tables(rng, nb, 3)
        for live in sorted({n, n // 2 + 1, max(n - 3, 1)}):
            x = make_batch(rng, 1, live, 3)[0]
            for tabs in ((A, C), (None, None)):
                for limit_bin in sorted({0, 1, nb - 1, nb}):
                    for log_domain in (True, False):
                        lit = MM.filter_literal(x, n, norm, tabs[0], tabs[1], limit_bin, log_domain)
                        if not np.abs(lit).max():
                            assert not np.abs(MM.filter_gain(x, n, norm, tabs[0], tabs[1], limit_bin, log_domain)).max()
                            continue
                        err = _rel(MM.filter_gain(x, n, norm, tabs[0], tabs[1], limit_bin, log_domain), lit)
                        worst = max(worst, err)
                        assert err <= 1e-12, (n, live, limit_bin, log_domain, err)
    print("literal against gain form: worst %.2e of the maximum" % worst)


@pytest.mark.parametrize("log_domain", (True, False))
@pytest.mark.parametrize("norm", NORMS)
def test_smoothing_alone_is_the_oracles_modspec_smoothing(norm, log_domain):
    rng = np.random.RandomState(2)
    modfs = 200
    for n in (4, 16, 64, 256, 4096):
        nb = n // 2 + 1
        for cutoff in (1, 20, 50, 100):
            limit_bin = MM.limit_bin_of(n, modfs, cutoff)
            assert limit_bin == min(int(n * cutoff / modfs) + 1, nb)
            for live in sorted({n, n // 2 + 1, max(n - 3, 1)}):
                x = make_batch(rng, 1, live, 2)[0]
                ref = oracle_ms.modspec_smoothing(x, modfs, n=n, norm=norm, cutoff=cutoff, log_domain=log_domain)
                for form in (MM.filter_literal, MM.filter_gain):
                    y = form(x, n, norm, None, None, limit_bin, log_domain)
                    assert _rel(y, ref) <= 1e-12, (n, cutoff, live, form.__name__)
    with pytest.raises(ValueError):
        MM.limit_bin_of(64, 200, 101)
    assert MM.limit_bin_of(64, 200, None) == 33


@pytest.mark.parametrize("norm", NORMS)
def test_a_pure_gain(norm):
    rng = np.random.RandomState(3)
    for n in (4, 64, 4096):
        nb = n // 2 + 1
        for g in (0.25, 3.0):
            x = make_batch(rng, 1, n - 1, 3)[0]
            A, C = np.ones((nb, 3)), np.full((nb, 3), 2.0 * np.log(g))
            for form in (MM.filter_literal, MM.filter_gain):
                assert _rel(form(x, n, norm, A, C), g * x) <= 1e-12


@pytest.mark.parametrize("norm", NORMS)
def test_filtered_statistics_are_the_natural_ones_at_full_emphasis(norm):
    """Every utterance is full length (live = n: nothing is cropped, so log MS of the output is A s + C exactly) and k = 1."""
    rng = np.random.RandomState(4)
    for n in (16, 256):
        gen = make_batch(rng, 6, n, 3)
        nat = 1.7 * make_batch(rng, 5, n, 3) + 0.3 * rng.randn(5, n, 3)
        mg, sg = MM.log_stats(gen, n, norm)
        mn, sn = MM.log_stats(nat, n, norm)
        A, C = MM.tables(mg, sg, mn, sn, k=1.0)
        for form in (MM.filter_literal, MM.filter_gain):
            y = MM.filter_batch(gen, n, norm, None, A, C, form=form)
            my, sy = MM.log_stats(y, n, norm)
            assert np.abs(my - mn).max() <= 1e-9 and np.abs(sy - sn).max() <= 1e-9, (n, np.abs(my - mn).max(), np.abs(sy - sn).max())
        # k = 0 is the identity
        A0, C0 = MM.tables(mg, sg, mn, sn, k=0.0)
        assert (A0 == 1).all() and (C0 == 0).all()


def test_log_stats_skip_empty_utterances_and_are_population_statistics():
    rng = np.random.RandomState(5)
    n, lengths = 32, [32, 0, 17, 9]
    X = make_batch(rng, 4, 32, 2, lengths)
    mean, std = MM.log_stats(X, n, None, lengths)
    s = np.stack([np.log(oracle_ms.modspec(X[b, :lengths[b]], n=n)) for b in (0, 2, 3)])
    assert np.allclose(mean, s.mean(0), rtol=0, atol=1e-13) and np.allclose(std, np.sqrt(((s - s.mean(0)) ** 2).mean(0)), rtol=0, atol=1e-13)


def test_the_table_builder_answers_bad_entries_with_the_identity():
    rng = np.random.RandomState(6)
    shape = (9, 4)
    mg, mn = rng.randn(*shape), rng.randn(*shape)
    sg, sn = rng.uniform(0.5, 2, shape), rng.uniform(0.5, 2, shape)
    k = 0.85
    A, C = MM.tables(mg, sg, mn, sn, k)
    assert np.allclose(A, 1 - k + k * sn / sg, rtol=1e-15, atol=0) and np.allclose(C, k * (mn - sn / sg * mg), rtol=1e-14, atol=1e-15)
    bad = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 0), (5, 1), (6, 2)]
    sg[0, 0] = 0.0
    sg[1, 1] = -1.0
    mg[2, 2] = np.nan
    sn[3, 3] = np.inf
    mn[4, 0] = -np.inf
    sg[5, 1] = np.nan
    sn[6, 2] = np.nan
    A2, C2 = MM.tables(mg, sg, mn, sn, k)
    mask = np.zeros(shape, dtype=bool)
    for ij in bad:
        mask[ij] = True
    assert (A2[mask] == 1).all() and (C2[mask] == 0).all()
    assert (A2[~mask] == A[~mask]).all() and (C2[~mask] == C[~mask]).all()
    assert np.isfinite(A2).all() and np.isfinite(C2).all()


def test_a_zero_power_bin_stays_zero_in_table_bins():
    rng = np.random.RandomState(7)
    n, nb = 64, 33
    A, C = _tables(rng, nb, 2)
    x = np.ones((n, 2))
    x[:, 1] = 0.0                      # column 0: only bin 0 has power; column 1: none at all
    S = np.fft.rfft(x, n=n, axis=0)
    assert (S[1:] == 0).all() and (S[0, 1] == 0)
    for norm in NORMS:
        for form in (MM.filter_literal, MM.filter_gain):
            y = form(x, n, norm, A, C)
            assert np.isfinite(y).all() and (y[:, 1] == 0).all()
            p0 = float(n * n) / (n if norm else 1)   # |S_0|^2 of the column of ones, under either norm
            g0 = np.exp(0.5 * ((A[0, 0] - 1) * np.log(p0) + C[0, 0]))
            assert np.abs(y[:, 0] - g0).max() <= 1e-12 * g0, (norm, form.__name__)
    # ... while a removed zero bin follows modspec_smoothing: unit magnitude in the log domain, zero otherwise
    y = MM.filter_literal(x, n, None, A, C, limit_bin=1, log_domain=False)
    assert np.isfinite(y).all() and (y[:, 1] == 0).all()
    ref = oracle_ms.modspec_smoothing(x, 200, n=n, cutoff=0, log_domain=True)
    assert _rel(MM.filter_gain(x, n, None, None, None, 1, True), ref) <= 1e-12


def test_padded_batch_rules():
    rng = np.random.RandomState(8)
    n, T, D = 32, 29, 3
    nb = n // 2 + 1
    lengths = [29, 17, 0, 40, -2]
    X = make_batch(rng, 5, T, D, np.clip(lengths, 0, T))
    A, C = _tables(rng, nb, D)
    for form in (MM.filter_literal, MM.filter_gain):
        Y = MM.filter_batch(X, n, "ortho", lengths, A, C, 9, True, form=form)
        assert Y.shape == X.shape and np.isfinite(Y).all()
        for b, live in enumerate((29, 17, 0, 29, 0)):
            assert (Y[b, live:] == 0).all()
            if live:
                assert (Y[b, :live] == form(X[b, :live], n, "ortho", A, C, 9, True)).all()
    dense = np.nan_to_num(X)
    assert (MM.filter_batch(dense, n)[3] == MM.filter_batch(dense, n, lengths=lengths)[3]).all()
