"""CPU: the numpy model of the Merlin post-filter (tools/postfilter_model.py, the executable specification of csrc/postfilter.hip)
pinned independently of its own recursions.  pysptk is not in this image, so no golden of the reference exists; what pins the four
restated SPTK operations instead:

  freqt   the warp identity of the all-pass substitution (the transformed cepstrum has the same log spectrum on the warped
          axis), and freqt(freqt(c, m, a), m, -a) = c for a large m
  c2acr0  the energy sum h[n]^2 of the minimum-phase impulse response the cepstrum defines (Parseval)
  mc2b / b2mc   inverses of each other
  whole   weight = 1 is the identity; the frame energy r0 is preserved; coefficients 2 .. D - 1 of mc2b(out) are coef times those
          of mc2b(mgc); the table form (what the kernel computes) against the literal form

Parity with the pysptk package itself stays unpinned here; test_against_pysptk_when_installed pins it wherever it is installed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import postfilter_model as PM  # noqa: E402

DIMS = (1, 2, 3, 25, 60, 64)
SIZES = ((15, 32), (31, 64), (63, 64), (511, 1024))
ALPHAS = (0.0, 0.35, 0.58, 0.77, -0.42)


def mgc_like(rng, T, D):
    """Mel-cepstra as a vocoder analysis gives them: a large c0, the others decaying with their index."""
    x = rng.randn(T, D) / (1.0 + np.arange(D))
    x[:, 0] += rng.uniform(-8.0, 2.0, T)
    return x


def grid():
    for D in DIMS:
        for order, fftlen in SIZES:
            for alpha in ALPHAS:
                yield D, order, fftlen, alpha


def test_freqt_keeps_the_log_spectrum_on_the_warped_axis():
    """c2 = freqt(c1, m2, a):  sum_k c1[k] cos(k w1) = sum_j c2[j] cos(j w2)  with  w1 = w2 - 2 atan(a sin w2 / (1 + a cos w2)),
    wherever the truncation at m2 is negligible -- which the test checks, so that it cannot quietly pass on nothing."""
    rng = np.random.RandomState(0)
    w2 = np.linspace(0.0, np.pi, 97)
    for D, a in [(40, -0.77), (40, 0.77), (60, -0.58), (25, -0.35), (25, 0.42), (5, 0.0)]:
        m2 = 511
        tail = np.abs(PM.freqt(np.eye(D), m2, a)[:, m2]).max()
        assert tail < 1e-13, (D, a, tail)
        c1 = mgc_like(rng, 3, D)
        c2 = PM.freqt(c1, m2, a)
        w1 = w2 - 2.0 * np.arctan(a * np.sin(w2) / (1.0 + a * np.cos(w2)))
        lhs = c1 @ np.cos(np.outer(np.arange(D), w1))
        rhs = c2 @ np.cos(np.outer(np.arange(m2 + 1), w2))
        err = np.abs(lhs - rhs).max()
        print("warp identity D=%d a=%+.2f: tail %.1e err %.2e" % (D, a, tail, err))
        assert err <= 1e-12, (D, a, err)


def test_freqt_is_undone_by_the_opposite_warp():
    rng = np.random.RandomState(1)
    for D, a in [(25, 0.42), (40, -0.58), (10, 0.77)]:
        m = 511
        c = mgc_like(rng, 2, D)
        back = PM.freqt(PM.freqt(c, m, a), m, -a)
        err = max(np.abs(back[:, :D] - c).max(), np.abs(back[:, D:]).max())
        print("freqt round trip D=%d a=%+.2f: %.2e" % (D, a, err))
        assert err <= 1e-12, (D, a, err)


def test_c2acr0_is_the_energy_of_the_minimum_phase_impulse_response():
    """h from the cepstrum by n h[n] = sum_{k=1..n} k c[k] h[n-k], h[0] = exp(c[0]); sum h^2 = (1/N) sum_k exp(2 Re X_k) once h has
    decayed within N."""
    rng = np.random.RandomState(2)
    N = 1024
    for trial in range(4):
        c = np.concatenate([[rng.uniform(-2.0, 1.0)], rng.randn(5) * 0.3])
        h = np.zeros(N)
        h[0] = np.exp(c[0])
        for n in range(1, N):
            k = np.arange(1, min(n, len(c) - 1) + 1)
            h[n] = (k * c[k] * h[n - k]).sum() / n
        assert np.abs(h[N // 2:]).max() < 1e-30 * np.abs(h).max()       # decayed long before N
        energy = (h * h).sum()
        got = PM.c2acr0(c, N)
        assert abs(got / energy - 1.0) <= 1e-12, (trial, got, energy)


def test_mc2b_and_b2mc_are_inverses():
    rng = np.random.RandomState(3)
    for D in DIMS:
        for a in ALPHAS:
            c = mgc_like(rng, 4, D)
            for f, g in ((PM.mc2b, PM.b2mc), (PM.b2mc, PM.mc2b)):
                assert np.abs(g(f(c, a), a) - c).max() <= 1e-14 * np.abs(c).max(), (D, a)


def test_whole_function_properties_and_table_form_over_the_grid():
    rng = np.random.RandomState(4)
    coef = 1.4
    worst = dict(identity=0.0, energy=0.0, emphasis=0.0, table=0.0)
    cases = 0
    for D, order, fftlen, alpha in grid():
        if order < D - 1:                       # outside the limits: refused, not computed
            with pytest.raises(ValueError):
                PM.check_limits(D, alpha, order, fftlen)
            continue
        PM.check_limits(D, alpha, order, fftlen)
        cases += 1
        mgc = mgc_like(rng, 3, D)
        ref = PM.post_filter_literal(mgc, alpha, order, fftlen, coef)
        scale = np.abs(ref).max()
        # weight = 1 returns the input
        same = PM.post_filter_literal(mgc, alpha, order, fftlen, weight=np.ones(D))
        e_id = np.abs(same - mgc).max() / np.abs(mgc).max()
        # the frame energy is put back
        r_in = PM.c2acr0(PM.freqt(mgc, order, -alpha), fftlen)
        r_out = PM.c2acr0(PM.freqt(ref, order, -alpha), fftlen)
        e_en = np.abs(r_out / r_in - 1.0).max()
        # the emphasis: in the b domain every coefficient from the third on is scaled by coef
        b_in, b_out = PM.mc2b(mgc, alpha), PM.mc2b(ref, alpha)
        e_em = np.abs(b_out[:, 2:] - coef * b_in[:, 2:]).max() / scale if D > 2 else 0.0
        # the form the kernel uses
        G = PM.table(D, alpha, order, fftlen)
        assert G.shape == (fftlen // 2 + 1, D)
        tab = PM.post_filter_table(mgc, alpha, G, fftlen, PM.default_weight(D, coef))
        e_tab = np.abs(tab - ref).max() / scale
        for k, v in (("identity", e_id), ("energy", e_en), ("emphasis", e_em), ("table", e_tab)):
            worst[k] = max(worst[k], v)
        assert e_id <= 1e-13 and e_en <= 1e-12 and e_em <= 1e-13 and e_tab <= 1e-13, (D, order, fftlen, alpha, e_id, e_en, e_em, e_tab)
    print("post-filter model over %d cases: %s" % (cases, worst))
    assert cases == 5 * (4 + 4 + 4 + 3 + 2 + 2)      # the (D, order) pairs inside the limits, every alpha


def test_limits():
    for bad in [(0, 0.5, 15, 32), (65, 0.5, 511, 1024), (5, 0.5, 2, 3), (5, 0.5, 15, 24), (5, 0.5, 511, 8192), (5, 0.5, 32, 32),
                (5, 0.5, 3, 32), (5, 1.0, 15, 32), (5, -1.0, 15, 32), (5, float("nan"), 15, 32)]:
        with pytest.raises(ValueError):
            PM.check_limits(*bad)
    PM.check_limits(64, 0.99, 63, 64)
    PM.check_limits(1, 0.0, 0, 4)


def test_padded_batch_semantics():
    rng = np.random.RandomState(5)
    B, Tmax, D = 4, 9, 5
    X = np.stack([mgc_like(rng, Tmax, D) for _ in range(B)])
    lengths = np.array([Tmax + 3, 4, 0, -2])
    Xn = X.copy()
    Xn[1, 4:] = Xn[2] = Xn[3] = np.nan
    for form in ("literal", "table"):
        out = PM.post_filter_batch(Xn, 0.42, 15, 32, lengths=lengths, form=form)
        assert np.array_equal(out[1, 4:], np.zeros((Tmax - 4, D))) and not out[2:].any() and np.isfinite(out).all()
        assert np.abs(out[0] - PM.post_filter_literal(X[0], 0.42, 15, 32)).max() <= 1e-13 * np.abs(out[0]).max()
        assert np.abs(out[1, :4] - PM.post_filter_literal(X[1, :4], 0.42, 15, 32)).max() <= 1e-13 * np.abs(out[1]).max()
    full = PM.post_filter_batch(X, 0.42, 15, 32)
    assert np.array_equal(full[0], PM.post_filter_batch(X, 0.42, 15, 32, lengths=lengths)[0])


def test_against_pysptk_when_installed():
    """The model restates SPTK's freqt, c2acr, mc2b and b2mc from their published definitions (parity unpinned: the package is not
    in this image).  Wherever pysptk IS installed this test pins each of the four and the whole function against it."""
    pysptk = pytest.importorskip("pysptk")
    rng = np.random.RandomState(6)
    for D, order, fftlen, alpha in [(25, 511, 1024, 0.42), (60, 511, 1024, 0.58), (40, 511, 1024, 0.77), (5, 31, 64, 0.35)]:
        mgc = mgc_like(rng, 4, D)
        for t in range(len(mgc)):
            c = np.ascontiguousarray(mgc[t])
            f = pysptk.freqt(c, order, -alpha)
            assert np.abs(PM.freqt(c, order, -alpha) - f).max() <= 1e-12 * np.abs(f).max()
            assert abs(PM.c2acr0(f, fftlen) / pysptk.c2acr(f, 0, fftlen)[0] - 1.0) <= 1e-12
            assert np.abs(PM.mc2b(c, alpha) - pysptk.mc2b(c, alpha)).max() <= 1e-13 * np.abs(c).max()
            assert np.abs(PM.b2mc(c, alpha) - pysptk.b2mc(c, alpha)).max() <= 1e-13 * np.abs(c).max()
        # the reference's loop (postfilters/__init__.py:44-62), frame by frame
        w = PM.default_weight(D)
        ref = np.empty_like(mgc)
        for t in range(len(mgc)):
            r0 = pysptk.c2acr(pysptk.freqt(mgc[t], order, -alpha), 0, fftlen)[0]
            p0 = pysptk.c2acr(pysptk.freqt(mgc[t] * w, order, -alpha), 0, fftlen)[0]
            b = pysptk.mc2b(w * mgc[t], alpha)
            b[0] = np.log(r0 / p0) / 2 + b[0]
            ref[t] = pysptk.b2mc(b, alpha)
        assert np.abs(PM.post_filter_literal(mgc, alpha, order, fftlen) - ref).max() <= 1e-12 * np.abs(ref).max()
