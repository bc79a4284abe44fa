"""The float64 reference of the padded-minibatch modulation spectrum and MS loss (tests/modspec_batch64.py), pinned on the
CPU: per utterance against oracle/modspec.py (itself pinned on the reference's goldens), and by central differences of its
own loss.  The GPU tests compare the kernels with this reference."""
import numpy as np
import pytest

import modspec_batch64 as R
from oracle import modspec as OM

# (B, T, D, n, lengths): len == Tmax, len < Tmax, len > n and len == 0 all occur
CASES = [
    (3, 200, 5, 256, [200, 131, 0]),
    (4, 300, 4, 256, [300, 256, 17, 0]),      # 300 > n: cropped at n
    (2, 90, 3, 100, [90, 41]),
    (3, 120, 2, 101, [120, 0, 77]),           # odd n, 120 > n
]


@pytest.mark.parametrize("B,T,D,n,lengths", CASES)
@pytest.mark.parametrize("norm", [None, "ortho"])
def test_spectrum_and_gradient_match_the_oracle_per_utterance(B, T, D, n, lengths, norm):
    rng = np.random.RandomState(n + T)
    x = R.make_batch(rng, B, T, D, lengths)                   # NaN in the padding
    w = rng.rand(B, n // 2 + 1, D)
    ms = R.modspec(x, n, norm, lengths)
    g = R.modspec_grad(x, w, n, norm, lengths)
    assert np.isfinite(ms).all() and np.isfinite(g).all()
    for b in range(B):
        xb = x[b, :lengths[b]]
        np.testing.assert_array_equal(ms[b], OM.modspec(xb, n=n, norm=norm))
        ref = OM.modspec_grad(xb, w[b], n, norm)
        live = min(lengths[b], n)
        if lengths[b]:
            assert np.abs(g[b, :lengths[b]] - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)
        assert not g[b, live:].any()                          # exactly 0 at and past min(len, n)
    # no lengths: every utterance has T frames
    xf = R.make_batch(rng, B, T, D)
    np.testing.assert_array_equal(R.modspec(xf, n, norm), np.stack([OM.modspec(xf[b], n=n, norm=norm) for b in range(B)]))


@pytest.mark.parametrize("log_domain", [True, False])
@pytest.mark.parametrize("norm", [None, "ortho"])
@pytest.mark.parametrize("n", [16, 15, 8])
def test_loss_gradient_by_central_differences(n, norm, log_domain):
    """h = 1e-5 on values of order 1: the truncation error of a central difference is h^2 f''' / 6 ~ 1e-10 relative, its rounding
    error ~ 1e-16 / h = 1e-11 of the loss per unit gradient; 1e-6 of the gradient's maximum leaves both three orders of magnitude."""
    rng = np.random.RandomState(7 * n)
    B, T, D, lengths = 3, 12, 2, [12, 5, 0]                   # 12 > 8: the crop is differentiated too
    x = R.make_batch(rng, B, T, D, lengths, pad=0.25)
    tgt = R.modspec(R.make_batch(rng, B, T, D, lengths), n, norm, lengths)
    val, grad = R.loss_and_grad(x, tgt, n, norm, lengths, log_domain, 1e-10)
    assert val == R.loss(x, tgt, n, norm, lengths, log_domain, 1e-10) and val > 0
    num = np.zeros_like(x)
    h = 1e-5
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        num[idx] = (R.loss(xp, tgt, n, norm, lengths, log_domain, 1e-10) - R.loss(xm, tgt, n, norm, lengths, log_domain, 1e-10)) / (2 * h)
    assert np.abs(grad - num).max() <= 1e-6 * np.abs(grad).max()
    for b in range(B):
        assert not grad[b, min(lengths[b], n):].any() and not num[b, min(lengths[b], n):].any()


def test_n_elems_scales_loss_and_gradient():
    rng = np.random.RandomState(3)
    x = R.make_batch(rng, 2, 20, 3)
    tgt = R.modspec(R.make_batch(rng, 2, 20, 3), 32)
    v1, g1 = R.loss_and_grad(x, tgt, 32)
    v2, g2 = R.loss_and_grad(x, tgt, 32, n_elems=2.0 * tgt.size)
    np.testing.assert_allclose(v1, 2.0 * v2, rtol=1e-15)
    np.testing.assert_allclose(g1, 2.0 * g2, rtol=1e-15)
