"""The chirp-z route of the float64 modulation-spectrum entries (csrc/modspec_chirp.hip: every DFT length in [3, 2048] that is no
power of two) against oracle/modspec.py, against the direct transform, and through the Python layers; which route served a call
is read off mlpg_hip_launch_count(20).  Bounds are those test_modspec_gpu.py::test_any_dft_length and
::test_direct_transform_equals_fft_path ask of the other routes."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

pytestmark = pytest.mark.gpu

NORMS = (None, "ortho")


def _close(a, b, rel):
    scale = max(np.abs(b).max(), 1e-300)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / scale
    assert err <= rel, err


def _counts():
    from nnmnkwii_amd import _hip
    return [_hip.lib().mlpg_hip_launch_count(k) for k in range(21)]


@contextlib.contextmanager
def _chirp_calls(k=1):
    """The block makes k C calls on the chirp-z route: kind 20 moves by k, the padded-minibatch kinds 17-19 do not move."""
    c0 = _counts()
    yield
    c1 = _counts()
    assert c1[20] - c0[20] == k, (c0[20], c1[20], k)
    assert c1[17:20] == c0[17:20]


def _traj(rng, *shape):
    return 0.1 * np.cumsum(rng.randn(*shape), axis=-2) + rng.rand(*shape)


def _per_utt(f, *arrs):
    return np.stack([f(*[a[b] for a in arrs]) for b in range(arrs[0].shape[0])])


@pytest.mark.parametrize("n", [3, 5, 6, 7, 12, 33, 100, 1000, 1025, 2046, 2047])
def test_parity_and_route(n):
    """Spectrum, phase, inverse, smoothing (both domains, three cutoffs) and the analytic gradient through autograd.modspec
    against the numpy restatement of the reference, both norms, a lone column and a batch with an unpaired last column."""
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd import preprocessing as P
    from oracle import modspec as OM
    assert _hip.modspec_route(n) == 2
    # an odd n is smoothed through modspec(n) and inv_modspec(n - 1): each leg on the route of its own length
    smooth_calls = 1 if n % 2 == 0 else 1 + (_hip.modspec_route(n - 1) == 2)
    rng = np.random.RandomState(n)
    for T in sorted({1, max(1, n // 3), n}):
        for B, D in ((1, 1), (3, 5)):
            x = _traj(rng, B, T, D)
            w = rng.rand(B, n // 2 + 1, D)
            for norm in NORMS:
                with _chirp_calls():
                    ms, ph = P.modspec(x, n=n, norm=norm, return_phase=True)
                mo = _per_utt(lambda a: OM.modspec(a, n=n, norm=norm), x)
                po = _per_utt(lambda a: OM.modspec(a, n=n, norm=norm, return_phase=True)[1], x)
                _close(ms, mo, 1e-11)
                big = mo > 1e-6 * mo.max()                    # the phase of a vanishing bin is noise
                assert np.abs(ph - po)[big].max() < 1e-8
                if n % 2 == 0:
                    with _chirp_calls():
                        inv = P.inv_modspec(mo, po, norm=norm)
                    _close(inv, _per_utt(lambda m, p: OM.inv_modspec(m, p, norm=norm), mo, po), 1e-11)
                for log_domain in (True, False):
                    for cutoff in (100, 25, 60):
                        with _chirp_calls(smooth_calls):
                            y = P.modspec_smoothing(x, 200, n=n, norm=norm, cutoff=cutoff, log_domain=log_domain)
                        yo = _per_utt(lambda a: OM.modspec_smoothing(a, 200, n=n, norm=norm, cutoff=cutoff, log_domain=log_domain), x)
                        _close(y, yo, 1e-9)
                for b in range(B):
                    yt = torch.from_numpy(x[b]).cuda().requires_grad_()
                    with _chirp_calls():
                        out = AF.modspec(yt, n=n, norm=norm)
                    with _chirp_calls():
                        (out * torch.from_numpy(w[b]).cuda()).sum().backward()
                    _close(yt.grad.cpu().numpy(), OM.modspec_grad(x[b], w[b], n, norm), 1e-10)


@pytest.mark.parametrize("n,shape", [(1000, (4, 700, 37)), (2047, (2, 2047, 3))])
def test_chirp_equals_the_direct_transform(n, shape):
    """The same problems through chirp-z and, behind mlpg_hip_modspec_set_direct(1), the direct transform: all four modes."""
    from nnmnkwii_amd import _hip
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(*shape, dtype=torch.float64, device="cuda", generator=gen)
    g = torch.rand(shape[0], n // 2 + 1, shape[2], dtype=torch.float64, device="cuda", generator=gen)

    def run():
        ms, ph = _hip.modspec(x, n, want_phase=True)
        ms_o, ph_o = _hip.modspec(x, n, ortho=True, want_phase=True)
        return (ms, ph, _inverse(ms, ph, n, False), _inverse(ms_o, ph_o, n, True), _hip.modspec_smoothing(x, n, n // 10, log_domain=True),
                _hip.modspec_smoothing(x, n, n // 10, log_domain=False, ortho=True), _hip.modspec_backward(x, g, n),
                _hip.modspec_backward(x, g, n, True), ms_o)

    c0 = _counts()
    a = run()
    c1 = _counts()
    assert c1[20] - c0[20] == 8 and c1[17:20] == c0[17:20]
    _hip.lib().mlpg_hip_modspec_set_direct(1)
    try:
        b = run()
    finally:
        _hip.lib().mlpg_hip_modspec_set_direct(0)
    assert _counts()[20] == c1[20]
    for i, (u, v) in enumerate(zip(a, b)):
        if i == 1:
            continue                                      # phases of tiny bins differ; compared through the inverse
        assert u.shape == v.shape
        assert float((u - v).abs().max()) <= 1e-10 * float(v.abs().max()), i


def _inverse(ms, ph, n, ortho):
    """mlpg_hip_inv_modspec at the length n itself (the Python wrapper derives an even n from the bin count; the C entry, like
    numpy's irfft, takes an odd one too)."""
    from nnmnkwii_amd import _hip
    B, nb, D = ms.shape
    assert nb == n // 2 + 1
    out = torch.empty((B, n, D), dtype=torch.float64, device=ms.device)
    rc = _hip.lib().mlpg_hip_inv_modspec(ms.device.index, _hip._stream(ms.device), _hip._p(ms), _hip._p(ph), B, n, D, int(ortho),
                                         _hip._p(out))
    assert rc == 0, _hip.lib().mlpg_hip_last_error()
    return out


def test_unchanged_routes():
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(2, 50, 3, dtype=torch.float64, device="cuda", generator=gen)
    for n in (1024, 4096, 2049, 3000, 5000, 8192):
        g = torch.rand(2, n // 2 + 1, 3, dtype=torch.float64, device="cuda", generator=gen)
        assert _hip.modspec_route(n) == (0 if n in (1024, 4096) else 1)
        with _chirp_calls(0):
            ms, ph = _hip.modspec(x, n, want_phase=True)
            _hip.inv_modspec(ms, ph)
            _hip.modspec_smoothing(x, n, 20)
            _hip.modspec_backward(x, g, n)
    # the padded-minibatch entries keep the direct transform at a length that is no power of two
    c0 = _counts()
    y = x.clone().requires_grad_()
    AF.modspec_batch(y, n=100).sum().backward()
    c1 = _counts()
    assert c1[18] > c0[18] and c1[20] == c0[20] and c1[17] == c0[17]


@pytest.mark.parametrize("n,calls", [(1001, 2), (1025, 1)])
def test_odd_length_smoothing_legs(n, calls):
    """n = 1001: modspec(1001) and inv_modspec(1000) both chirp-z; n = 1025: the inverse at 1024 runs on the FFT."""
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import preprocessing as P
    from oracle import modspec as OM
    assert _hip.modspec_route(n) == 2 and _hip.modspec_route(n - 1) == (2 if calls == 2 else 0)
    rng = np.random.RandomState(n)
    x = _traj(rng, 400, 5)
    for norm in NORMS:
        for log_domain in (True, False):
            with _chirp_calls(calls):
                y = P.modspec_smoothing(x, 200, n=n, norm=norm, cutoff=40, log_domain=log_domain)
            _close(y, OM.modspec_smoothing(x, 200, n=n, norm=norm, cutoff=40, log_domain=log_domain), 1e-9)


def test_dtypes_devices_and_batches():
    from nnmnkwii_amd import preprocessing as P
    from oracle import modspec as OM
    n = 100
    rng = np.random.RandomState(7)
    x32 = _traj(rng, 70, 4).astype(np.float32)
    ms, ph = P.modspec(x32, n=n, return_phase=True)
    assert ms.dtype == np.float32 and ph.dtype == np.complex64
    _close(ms, OM.modspec(x32.astype(np.float64), n=n), 2e-6)     # float32's own rounding of the result
    assert P.modspec_smoothing(x32, 200, n=n, cutoff=30).dtype == np.float32
    assert P.modphase(x32, n=n).dtype == np.complex64
    # a (B, T, D) batch, numpy or CUDA, is the stack of the per-utterance results, bit for bit
    xb = _traj(rng, 3, 70, 5)
    yb = P.modspec_smoothing(xb, 200, n=n, cutoff=40)
    mb, pb = P.modspec(xb, n=n, return_phase=True)
    for b in range(3):
        np.testing.assert_array_equal(yb[b], P.modspec_smoothing(xb[b], 200, n=n, cutoff=40))
        m1, p1 = P.modspec(xb[b], n=n, return_phase=True)
        np.testing.assert_array_equal(mb[b], m1)
        np.testing.assert_array_equal(pb[b], p1)
    xt = torch.from_numpy(xb).cuda()
    yt = P.modspec_smoothing(xt, 200, n=n, cutoff=40)
    assert yt.is_cuda and np.array_equal(yt.cpu().numpy(), yb)
    mt, pt = P.modspec(xt, n=n, return_phase=True)
    assert mt.is_cuda and pt.is_cuda and pt.dtype == torch.complex128 and np.array_equal(mt.cpu().numpy(), mb)


@pytest.mark.parametrize("norm", NORMS)
def test_gradcheck(norm):
    from nnmnkwii_amd import autograd as AF
    gen = torch.Generator(device="cuda").manual_seed(12)
    y = torch.rand(8, 3, dtype=torch.float64, device="cuda", generator=gen).requires_grad_()
    c0 = _counts()
    assert torch.autograd.gradcheck(lambda t: AF.ModSpec.apply(t, 12, norm), (y,), eps=1e-6, atol=1e-6)
    assert _counts()[20] > c0[20]


def test_size_independent_properties():
    """64 x 1000 x 60 at n = 2000: Parseval with the Hermitian weights, the scale factor, the band removal -- checks that need no
    CPU transform (modelled on test_modspec_gpu.py::test_full_size_properties)."""
    from nnmnkwii_amd import _hip
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(64, 1000, 60, dtype=torch.float64, device="cuda", generator=gen)
    n = 2000
    assert _hip.modspec_route(n) == 2
    with _chirp_calls():
        ms, _ = _hip.modspec(x, n)
    # Parseval for a real signal: n sum x^2 = ms[0] + 2 sum_{0<k<n/2} ms[k] + ms[n/2]
    lhs = n * (x * x).sum(dim=1)
    rhs = ms[:, 0] + 2.0 * ms[:, 1:n // 2].sum(dim=1) + ms[:, n // 2]
    assert torch.allclose(lhs, rhs, rtol=1e-11, atol=0)
    mo, _ = _hip.modspec(x, n, ortho=True)
    assert torch.allclose(mo * n, ms, rtol=1e-12, atol=0)
    # the square root of the spectrum is linear in a scale factor
    m3, _ = _hip.modspec(-3.0 * x, n)
    assert torch.allclose(m3.sqrt(), 3.0 * ms.sqrt(), rtol=1e-12, atol=1e-12 * float(ms.max().sqrt()))
    lim = 250
    s1 = _hip.modspec_smoothing(x, n, lim, log_domain=False)
    # the linear band removal followed by truncation to T frames is not a projection, but removing nothing is the identity and
    # the operator is linear
    ident = _hip.modspec_smoothing(x, n, n // 2 + 1, log_domain=False)
    assert torch.allclose(ident, x, rtol=0, atol=1e-12)
    y = torch.randn(64, 1000, 60, dtype=torch.float64, device="cuda", generator=gen)
    lin = _hip.modspec_smoothing(2.0 * x - 3.0 * y, n, lim, log_domain=False)
    assert torch.allclose(lin, 2.0 * s1 - 3.0 * _hip.modspec_smoothing(y, n, lim, log_domain=False), rtol=0, atol=1e-11)
    assert torch.isfinite(s1).all()
    # smoothing lowers the high-band power of the padded trajectory
    hi_before = ms[:, lim:].sum()
    hi_after = _hip.modspec(s1, n)[0][:, lim:].sum()
    assert hi_after < 0.2 * hi_before
    # with nothing truncated (T = n) the band removal is a projection: removing the band twice is removing it once
    z = torch.randn(4, n, 6, dtype=torch.float64, device="cuda", generator=gen)
    p1 = _hip.modspec_smoothing(z, n, lim, log_domain=False)
    p2 = _hip.modspec_smoothing(p1, n, lim, log_domain=False)
    assert torch.allclose(p2, p1, rtol=0, atol=1e-12)
    # (what is left in the removed band is rounding: 1e-12 of the largest amplitude at the very most, squared)
    assert float(_hip.modspec(p1, n)[0][:, lim:].max()) <= 1e-24 * float(_hip.modspec(z, n)[0].max())
