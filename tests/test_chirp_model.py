"""CPU: the numpy model of the chirp-z modulation-spectrum kernel (tools/chirp_model.py, the executable specification of
csrc/modspec_chirp.hip) against numpy's rfft / irfft and oracle/modspec.py: the choice of M, the j^2 mod 2n phase, the wrapped
filter, conjugation for the inverse, the pair packing at a length that is no power of two, the four modes, both norms.

Bound: max|delta| <= 1e-12 * max|reference|, the tightest modulation-spectrum tolerance of the suite (test_modspec_gpu.py).  A
float64 chirp-z of this construction sits at 1e-15 to 2e-15 for the spectrum and the inverse (python tools/chirp_model.py prints
the figures), so the bound has about three orders of room."""
import os
import sys

import numpy as np
import pytest

from oracle import modspec as OM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import chirp_model as CM  # noqa: E402

REL = 1e-12
LENGTHS = [n for n in range(3, 301) if n & (n - 1)] + [1000, 1025, 2046, 2047]
NORMS = (None, "ortho")
D = 3                      # one pair of columns and the unpaired last column


def _close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(np.abs(b).max(), 1e-300)
    err = np.abs(a - b).max() / scale
    assert err <= REL, (what, err)


def _frames(n):
    return sorted({1, max(1, n // 3), n})


def _x(rng, T):
    return 0.1 * np.cumsum(rng.randn(T, D), 0) + rng.rand(T, D)


def _chunks(k):
    """The lengths in four parametrised slices, so that no single case runs long."""
    return LENGTHS[k::4]


def test_the_lengths_and_M():
    assert CM.conv_length(3) == 8 and CM.conv_length(33) == 128 and CM.conv_length(100) == 256
    for n in range(1025, 2049):
        assert CM.conv_length(n) == 4096
    for n in range(3, 2049):
        M = CM.conv_length(n)
        assert M >= 2 * n - 1 and M // 2 < 2 * n - 1 and M & (M - 1) == 0
    assert not CM.takes(2) and CM.takes(3) and not CM.takes(4) and CM.takes(2047) and not CM.takes(2048) and not CM.takes(2049)
    with pytest.raises(ValueError):
        CM.modspec(np.zeros((4, 2)), 16)
    with pytest.raises(ValueError):
        CM.modspec(np.zeros((4, 2)), 3000)


def test_tables():
    for n in (3, 6, 7, 100, 1025, 2047):
        w = CM.chirp_table(n)
        j = np.arange(n)
        # the phase against extended precision, Python integers for j^2 mod 2n: the float64 angle (up to 2 pi) carries a
        # rounding of 2 pi 2^-53 = 7e-16, cos / sin another 1e-16 each
        ang = np.array([(int(q) * int(q)) % (2 * n) for q in j], dtype=np.longdouble) / np.longdouble(n) * np.longdouble(np.pi)
        exact = (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex128)
        assert np.abs(w - exact).max() < 2e-15
        M = CM.conv_length(n)
        f = np.fft.ifft(CM.chirp_filter(n) * M)
        assert np.abs(f[:n] - np.conj(w)).max() < 1e-13 and np.abs(f[n:M - n + 1]).max() < 1e-13
        assert np.abs(f[M - n + 1:] - np.conj(w[1:])[::-1]).max() < 1e-13


@pytest.mark.parametrize("part", range(4))
def test_spectrum_and_phase(part):
    rng = np.random.RandomState(100 + part)
    for n in _chunks(part):
        for T in _frames(n):
            x = _x(rng, T)
            for norm in NORMS:
                ref = np.fft.rfft(x, n=n, axis=0, norm=norm)
                ms, ph = CM.modspec(x, n, ortho=norm == "ortho")
                mo, po = OM.modspec(x, n=n, norm=norm, return_phase=True)
                _close(ms, ref.real ** 2 + ref.imag ** 2, ("ms", n, T, norm))
                _close(ms, mo, ("ms oracle", n, T, norm))
                # the phase of a bin is ill-conditioned where the bin is ~0: compare amplitude-weighted
                _close(ph * np.sqrt(mo), ref, ("phase", n, T, norm))
                assert np.abs(np.abs(ph) - 1.0).max() < 1e-14


@pytest.mark.parametrize("part", range(4))
def test_inverse(part):
    rng = np.random.RandomState(200 + part)
    for n in _chunks(part):
        for T in _frames(n):
            x = _x(rng, T)
            for norm in NORMS:
                mo, po = OM.modspec(x, n=n, norm=norm, return_phase=True)
                y = CM.inv_modspec(mo, po, n, ortho=norm == "ortho")
                _close(y, np.fft.irfft(np.sqrt(mo) * po, n=n, axis=0, norm=norm), ("inverse", n, T, norm))
                if n % 2 == 0:
                    _close(y, OM.inv_modspec(mo, po, norm=norm), ("inverse oracle", n, T, norm))


def _smooth_ref(x, n, norm, limit_bin, log_domain):
    """numpy's rfft / irfft at the same n for both directions (the C entry's rule; the oracle inverts an odd n at n - 1)."""
    s = np.fft.rfft(x, n=n, axis=0, norm=norm)
    if limit_bin < len(s):
        mag = np.abs(s[limit_bin:])
        s[limit_bin:] = np.where(mag > 0, s[limit_bin:] / np.where(mag > 0, mag, 1.0), 1.0) if log_domain else 0.0
    return np.fft.irfft(s, n=n, axis=0, norm=norm)[:x.shape[0]]


@pytest.mark.parametrize("part", range(4))
def test_smoothing(part):
    rng = np.random.RandomState(300 + part)
    for n in _chunks(part):
        for T in _frames(n):
            x = _x(rng, T)
            for norm in NORMS:
                for log_domain in (True, False):
                    for cutoff in (100, 25, 60):
                        limit_bin = int(n * cutoff / 200) + 1
                        y = CM.modspec_smoothing(x, n, limit_bin, log_domain=log_domain, ortho=norm == "ortho")
                        _close(y, _smooth_ref(x, n, norm, limit_bin, log_domain), ("smooth", n, T, norm, log_domain, cutoff))
                        if n % 2 == 0:
                            _close(y, OM.modspec_smoothing(x, 200, n=n, norm=norm, cutoff=cutoff, log_domain=log_domain),
                                   ("smooth oracle", n, T, norm, log_domain, cutoff))


@pytest.mark.parametrize("part", range(4))
def test_backward(part):
    rng = np.random.RandomState(400 + part)
    for n in _chunks(part):
        for T in _frames(n):
            x = _x(rng, T)
            g = rng.rand(n // 2 + 1, D)
            for norm in NORMS:
                _close(CM.modspec_backward(x, g, n, ortho=norm == "ortho"), OM.modspec_grad(x, g, n, norm), ("backward", n, T, norm))
