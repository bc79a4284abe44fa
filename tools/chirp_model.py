"""Executable specification (numpy) of the chirp-z modulation-spectrum kernel (csrc/modspec_chirp.hip: the float64 entries at a DFT
length n in [3, 2048] that is no power of two).  NOT product code and not the oracle.

Bluestein: with j k = (j^2 + k^2 - (k - j)^2) / 2 and w_j = exp(-i pi j^2 / n),

    Z_k = sum_j z_j e^{-2 pi i j k / n} = w_k sum_j (z_j w_j) conj(w_{k-j}),

a convolution that a circular one of length M = 2^ceil(log2(2n - 1)) holds:

    a_j = z_j w_j (j < T), 0 up to M;   f_m = f_{M-m} = conj(w_m) (m < n), 0 in between;   F = FFT_M(f)
    c = IFFT_M(FFT_M(a) F);             Z_k = w_k c_k (k < n)

The inverse n-point DFT is conj(DFT(conj Z)): the same two tables.  The phase of w_j is the integer j^2 mod 2n, reduced exactly
before it meets pi.  numpy.fft does the inner M-point transforms and nothing else: every length-n step -- the chirp products, the
packing of two real columns as z = x1 + i x2, unpack2 / pack2 with the mirror bin (n - k) % n, the edge bins (0, and n/2 for
even n only), the four modes and their scalings -- is written out as the kernel does it.

Shapes: x (T, D) with T <= n; ms (n/2+1, D); phase (n/2+1, D) complex unit phasors; results as the C entries return them
(inverse (n, D); smoothing and backward (T, D)).  Columns are processed in pairs, the last column of an odd D alone."""
import numpy as np

MODE_SPEC, MODE_INVERSE, MODE_SMOOTH, MODE_BACKWARD = range(4)


def takes(n):
    """The lengths the chirp-z route serves (mlpg_hip_modspec_route answers 2)."""
    return 3 <= n <= 2048 and (n & (n - 1)) != 0


def conv_length(n):
    """M: the smallest power of two that holds the linear convolution of n samples with the 2n - 1 filter taps."""
    M = 1
    while M < 2 * n - 1:
        M <<= 1
    return M


def chirp_table(n):
    """w_j = exp(-i pi j^2 / n), j < n, the phase reduced as the integer j^2 mod 2n."""
    j = np.arange(n, dtype=np.int64)
    r = (j * j) % (2 * n)
    ang = -np.pi * (r.astype(np.float64) / n)
    return np.cos(ang) + 1j * np.sin(ang)


def chirp_filter(n):
    """F = FFT_M(f) / M with f_m = f_{M-m} = conj(w_m), m < n (the kernel folds the 1 / M of the inverse transform in here)."""
    M = conv_length(n)
    w = chirp_table(n)
    f = np.zeros(M, dtype=np.complex128)
    f[:n] = np.conj(w)
    f[M - n + 1:] = np.conj(w[1:])[::-1]
    return np.fft.fft(f) / M


def chirp_dft(z, n, w=None, F=None):
    """n-point DFT of the complex sequence z (len(z) <= n, zero-padded) through the length-M circular convolution."""
    w = chirp_table(n) if w is None else w
    F = chirp_filter(n) if F is None else F
    M = len(F)
    a = np.zeros(M, dtype=np.complex128)
    a[:len(z)] = z * w[:len(z)]
    c = np.fft.ifft(np.fft.fft(a) * F) * M      # (unscaled inverse transform; F carries the 1 / M)
    return w * c[:n]


def chirp_idft(Z, n, w=None, F=None):
    """Unscaled inverse n-point DFT, sum_k Z_k e^{+2 pi i k t / n}, as conj(DFT(conj Z))."""
    return np.conj(chirp_dft(np.conj(Z), n, w, F))


def unpack2(zk, zm):
    """Spectra of the two packed real columns at bin k from Z_k and Z_{(n-k) % n}."""
    return 0.5 * (zk + np.conj(zm)), -0.5j * (zk - np.conj(zm))


def pack2(h1, h2):
    """Z_k and Z_{(n-k) % n} of h1 + i h2 for two Hermitian spectra given at bin k."""
    return h1 + 1j * h2, np.conj(h1) + 1j * np.conj(h2)


def unit_phasor(s):
    mag = np.abs(s)
    return np.where(mag > 0, s / np.where(mag > 0, mag, 1.0), 1.0 + 0j)


def _edge(n):
    """Bins of the half spectrum that are their own mirror: 0 and, for even n, n/2."""
    e = np.zeros(n // 2 + 1, dtype=bool)
    e[0] = True
    if n % 2 == 0:
        e[n // 2] = True
    return e


def _pair(mode, x1, x2, m1, m2, p1, p2, n, ortho, limit_bin, log_domain, w, F):
    """One workgroup: the column pair (x2 / m2 / p2 None: the unpaired last column)."""
    nb = n // 2 + 1
    k = np.arange(nb)
    km = (n - k) % n
    edge = _edge(n)
    fwd_scale = 1.0 / np.sqrt(n) if ortho else 1.0
    inv_scale = 1.0 / np.sqrt(n) if ortho else 1.0 / n
    two = (x2 is not None) if mode != MODE_INVERSE else (m2 is not None)

    def back(h1, h2):
        h1 = np.where(edge, h1.real, h1)
        h2 = np.where(edge, h2.real, h2) if two else np.zeros(nb, dtype=np.complex128)
        zk, zm = pack2(h1, h2)
        Z = np.zeros(n, dtype=np.complex128)
        Z[k] = zk
        Z[km[~edge]] = zm[~edge]
        return chirp_idft(Z, n, w, F)

    if mode == MODE_INVERSE:
        h1 = np.sqrt(m1) * p1
        h2 = np.sqrt(m2) * p2 if two else None
        y = back(h1, h2) * inv_scale
        return y.real, (y.imag if two else None)

    T = len(x1)
    z = x1.astype(np.complex128)
    if two:
        z = z + 1j * x2
    Z = chirp_dft(z, n, w, F)
    s1, s2 = unpack2(Z[k], Z[km])
    s1, s2 = s1 * fwd_scale, s2 * fwd_scale
    if mode == MODE_SPEC:
        return (np.abs(s1) ** 2, unit_phasor(s1)), ((np.abs(s2) ** 2, unit_phasor(s2)) if two else None)
    if mode == MODE_SMOOTH:
        cut = k >= limit_bin
        h1 = np.where(cut, unit_phasor(s1) if log_domain else 0.0, s1)
        h2 = np.where(cut, unit_phasor(s2) if log_domain else 0.0, s2)
        y = back(h1, h2) * inv_scale
    else:
        f = np.where(edge, 1.0, 0.5)
        h1 = f * m1 * s1
        h2 = f * m2 * s2 if two else None
        y = back(h1, h2) * (2.0 / np.sqrt(n) if ortho else 2.0)
    return y.real[:T], (y.imag[:T] if two else None)


def _run(mode, n, D, ortho, x=None, ms=None, phase=None, limit_bin=0, log_domain=True):
    if not takes(n):
        raise ValueError("the chirp-z route takes a DFT length in [3, 2048] that is no power of two (got %d)" % n)
    w, F = chirp_table(n), chirp_filter(n)
    outs = [None] * D
    for d in range(0, D, 2):
        two = d + 1 < D
        col = lambda arr, dd: None if arr is None or dd >= D else np.asarray(arr)[:, dd]
        r1, r2 = _pair(mode, col(x, d), col(x, d + 1) if two else None, col(ms, d), col(ms, d + 1) if two else None,
                       col(phase, d), col(phase, d + 1) if two else None, n, ortho, limit_bin, log_domain, w, F)
        outs[d] = r1
        if two:
            outs[d + 1] = r2
    return outs


def modspec(x, n, ortho=False):
    """(ms (n/2+1, D), phase (n/2+1, D) complex) of x (T, D), T <= n."""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[0] <= n
    outs = _run(MODE_SPEC, n, x.shape[1], ortho, x=x)
    return np.stack([o[0] for o in outs], axis=1), np.stack([o[1] for o in outs], axis=1)


def inv_modspec(ms, phase, n, ortho=False):
    """(n, D): irfft of sqrt(ms) * phase at length n (the C entry takes any n; numpy's inv_modspec calls it at n = 2 (K - 1))."""
    ms = np.asarray(ms, dtype=np.float64)
    assert ms.shape[0] == n // 2 + 1
    return np.stack(_run(MODE_INVERSE, n, ms.shape[1], ortho, ms=ms, phase=np.asarray(phase)), axis=1)


def modspec_smoothing(x, n, limit_bin, log_domain=True, ortho=False):
    """(T, D): bins >= limit_bin removed (log domain: unit magnitude, phase kept) and transformed back at the same n."""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[0] <= n
    return np.stack(_run(MODE_SMOOTH, n, x.shape[1], ortho, x=x, limit_bin=limit_bin, log_domain=log_domain), axis=1)


def modspec_backward(x, grad_ms, n, ortho=False):
    """(T, D): d sum(grad_ms * modspec(x)) / dx."""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[0] <= n
    return np.stack(_run(MODE_BACKWARD, n, x.shape[1], ortho, x=x, ms=np.asarray(grad_ms, dtype=np.float64)), axis=1)


if __name__ == "__main__":
    rng = np.random.RandomState(0)
    for n in (3, 5, 6, 7, 12, 33, 100, 127, 1000, 1025, 2046, 2047):
        x = 0.1 * np.cumsum(rng.randn(n, 3), 0) + rng.rand(n, 3)
        ref = np.fft.rfft(x, n=n, axis=0)
        ms, ph = modspec(x, n)
        e_ms = np.abs(ms - np.abs(ref) ** 2).max() / (np.abs(ref) ** 2).max()
        e_inv = np.abs(inv_modspec(np.abs(ref) ** 2, unit_phasor(ref), n) - np.fft.irfft(ref, n=n, axis=0)).max() / np.abs(x).max()
        print("n=%4d M=%4d  spectrum %.1e  inverse %.1e" % (n, conv_length(n), e_ms, e_inv))
