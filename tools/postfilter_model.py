"""Executable specification (numpy) of the Merlin post-filter for mel-cepstra (csrc/postfilter.hip, nnmnkwii_amd.postfilters;
the reference's postfilters/__init__.py:7-62).  NOT product code and not an oracle built from the reference: the four SPTK
operations are restated from their published definitions, every function here works on a whole (T, ...) block of frames at once.

For one frame c of D coefficients, w = weight (default: coef everywhere, 1 at indices 0 and 1) and v = w * c:

    r0 = c2acr0(freqt(c, m2, -alpha), N)        p0 = c2acr0(freqt(v, m2, -alpha), N)
    b  = mc2b(v, alpha);   b[0] += log(r0 / p0) / 2;   out = b2mc(b, alpha)

freqt and the real part of the DFT are linear, so L = Re X on the half spectrum is G c with a table G of (N/2+1, D) that depends
on (D, alpha, m2, N) alone (table()): the form the kernel uses (post_filter_table()).  post_filter_batch() adds the padded-batch
semantics of mlpg_hip_merlin_post_filter: frames at or past min(max(len_b, 0), Tmax) are never read and come out as exact zeros."""
import numpy as np


def freqt(c1, m2, a):
    """Frequency transform of cepstra c1 (..., m1 + 1) to order m2 with all-pass constant a: (..., m2 + 1)."""
    c1 = np.asarray(c1, dtype=np.float64)
    m1 = c1.shape[-1] - 1
    lead = c1.shape[:-1]
    g = np.zeros((m2 + 1,) + lead)
    beta = 1.0 - a * a
    cT = np.moveaxis(c1, -1, 0)
    for i in range(-m1, 1):
        d = g.copy()
        g[0] = cT[-i] + a * d[0]
        if m2 >= 1:
            g[1] = beta * d[0] + a * d[1]
        for j in range(2, m2 + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return np.moveaxis(g, 0, -1)


def c2acr0(c, N):
    """Zeroth autocorrelation coefficient of the spectrum exp(X), X the N-point DFT of c (..., <= N) zero-padded."""
    c = np.asarray(c, dtype=np.float64)
    assert c.shape[-1] <= N
    x = np.zeros(c.shape[:-1] + (N,))
    x[..., :c.shape[-1]] = c
    X = np.fft.rfft(x, axis=-1).real
    full = np.concatenate([X, X[..., -2:0:-1]], axis=-1)
    return np.exp(2.0 * full).sum(axis=-1) / N


def mc2b(mc, a):
    mc = np.asarray(mc, dtype=np.float64)
    b = mc.copy()
    for i in range(mc.shape[-1] - 2, -1, -1):
        b[..., i] = mc[..., i] - a * b[..., i + 1]
    return b


def b2mc(b, a):
    b = np.asarray(b, dtype=np.float64)
    mc = b.copy()
    delta = b[..., -1].copy()
    for i in range(b.shape[-1] - 2, -1, -1):
        o = b[..., i] + a * delta
        delta = b[..., i].copy()
        mc[..., i] = o
    return mc


def default_weight(D, coef=1.4):
    w = np.ones(D) * coef
    w[:2] = 1.0
    return w


def check_limits(D, alpha, order, fftlen):
    """The limits of the C entries (ValueError outside them)."""
    if not 1 <= D <= 64:
        raise ValueError("the number of coefficients must be in [1, 64] (got %d)" % D)
    if fftlen < 4 or fftlen > 4096 or fftlen & (fftlen - 1):
        raise ValueError("fftlen must be a power of two in [4, 4096] (got %d)" % fftlen)
    if not D - 1 <= order < fftlen:
        raise ValueError("minimum_phase_order must be in [D - 1, fftlen) (got %d)" % order)
    if not abs(alpha) < 1.0:
        raise ValueError("|alpha| must be below 1 (got %r)" % (alpha,))


def post_filter_literal(mgc, alpha, minimum_phase_order=511, fftlen=1024, coef=1.4, weight=None):
    """The definition above, frame by frame in meaning, all frames of mgc (T, D) at once in execution."""
    mgc = np.asarray(mgc, dtype=np.float64)
    T, D = mgc.shape
    w = default_weight(D, coef) if weight is None else np.asarray(weight, dtype=np.float64)
    assert w.shape == (D,)
    v = w * mgc
    r0 = c2acr0(freqt(mgc, minimum_phase_order, -alpha), fftlen)
    p0 = c2acr0(freqt(v, minimum_phase_order, -alpha), fftlen)
    b = mc2b(v, alpha)
    b[:, 0] = np.log(r0 / p0) / 2 + b[:, 0]
    return b2mc(b, alpha)


def warp_matrix(D, alpha, order):
    """A (order + 1, D): column d is freqt(e_d, order, -alpha)."""
    return np.ascontiguousarray(freqt(np.eye(D), order, -alpha).T)   # the D unit vectors as D frames


def cos_matrix(order, N):
    """C (N/2 + 1, order + 1): cos(2 pi (k j mod N) / N), the phase reduced as an integer before it meets pi."""
    k = np.arange(N // 2 + 1, dtype=np.int64)[:, None]
    j = np.arange(order + 1, dtype=np.int64)[None, :]
    roots = np.cos(2.0 * np.pi * np.arange(N) / N)
    roots[0] = 1.0
    roots[N // 2] = -1.0
    roots[N // 4] = roots[3 * N // 4] = 0.0
    return roots[(k * j) % N]


def table(D, alpha, order, N):
    """G (N/2 + 1, D) = C A: Re of the N-point DFT of freqt(c, order, -alpha) is G c."""
    return cos_matrix(order, N) @ warp_matrix(D, alpha, order)


def r0_from_table(c, G, N):
    """c2acr0(freqt(c, order, -alpha), N) through the half spectrum: bins 0 and N/2 count once, the others twice."""
    wk = np.full(N // 2 + 1, 2.0)
    wk[0] = wk[-1] = 1.0
    return (np.exp(2.0 * (np.asarray(c, dtype=np.float64) @ G.T)) * wk).sum(axis=-1) / N


def post_filter_table(mgc, alpha, G, fftlen, weight):
    """The form the kernel uses: two products with G, exponentials, two sums, two recursions."""
    mgc = np.asarray(mgc, dtype=np.float64)
    w = np.asarray(weight, dtype=np.float64)
    v = w * mgc
    r0 = r0_from_table(mgc, G, fftlen)
    p0 = r0_from_table(v, G, fftlen)
    b = mc2b(v, alpha)
    b[:, 0] = np.log(r0 / p0) / 2 + b[:, 0]
    return b2mc(b, alpha)


def post_filter_batch(mgc, alpha, minimum_phase_order=511, fftlen=1024, coef=1.4, weight=None, lengths=None, form="literal"):
    """Padded batch (B, Tmax, D): utterance b's frames [0, min(max(len_b, 0), Tmax)) are filtered, the others are never read
    (NaN there reaches nothing) and come out as exact zeros.  form: "literal" or "table"."""
    mgc = np.asarray(mgc, dtype=np.float64)
    B, Tmax, D = mgc.shape
    w = default_weight(D, coef) if weight is None else np.asarray(weight, dtype=np.float64)
    out = np.zeros_like(mgc)
    G = table(D, alpha, minimum_phase_order, fftlen) if form == "table" else None
    for b in range(B):
        n = Tmax if lengths is None else min(max(int(lengths[b]), 0), Tmax)
        if n == 0:
            continue
        if form == "table":
            out[b, :n] = post_filter_table(mgc[b, :n], alpha, G, fftlen, w)
        else:
            out[b, :n] = post_filter_literal(mgc[b, :n], alpha, minimum_phase_order, fftlen, weight=w)
    return out
