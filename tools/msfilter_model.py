"""Executable specification of the modulation-spectrum filter (csrc/modspec_filter.hip,
``postfilters.modspec_post_filter_batch``, ``preprocessing.modspec_smoothing_batch``).  numpy only; ``numpy.fft`` does the transforms.

The post-filter (Takamichi et al., ICASSP 2014 / TASLP 2016) moves the log modulation spectrum ``s = log |rfft(x, n)|^2`` of a
generated trajectory toward natural-speech statistics, per (bin, column), and keeps the phase:

    s' = (1 - k) s + k [(sigma_N / sigma_G)(s - mu_G) + mu_N] = A s + C
    A  = 1 - k + k sigma_N / sigma_G,      C = k (mu_N - (sigma_N / sigma_G) mu_G)

One utterance ``x`` of ``live <= n`` frames, per column d, ``nb = n/2 + 1``:

1. ``S = rfft(x[:, d], n)`` (times ``1/sqrt(n)`` for ``norm="ortho"``), ``P = |S|^2``;
2. table bins ``k < limit_bin``: ``P'_k = exp(A[k, d] log P_k + C[k, d])`` where ``P_k > 0``, 0 where ``P_k == 0``; without
   tables ``P' = P``;
3. removed bins ``k >= limit_bin``: ``modspec_smoothing``'s rule -- in the log domain the log-power becomes 0 (``P' = exp(0)``,
   also for a zero bin, whose phase numpy gives as 1), otherwise ``P' = 0``;
4. ``y = irfft(sqrt(P') * exp(i angle S), n)[:live]`` with the same norm.

``filter_literal`` is that text.  ``filter_gain`` is the form the kernel uses: the phase is kept, so ``S' = S * g`` with the real
gain ``g = exp(((A - 1) log P + C) / 2)``, and ``S / |S|`` or 0 in the removed bins.  ``filter_batch`` adds the padded-batch rules:
``live_b = min(max(lengths[b], 0), Tmax)``, nothing at or past ``live_b`` is read, rows ``live_b <= t < Tmax`` of the output are
0, an utterance with ``live_b == 0`` computes nothing.  ``log_stats`` and ``tables`` are the statistics and the table builder.
"""
import numpy as np


def live_frames(lengths, B, T):
    L = np.full(B, T, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
    assert L.shape == (B,)
    return np.clip(L, 0, T)


def limit_bin_of(n, modfs, cutoff):
    """First removed bin (the reference's preprocessing/modspec.py:145-163); cutoff None removes nothing."""
    nb = n // 2 + 1
    if cutoff is None:
        return nb
    if cutoff > modfs // 2:
        raise ValueError("cutoff above Nyquist")
    return min(int(n * cutoff / modfs) + 1, nb)


def _check(x, n, A, C, limit_bin):
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 2 and n >= 2 and n % 2 == 0 and x.shape[0] <= n
    nb = n // 2 + 1
    limit_bin = nb if limit_bin is None else int(limit_bin)
    assert 0 <= limit_bin <= nb and (A is None) == (C is None)
    if A is not None:
        A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
        assert A.shape == C.shape == (nb, x.shape[1])
    return x, nb, limit_bin, A, C


def filter_literal(x, n, norm=None, A=None, C=None, limit_bin=None, log_domain=True):
    """The definition, word for word: (live, D) -> (live, D)."""
    x, nb, limit_bin, A, C = _check(x, n, A, C, limit_bin)
    S = np.fft.rfft(x, n=n, axis=0, norm=norm)
    P = S.real ** 2 + S.imag ** 2
    phase = np.exp(1j * np.angle(S))
    Pn = P.copy()
    if A is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            Pn[:limit_bin] = np.where(P[:limit_bin] > 0, np.exp(A[:limit_bin] * np.log(P[:limit_bin]) + C[:limit_bin]), 0.0)
    Pn[limit_bin:] = np.exp(0.0) if log_domain else 0.0
    return np.ascontiguousarray(np.fft.irfft(np.sqrt(Pn) * phase, n=n, axis=0, norm=norm)[:x.shape[0]])


def filter_gain(x, n, norm=None, A=None, C=None, limit_bin=None, log_domain=True):
    """The kernel's form: one real gain per table bin on the complex spectrum, S / |S| or 0 in the removed bins."""
    x, nb, limit_bin, A, C = _check(x, n, A, C, limit_bin)
    S = np.fft.rfft(x, n=n, axis=0, norm=norm)
    P = S.real ** 2 + S.imag ** 2
    Sn = S.copy()
    if A is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(P > 0, np.exp(0.5 * ((A - 1.0) * np.log(P) + C)), 0.0)
        Sn[:limit_bin] = (S * g)[:limit_bin]
    if log_domain:
        mag = np.hypot(S.real, S.imag)
        with np.errstate(divide="ignore", invalid="ignore"):
            Sn[limit_bin:] = np.where(mag > 0, S / mag, 1.0)[limit_bin:]
    else:
        Sn[limit_bin:] = 0.0
    return np.ascontiguousarray(np.fft.irfft(Sn, n=n, axis=0, norm=norm)[:x.shape[0]])


def filter_batch(X, n, norm=None, lengths=None, A=None, C=None, limit_bin=None, log_domain=True, form=filter_literal):
    """(B, Tmax, D) -> (B, Tmax, D) float64 by the padded-batch rules; what lies at or past live_b is never looked at."""
    X = np.asarray(X)
    B, T, D = X.shape
    assert T <= n
    live = live_frames(lengths, B, T)
    out = np.zeros((B, T, D))
    for b in range(B):
        if live[b]:
            out[b, :live[b]] = form(X[b, :live[b]].astype(np.float64), n, norm, A, C, limit_bin, log_domain)
    return out


def log_ms(X, n, norm=None, lengths=None):
    """log |rfft(x[b, :live_b], n)|^2 of the utterances with live_b > 0 (live_b = min(len_b, Tmax, n)): (B', n/2+1, D)."""
    X = np.asarray(X, dtype=np.float64)
    B, T, D = X.shape
    live = np.minimum(live_frames(lengths, B, T), n)
    rows = []
    for b in range(B):
        if live[b]:
            S = np.fft.rfft(X[b, :live[b]], n=n, axis=0, norm=norm)
            with np.errstate(divide="ignore"):
                rows.append(np.log(S.real ** 2 + S.imag ** 2))
    return np.stack(rows) if rows else np.zeros((0, n // 2 + 1, D))


def log_stats(X, n, norm=None, lengths=None):
    """(mean, population standard deviation) of log MS over the batch's live utterances, per (bin, column)."""
    s = log_ms(X, n, norm, lengths)
    assert len(s), "no utterance with a live frame"
    return s.mean(axis=0), s.std(axis=0, ddof=0)


def tables(gen_mean, gen_std, nat_mean, nat_std, k=0.85):
    """(A, C); the identity (A = 1, C = 0) where an input is not finite or sigma_G <= 0."""
    mg, sg, mn, sn = (np.asarray(t, dtype=np.float64) for t in (gen_mean, gen_std, nat_mean, nat_std))
    ok = np.isfinite(mg) & np.isfinite(sg) & np.isfinite(mn) & np.isfinite(sn) & (sg > 0)
    with np.errstate(all="ignore"):
        ratio = sn / np.where(ok, sg, 1.0)
        A = np.where(ok, 1.0 - k + k * ratio, 1.0)
        C = np.where(ok, k * (mn - ratio * mg), 0.0)
    return A, C
