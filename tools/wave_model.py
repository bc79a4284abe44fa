"""Executable specification of the waveform kernels (csrc/wave_codec.hip, include/nnmnkwii_wave.h), in numpy.

  literal   the definitions: the reference's six functions (preprocessing/generic.py:56-226) restated with the two deliberate
            deviations of the header -- mu-law is evaluated in float64 on the value as read and rounded once to the input's
            dtype, and the class is that float64 value truncated.  ``preemphasis``, ``inv_preemphasis`` (the sequential
            recurrence in the input's dtype: the reference's bits), ``inv_mulaw_table`` / ``inv_mulaw_quantize`` equal the
            reference bit for bit.
  tiled     the decode kernel's partition, plan and order of operations: ``plan`` (nnmk_wave_plan), ``powers`` (the twelve
            multipliers), ``decode`` (front end, the walk in tiles with the Kogge-Stone scan, segments with their warm-up, one
            rounding on store).  The kernel equals it bit for bit wherever no device transcendental is involved (every front end
            but the float inv_mulaw).  The tile is a parameter so that the partition can be tested against ``truth``.
  batch     ``encode_batch`` / ``decode_batch``: padded batches with the header's padding rules.
  truth     the exact recurrence in rational arithmetic (integers over a power-of-two denominator: Fractions without the gcd).
  bounds    ``ref_bound``: the running a-posteriori bound of the reference's sequential recurrence;  the walk returns the
            running bound of its own order of operations next to its values (first order in u, every operation counted, the
            relative errors of the multipliers included, and the truncation |c|^W |Y| of a segment's zero start).
"""
import numpy as np

TILE = 1024
TABLE_LDS = 4096
AUTO_SEGMENT = 16384                 # kWaveAutoSegment
F32, F64, U8, I16, I32, I64 = range(6)
PLAIN, MULAW, QUANTIZE = range(3)
NP_DTYPE = {F32: np.dtype(np.float32), F64: np.dtype(np.float64), U8: np.dtype(np.uint8), I16: np.dtype(np.int16),
            I32: np.dtype(np.int32), I64: np.dtype(np.int64)}
CODE = {v: k for k, v in NP_DTYPE.items()}
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
# documented errors in ulp: the device's float64 log1p (OpenCL accuracy table: 2) and pow (16), numpy's (1)
E_LOG1P_DEVICE, E_POW_DEVICE, E_NUMPY = 2, 16, 1
MULAW_ULPS = 2 * E_LOG1P_DEVICE + 2 * E_NUMPY + 5          # two log1p calls and 2.5 roundings a side
INV_MULAW_ULPS = E_POW_DEVICE + E_NUMPY + 4                # pow a side and 4 roundings


# ---- literal ----------------------------------------------------------------------------------------------------------------------

def _float_in(x, who):
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError("%s: float32 or float64 only, got %s" % (who, x.dtype))
    return x


def preemphasis(x, coef=0.97):
    """y[0] = x[0], y[n] = fl(x[n] + fl(fl(-coef) x[n-1])) in x's dtype: bit for bit lfilter([1, -coef], [1], x)."""
    x = _float_in(x, "preemphasis")
    nc = x.dtype.type(-x.dtype.type(coef))
    y = x + x.dtype.type(0)                      # (the filter's state starts at +0.0: a first sample of -0.0 comes out as +0.0)
    y[1:] = x[1:] + nc * x[:-1]
    return y


def inv_preemphasis(x, coef=0.97):
    """The sequential recurrence y[n] = fl(x[n] + fl(c y[n-1])) in x's dtype: bit for bit lfilter([1], [1, -coef], x)."""
    x = _float_in(x, "inv_preemphasis")
    T = x.dtype.type
    c = T(coef)
    y = np.empty_like(x)
    prev = T(0)
    with np.errstate(all="ignore"):
        for n in range(len(x)):
            prev = T(x[n] + T(c * prev)) if n else T(x[0] + T(0))
            y[n] = prev
    return y


def _mulaw64(d, mu):
    with np.errstate(all="ignore"):
        return np.sign(d) * np.log1p(mu * np.abs(d)) / np.log1p(float(mu))


def mulaw(x, mu=256):
    """sign(x) log1p(mu |x|) / log1p(mu) in float64 on x as read, rounded once to x's dtype."""
    x = _float_in(x, "mulaw")
    return _mulaw64(x.astype(np.float64), mu).astype(x.dtype)


def mulaw_v(x, mu=256):
    """The float64 value whose truncation is the class: (mulaw + 1) / 2 * mu."""
    x = _float_in(x, "mulaw_quantize")
    return (_mulaw64(x.astype(np.float64), mu) + 1.0) / 2.0 * mu


def classes_of(v):
    """v truncated toward zero as int64; NaN gives 0."""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(v), 0.0, np.clip(v, -2.0 ** 62, 2.0 ** 62)).astype(np.int64)


def mulaw_quantize(x, mu=256):
    return classes_of(mulaw_v(x, mu))


def inv_mulaw(y, mu=256):
    """sign(y) (1 / mu) ((1 + mu)^|y| - 1) in float64 on y as read, rounded once to y's dtype."""
    y = _float_in(y, "inv_mulaw")
    return _inv_mulaw64(y.astype(np.float64), mu).astype(y.dtype)


def _inv_mulaw64(d, mu):
    with np.errstate(all="ignore"):
        return np.sign(d) * (1.0 / mu) * ((1.0 + mu) ** np.abs(d) - 1.0)


def inv_mulaw_table(mu=256):
    """The reference's inv_mulaw_quantize on arange(mu + 1), its literal expression: float32 (mu + 1)."""
    y = np.arange(int(mu) + 1).astype(np.float32)
    y = 2 * y / mu - 1
    return np.asarray(np.sign(y) * (1.0 / mu) * ((1.0 + mu) ** np.abs(y) - 1.0), dtype=np.float32)


def inv_mulaw_quantize(y, mu=256):
    """table[class], classes clamped to [0, mu]: float32."""
    return inv_mulaw_table(mu)[np.clip(np.asarray(y).astype(np.int64), 0, int(mu))]


def silence(mu):
    return int((0 + 1) / 2 * mu)


# ---- the plan and the multipliers -------------------------------------------------------------------------------------------------

def warm_up(coef, tile=TILE):
    """The smallest positive multiple W of the tile with |coef|^W <= 2^-80, by the header's recipe (-1: none)."""
    p = abs(float(coef))
    t = 1
    while t < tile:                    # |c|^tile by squaring (ten squarings at the real tile)
        p = p * p
        t *= 2
    assert t == tile, "the tile must be a power of two here"
    if not p < 1.0:
        return -1
    q, k = p, 1
    while q > 2.0 ** -80 and k < (1 << 20):
        q = q * p
        k += 1
    return k * tile if q <= 2.0 ** -80 else -1


def plan(Lmax, coef, segment=0, tile=TILE, auto=AUTO_SEGMENT):
    """(S, W, nseg) of nnmk_wave_plan; ValueError where it returns -1."""
    W = warm_up(coef, tile)
    S = Lmax
    if segment < 0:
        raise ValueError("wave: negative segment")
    if segment == 0:
        if Lmax > auto and 0 < W <= auto // 4:
            S = auto
    elif segment < Lmax:
        if segment % tile:
            raise ValueError("wave: segment is no multiple of the tile")
        if W < 0 or W > segment:
            raise ValueError("wave: segment is too short for this coef")
        S = segment
    return S, W, (-(-Lmax // S) if S < Lmax else 1)


def powers(c, steps=8):
    """(c^(4 2^s) for s < steps, (c, c^2, c^3, c^4)) as the host computes them, and their relative errors in u."""
    c2 = c * c
    pw, rel = [c2 * c2], [3]
    for _ in range(1, steps):
        pw.append(pw[-1] * pw[-1])
        rel.append(2 * rel[-1] + 1)
    return pw, rel, [c, c2, c2 * c, pw[0]], [0, 1, 2, 3]


# ---- tiled ------------------------------------------------------------------------------------------------------------------------

_U = 2.0 ** -53


def _axpy(a, ea, m, rel_m, b, eb):
    """q = fl(a + fl(m b)) and the bound of |q - exact|, given those of a and b and the multiplier's relative error (in u)."""
    with np.errstate(all="ignore"):
        t = m * b
        q = a + t
        e = (ea + np.abs(m) * eb + (rel_m + 1) * _U * np.abs(t) + _U * np.abs(q)) * (1 + 2.0 ** -40)
    return q, e


def _walk(v, c, start, lo, hi, tile, e0):
    """The workgroup's walk over v[start:hi] from a zero state, storing [lo, hi): (values float64, running bound).  e0: the bound of
    the true state in front of `start` (the zero start's truncation)."""
    nt = tile // 4
    nw = -(-nt // 64)
    NT = nw * 64
    steps = 7
    while (1 << (steps - 6)) < nw:
        steps += 1
    pw, rel_pw, cp, rel_cp = powers(c, max(steps, 8))
    idx = np.arange(NT)
    lane, wave = idx % 64, idx // 64
    lanepow, rel_lp = np.ones(NT), np.zeros(NT)
    for s in range(7):
        sel = ((lane + 1) >> s) & 1 == 1
        lanepow[sel] = lanepow[sel] * pw[s]
        rel_lp[sel] += rel_pw[s] + 1
    out, bound = np.zeros(hi - lo), np.zeros(hi - lo)
    carry, ecarry = 0.0, e0
    for t0 in range(start, hi, tile):
        n = min(tile, hi - t0)
        blk = np.zeros(NT * 4)
        blk[:n] = v[t0:t0 + n]
        V, EV = blk.reshape(NT, 4), np.zeros((NT, 4))
        # local
        V[0, 0], EV[0, 0] = _axpy(V[0, 0], 0.0, c, 0, carry, ecarry)
        for m in range(1, 4):
            V[:, m], EV[:, m] = _axpy(V[:, m], EV[:, m], c, 0, V[:, m - 1], EV[:, m - 1])
        # scan
        e, ee = V[:, 3].copy(), EV[:, 3].copy()
        for s in range(6):
            off = 1 << s
            sel = idx[lane >= off]
            e2, ee2 = e.copy(), ee.copy()
            e2[sel], ee2[sel] = _axpy(e[sel], ee[sel], pw[s], rel_pw[s], e[sel - off], ee[sel - off])
            e, ee = e2, ee2
        P, eP = e[63::64].copy(), ee[63::64].copy()
        s, d = 6, 1
        while d < nw:
            P2, eP2 = P.copy(), eP.copy()
            P2[d:], eP2[d:] = _axpy(P[d:], eP[d:], pw[s], rel_pw[s], P[:-d], eP[:-d])
            P, eP = P2, eP2
            s, d = s + 1, d * 2
        in_w, ein_w = np.concatenate([[0.0], P[:-1]])[wave], np.concatenate([[0.0], eP[:-1]])[wave]
        f, ef = e.copy(), ee.copy()
        sel = wave > 0
        f[sel], ef[sel] = _axpy(e[sel], ee[sel], lanepow[sel], rel_lp[sel], in_w[sel], ein_w[sel])
        inn, einn = np.roll(f, 1), np.roll(ef, 1)
        inn[lane == 0], einn[lane == 0] = in_w[lane == 0], ein_w[lane == 0]
        for m in range(4):
            V[1:, m], EV[1:, m] = _axpy(V[1:, m], EV[1:, m], cp[m], rel_cp[m], inn[1:], einn[1:])
        carry, ecarry = f[nt - 1], ef[nt - 1]            # the tile's last thread's final value
        if t0 >= lo:
            out[t0 - lo:t0 - lo + n] = V.reshape(-1)[:n]
            bound[t0 - lo:t0 - lo + n] = EV.reshape(-1)[:n]
    return out, bound


def scan(v, c, Lmax=None, segment=None, tile=TILE, auto=AUTO_SEGMENT):
    """De-emphasis of the float64 values v (the live samples of an utterance of a batch padded to Lmax) as the kernel does it:
    (y float64 before the store's rounding, the running bound of |y - exact|).  segment: None no split, 0 automatic, else S."""
    v = np.asarray(v, dtype=np.float64)
    L = len(v)
    Lmax = L if Lmax is None else Lmax
    S, W, nseg = (Lmax, 0, 1) if segment is None else plan(Lmax, c, segment, tile, auto)
    y, E = np.zeros(L), np.zeros(L)
    for j in range(nseg):
        lo, hi = j * S, min((j + 1) * S, L)
        if lo >= hi:
            break
        start, e0 = lo, 0.0
        if j:
            start = lo - W
            e0 = abs(y[start - 1]) + E[start - 1] if start else 0.0      # the true state the zero start leaves out
        y[lo:hi], E[lo:hi] = _walk(v, float(c), start, lo, hi, tile, e0)
    return y, E


def front(x, stage, mu=256, table=None):
    """The decode front end: float64 values of what x holds."""
    x = np.asarray(x)
    if stage == QUANTIZE:
        table = inv_mulaw_table(mu) if table is None else table
        return table[np.clip(x.astype(np.int64), 0, int(mu))].astype(np.float64)
    if stage == MULAW:
        return _inv_mulaw64(x.astype(np.float64), mu)
    return x.astype(np.float64)


def decode(x, stage=PLAIN, mu=256, coef=None, segment=None, dtype=np.float32, Lmax=None, table=None, tile=TILE):
    """One utterance's live samples through nnmk_wave_decode: the result in `dtype`."""
    v = front(x, stage, mu, table)
    if coef is not None:
        v = scan(v, coef, Lmax, segment, tile)[0]
    with np.errstate(all="ignore"):
        return v.astype(dtype)


def encode(x, coef=None, stage=QUANTIZE, mu=256, dtype=None):
    """One utterance's live samples through nnmk_wave_encode."""
    x = _float_in(x, "encode")
    p = preemphasis(x, coef) if coef is not None else x
    if stage == PLAIN:
        return p.astype(x.dtype if dtype is None else dtype)
    if stage == MULAW:
        return _mulaw64(p.astype(np.float64), mu).astype(x.dtype if dtype is None else dtype)
    return mulaw_quantize(p, mu).astype(np.int64 if dtype is None else dtype)


# ---- batch ------------------------------------------------------------------------------------------------------------------------

def _live(lengths, B, Lmax):
    return [Lmax] * B if lengths is None else [int(min(max(n, 0), Lmax)) for n in lengths]


def encode_batch(X, lengths=None, coef=None, stage=QUANTIZE, mu=256, dtype=None):
    X = np.asarray(X)
    B, Lmax = X.shape
    dt = np.dtype(dtype if dtype is not None else (np.int64 if stage == QUANTIZE else X.dtype))
    Y = np.full((B, Lmax), silence(mu) if stage == QUANTIZE else 0, dtype=dt)
    for b, n in enumerate(_live(lengths, B, Lmax)):
        Y[b, :n] = encode(X[b, :n], coef, stage, mu, dt)
    return Y


def decode_batch(X, lengths=None, stage=PLAIN, mu=256, coef=None, segment=None, dtype=np.float32, table=None):
    X = np.asarray(X)
    B, Lmax = X.shape
    Y = np.zeros((B, Lmax), dtype=dtype)
    for b, n in enumerate(_live(lengths, B, Lmax)):
        Y[b, :n] = decode(X[b, :n], stage, mu, coef, segment, dtype, Lmax, table)
    return Y


# ---- truth and the reference's bound ----------------------------------------------------------------------------------------------

class Truth(object):
    """y[n] = x[n] + c y[n-1], exactly: y[n] = num[n] / 2^(q + p n) with integers num[n]."""

    def __init__(self, x, c):
        x = np.asarray(x, dtype=np.float64)
        assert np.isfinite(x).all() and np.isfinite(c)
        ratios = [float(v).as_integer_ratio() for v in x]            # denominators are powers of two
        C, cb = float(c).as_integer_ratio()
        self.p = cb.bit_length() - 1
        self.q = max([b.bit_length() - 1 for _, b in ratios] + [0])
        self.num, self.shift = [], []
        prev = 0
        for n, (a, b) in enumerate(ratios):
            k = self.q + self.p * n
            prev = a * ((1 << k) // b) + C * prev
            self.num.append(prev)
            self.shift.append(k)

    def nearest(self):
        return np.array([n / (1 << k) for n, k in zip(self.num, self.shift)])

    def distance(self, y):
        """|y[n] - exact[n]| as float64 (correctly rounded)."""
        out = np.empty(len(self.num))
        for i, (n, k) in enumerate(zip(self.num, self.shift)):
            a, b = float(y[i]).as_integer_ratio()
            kb = b.bit_length() - 1
            K = max(k, kb)
            out[i] = abs((a << (K - kb)) - (n << (K - k))) / (1 << K)
        return out


def truth(x, c):
    return Truth(x, c)


def ref_bound(y_ref, coef):
    """The running a-posteriori bound of the reference's recurrence in y_ref's dtype:
    E[n] = |c| E[n-1] + u (|c| |y[n-1]| + |y[n]|) (1 + 4 u), E[-1] = 0."""
    y_ref = np.asarray(y_ref)
    u = U[y_ref.dtype]
    c = abs(float(y_ref.dtype.type(coef)))
    a = np.abs(y_ref.astype(np.float64))
    E = np.zeros(len(a))
    prev_e, prev_a = 0.0, 0.0
    for n in range(len(a)):
        prev_e = c * prev_e + (u * (c * prev_a + a[n]) * (1 + 4 * u) if n else 0.0)
        prev_a = a[n]
        E[n] = prev_e
    return E
