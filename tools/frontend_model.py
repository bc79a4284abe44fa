"""Executable specification of frame expansion (include/nnmnkwii_frontend.h; csrc/frame_expand.hip): the step of
the reference's ``frontend.merlin.linguistic_features(..., add_frame_features=True, subphone_features=...)`` that depends on the
durations.  The phone-level matrix P (n, Dl) -- the answers to the question set, which need text and no durations -- is an
input; durations d (n, S) turn it into one row per frame: P[phone] followed by the sub-phone columns.

Everything is plain Python floats (IEEE float64) on exactly represented integers: every quotient below is ONE division, the
products in ``uniform_state`` and ``coarse_coding`` ONE multiplication, the optional affine map one multiplication and one
addition, each rounded.  The kernel performs the same operations (compiled with -ffp-contract=off), so the two agree bit for bit
and the tests compare with ``np.array_equal``.

Durations in frames: r = rint(d) for floating-point durations (half to even), d itself for integers; then anything that is not
greater than min_frames -- NaN included -- becomes min_frames, and anything above 2^31 - 1 counts as 2^31 - 1 (no output holds
that many rows).  min_frames defaults to 0 for integer durations and to 1 for floating-point ones (the Merlin recipe's
``np.round`` followed by ``<= 0 -> 1``).  States and whole phones of 0 frames produce no rows and no division."""
import numpy as np

KINDS = (None, "full", "minimal_frame", "state_only", "frame_only", "uniform_state", "coarse_coding", "minimal_phoneme")
SIZES = (0, 9, 2, 1, 1, 2, 4, 3)
NONE, FULL, MINIMAL_FRAME, STATE_ONLY, FRAME_ONLY, UNIFORM_STATE, COARSE_CODING, MINIMAL_PHONEME = range(8)
MAX_FRAMES = 2 ** 31 - 1
MAX_S = 8
BLOCK_ROWS = 64          # NNMK_FRONTEND_BLOCK_ROWS
MAX_STATES = 8192        # NNMK_FRONTEND_MAX_STATES
CC_POINTS = 600


def kind_of(subphone_features):
    """The kind's number (the order of KINDS); the reference's ValueErrors for "none" and unknown names."""
    if subphone_features is None:
        return NONE
    name = subphone_features.strip().lower()
    if name == "none":
        raise ValueError("subphone_features = 'none' is deprecated, use None instead")
    if name not in KINDS:
        raise ValueError("Unknown value for subphone_features: %s" % (name,))
    return KINDS.index(name)


def get_frame_feature_size(subphone_features="full"):
    return SIZES[kind_of(subphone_features)]


def coarse_coding_table():
    """The reference's compute_coarse_coding_features(): three normal densities (sigma 0.4; mu 0, 0.5, 1) on 600 points each,
    float64 (3, 600), from the closed form (the reference asks scipy.stats.norm; the values are the same bits)."""
    cc = np.zeros((3, CC_POINTS))
    for k, (lo, hi, mu) in enumerate(((-1.5, 1.5, 0.0), (-1.0, 2.0, 0.5), (-0.5, 2.5, 1.0))):
        z = (np.linspace(lo, hi, CC_POINTS) - mu) / 0.4
        cc[k] = np.exp(-z ** 2 / 2.0) / np.sqrt(2 * np.pi) / 0.4
    return cc


def default_min_frames(durations):
    return 1 if np.asarray(durations).dtype.kind == "f" else 0


def frames(durations, min_frames=None):
    """Durations -> frames per state, int64, same shape."""
    d = np.asarray(durations)
    mf = default_min_frames(d) if min_frames is None else int(min_frames)
    if mf < 0:
        raise ValueError("min_frames must be at least 0, got %d" % mf)
    if d.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            r = np.rint(d.astype(np.float64))
            r = np.where(r > mf, r, float(mf))            # NaN compares false: min_frames
            r = np.minimum(r, float(MAX_FRAMES))
        return r.astype(np.int64)
    if d.dtype.kind not in "iu":
        raise ValueError("durations must be integers or floating point, got %s" % d.dtype)
    return np.minimum(np.maximum(d.astype(np.int64), mf), MAX_FRAMES)


def frame_count(durations, min_frames=None):
    return int(frames(durations, min_frames).sum())


def subphone_row(kind, cc, S, s, i, fn, base, pd):
    """The sub-phone columns of frame i (from 0) of state s (from 1) of fn frames, `base` frames into a phone of pd frames."""
    j = base + i
    if kind == FULL:
        return [float(i + 1) / float(fn), float(fn - i) / float(fn), float(fn), float(s), float(S + 1 - s), float(pd),
                float(fn) / float(pd), float(pd - i - base) / float(pd), float(base + i + 1) / float(pd)]
    if kind == MINIMAL_FRAME:
        return [float(i + 1) / float(fn), float(s)]
    if kind == STATE_ONLY:
        return [float(s)]
    if kind == FRAME_ONLY:
        return [float(j + 1) / float(pd)]
    if kind == UNIFORM_STATE:
        x = float(j + 1) / float(pd)
        return [x, float(max(1, round(x * 5)))]           # (the literal 5 is the reference's; round: half to even)
    if kind == COARSE_CODING:
        q = int((200 / float(pd)) * j)
        return [float(np.float32(cc[0, 300 + q])), float(np.float32(cc[1, 200 + q])), float(np.float32(cc[2, 100 + q])), float(pd)]
    if kind == MINIMAL_PHONEME:
        return [float(j + 1) / float(pd), float(pd - j) / float(pd), float(pd)]
    return []


def frame_features(P, durations, subphone_features="full", min_frames=None, scale_=None, min_=None, dtype=np.float64, cc=None,
                   with_phone=False):
    """One utterance, frame by frame: P (n, Dl), durations (n, S) -> (T, Dl + F) of `dtype` (computed in float64, rounded once).
    scale_, min_ (Dl + F,): v -> v * scale_[c] + min_[c], the multiplication and the addition each rounded.  with_phone: also
    each frame's phone index."""
    kind = kind_of(subphone_features)
    P = np.asarray(P)
    d = np.asarray(durations)
    if P.ndim != 2 or d.ndim != 2 or d.shape[0] != P.shape[0] or not 1 <= d.shape[1] <= MAX_S:
        raise ValueError("frame_features: P (n, Dl) and durations (n, S) with S in 1 .. %d, got %s and %s" % (MAX_S, P.shape, d.shape))
    n, S = d.shape
    Dl, F = P.shape[1], SIZES[kind]
    r = frames(d, min_frames)
    if kind == COARSE_CODING and cc is None:
        cc = coarse_coding_table()
    rows, phone = [], []
    for p in range(n):
        pd = int(r[p].sum())
        base = 0
        for s in range(1, S + 1):
            fn = int(r[p, s - 1])
            for i in range(fn):
                row = np.empty(Dl + F)
                row[:Dl] = P[p]
                row[Dl:] = subphone_row(kind, cc, S, s, i, fn, base, pd)
                rows.append(row)
                phone.append(p)
            base += fn
    out = np.array(rows, dtype=np.float64).reshape(len(rows), Dl + F)
    if (scale_ is None) != (min_ is None):
        raise ValueError("frame_features: scale_ and min_ go together")
    if scale_ is not None:
        out = out * np.asarray(scale_, dtype=np.float64) + np.asarray(min_, dtype=np.float64)
    out = out.astype(dtype)
    return (out, np.array(phone, dtype=np.int64)) if with_phone else out


def frame_features_batch(P, durations, num_phones=None, subphone_features="full", min_frames=None, scale_=None, min_=None, Tmax=None,
                         dtype=np.float64, cc=None):
    """A padded batch: P (B, Nmax, Dl), durations (B, Nmax, S), num_phones (B) or None (clamped to [0, Nmax]).  Returns (out
    (B, Tmax, Dl + F) with zeros behind each utterance's rows, lengths (B) = min(T_b, Tmax), counts (B) = T_b).  Tmax None: the
    longest utterance."""
    P, d = np.asarray(P), np.asarray(durations)
    B, Nmax = d.shape[:2]
    n = np.full(B, Nmax) if num_phones is None else np.clip(np.asarray(num_phones, dtype=np.int64), 0, Nmax)
    each = [frame_features(P[b, :n[b]], d[b, :n[b]], subphone_features, min_frames, scale_, min_, dtype, cc) for b in range(B)]
    counts = np.array([len(e) for e in each], dtype=np.int64)
    if Tmax is None:
        Tmax = int(counts.max()) if B else 0
    out = np.zeros((B, Tmax, P.shape[2] + get_frame_feature_size(subphone_features)), dtype=dtype)
    for b, e in enumerate(each):
        out[b, :min(len(e), Tmax)] = e[:Tmax]
    return out, np.minimum(counts, Tmax).astype(np.int32), counts
