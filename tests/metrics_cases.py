"""Inputs and bounds shared by the tests of the objective metrics (tests/test_metrics_*.py) and by
tests/golden/make_golden_metrics.py: acoustic-feature-like batches (cepstra, a log-F0 column whose two sides differ by at least
0.1, a 0/1 vuv column), the golden file's layout, and the tolerances, which come from tools/metrics_model.py alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import metrics_model as MM  # noqa: E402

BLOCK = MM.BLOCK_ROWS
U = MM.U


def pair(seed, B, Tmax, D, dtype=np.float64, lf0_cols=(), vuv_cols=()):
    """(X, Y) of shape (B, Tmax, D): Y = X + noise; the lf0 columns sit around 5 with |x - y| in [0.1, 0.5], the vuv columns hold
    0 / 1 and agree in about 85 % of the frames."""
    rng = np.random.RandomState(seed)
    X = rng.randn(B, Tmax, D)
    Y = X + 0.3 * rng.randn(B, Tmax, D)
    for c in lf0_cols:
        X[:, :, c] = 5.0 + 0.3 * rng.randn(B, Tmax)
        Y[:, :, c] = X[:, :, c] + np.where(rng.rand(B, Tmax) < 0.5, -1.0, 1.0) * (0.1 + 0.4 * rng.rand(B, Tmax))
    for c in vuv_cols:
        X[:, :, c] = rng.rand(B, Tmax) < 0.7
        Y[:, :, c] = np.where(rng.rand(B, Tmax) < 0.85, X[:, :, c], 1.0 - X[:, :, c])
    X, Y = X.astype(dtype), Y.astype(dtype)
    for c in lf0_cols:                      # the rounding to float32 must not bring the two sides closer than 0.1
        close = np.abs(X[:, :, c].astype(np.float64) - Y[:, :, c].astype(np.float64)) < 0.1
        Y[:, :, c] = np.where(close, X[:, :, c] + dtype(0.25), Y[:, :, c])
    return X, Y


def pad_with(A, lengths, value=np.nan):
    """A copy of A whose frames past the lengths hold `value` (NaN: a kernel that reads one shows it)."""
    A = A.copy()
    for b, n in enumerate(lengths):
        A[b, max(int(n), 0):] = value
    return A


# ---- the golden file (tests/golden/metrics_ref.npz) -------------------------------------------------------------------------
# a small Merlin-like layout: column 0 energy, 1 .. 11 cepstra, 12 lf0, 13 vuv, 14 .. 16 bap, 17 spare
G_D, G_MGC, G_LF0, G_VUV, G_BAP = 18, slice(1, 12), 12, 13, slice(14, 17)
G_LENGTHS = [BLOCK + 3, 0, 1, BLOCK, 130]
G_CASES = {"f64": (11, np.float64), "f32": (12, np.float32)}


def golden_inputs(name):
    seed, dtype = G_CASES[name]
    X, Y = pair(seed, len(G_LENGTHS), max(G_LENGTHS), G_D, dtype, lf0_cols=(G_LF0,), vuv_cols=(G_VUV,))
    lengths = np.array(G_LENGTHS, dtype=np.int32)
    return pad_with(X, lengths, 0.0), pad_with(Y, lengths, 0.0), lengths


def golden_calls(M, X, Y, lengths):
    """name -> value of every call of the four functions the golden file records; M: the module under test (or the reference)."""
    L = [int(n) for n in lengths]
    f0x, vx, f0y, vy = X[:, :, G_LF0], X[:, :, G_VUV], Y[:, :, G_LF0], Y[:, :, G_VUV]
    u = 3                                                                  # a full-block utterance for the forms without lengths
    n = L[u]
    return {
        "melcd/lengths": M.melcd(X[:, :, G_MGC], Y[:, :, G_MGC], L),
        "melcd/one_feature": M.melcd(X[:, :, 0], Y[:, :, 0], L),           # (B, T) with lengths
        "melcd/utterance": M.melcd(X[u, :n, G_MGC], Y[u, :n, G_MGC]),      # (T, D)
        "melcd/frame": M.melcd(X[u, 7, G_MGC], Y[u, 7, G_MGC]),            # (D,)
        "mse/lengths": M.mean_squared_error(X[:, :, G_BAP], Y[:, :, G_BAP], L),
        "mse/utterance": M.mean_squared_error(X[u, :n, G_BAP], Y[u, :n, G_BAP]),
        "mse/batch": M.mean_squared_error(X[3:4, :n, G_MGC], Y[3:4, :n, G_MGC]),   # (B, T, D) without lengths
        "lf0/lengths": M.lf0_mean_squared_error(f0x, vx, f0y, vy, L),
        "lf0/lengths_linear": M.lf0_mean_squared_error(f0x, vx, f0y, vy, L, linear_domain=True),
        "lf0/lengths_3d": M.lf0_mean_squared_error(f0x[:, :, None], vx[:, :, None], f0y[:, :, None], vy[:, :, None], L),
        "lf0/utterance": M.lf0_mean_squared_error(f0x[u, :n], vx[u, :n], f0y[u, :n], vy[u, :n]),
        "lf0/utterance_linear": M.lf0_mean_squared_error(f0x[u, :n], vx[u, :n], f0y[u, :n], vy[u, :n], linear_domain=True),
        "vuv/lengths": M.vuv_error(vx, vy, L),
        "vuv/lengths_3d": M.vuv_error(vx[:, :, None], vy[:, :, None], L),
        "vuv/utterance": M.vuv_error(vx[u, :n], vy[u, :n]),
    }


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "metrics_ref.npz"))


def golden_terms():
    """The golden file's four batch figures as terms of one evaluation, with the names of golden_calls."""
    return {"melcd/lengths": MM.term(MM.FRAME_L2, G_MGC.start, width=G_MGC.stop - G_MGC.start),
            "melcd/one_feature": MM.term(MM.FRAME_L2, 0),
            "mse/lengths": MM.term(MM.SQUARED, G_BAP.start, width=G_BAP.stop - G_BAP.start),
            "lf0/lengths": MM.term(MM.VOICED_SQUARED, G_LF0, x_mask_col=G_VUV),
            "lf0/lengths_linear": MM.term(MM.VOICED_SQUARED, G_LF0, x_mask_col=G_VUV, flags=MM.FLAG_EXP),
            "vuv/lengths": MM.term(MM.MISMATCH, G_VUV)}


def figure(name, pair_):
    return MM.value({"melcd": "melcd", "mse": "mse", "lf0": "lf0_mse", "vuv": "vuv_error"}[name.split("/")[0]], pair_)


# ---- tolerances -------------------------------------------------------------------------------------------------------------
def rel_bound(B, Tmax, t):
    """Relative bound of a term's sum from nnmk_metrics_batch against the truth: tools/metrics_model.py bound()."""
    return MM.bound(B, Tmax, t)


def reference_bound(B, Tmax, t, dtype):
    """Relative bound against the reference's own value of the golden file.  float64 inputs: the reference adds the same
    non-negative summands in float64 in another order (numpy's pairwise sums, a Python loop over the utterances), so twice the
    kernel's bound covers both.  float32 inputs: the reference computes in float32 -- difference, square (2 + 1 roundings),
    a square root or exponentials of float32 accuracy, pairwise sums of at most 128 / 8 + 3 + log2(n / 128) additions per
    utterance and one addition per utterance -- so its own error, in units of 2^-24, is at most that count plus the same EXP
    term as the model's, and dominates the kernel's."""
    if np.dtype(dtype) == np.float64:
        return 2 * MM.bound(B, Tmax, t)
    n = max(Tmax * t["width"], 129)
    chain = 3 + 1 + 16 + 3 + int(np.ceil(np.log2(n / 128.0))) + B
    extra = 2 * 21 * 2 if t["flags"] & MM.FLAG_EXP else 0
    return (chain + extra) * 2.0 ** -24 + MM.bound(B, Tmax, t)


def close(got, want, rel):
    """|got - want| <= rel * |want|, NaN only where both are."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all((np.abs(got - want) <= rel * np.abs(want)) | (np.isnan(got) & np.isnan(want))))


# ---- the kernel's cases -----------------------------------------------------------------------------------------------------
LF0, VUV = 60, 61


def eight_terms():
    """Eight terms at non-zero, overlapping column offsets (x_col != y_col in two of them) of rows at least 134 wide: widths 1,
    59, 64, 65 and 129, every kind, both voiced rules, both mismatch rules.  Columns LF0 and VUV are pair()'s lf0 and vuv ones."""
    T = MM.term
    return [T(MM.FRAME_L2, 1, width=59), T(MM.FRAME_L2, 3, 5, width=129), T(MM.SQUARED, 62, width=65), T(MM.SQUARED, 10, 9, width=64),
            T(MM.VOICED_SQUARED, LF0, x_mask_col=VUV), T(MM.VOICED_SQUARED, LF0, x_mask_col=VUV, flags=MM.FLAG_EXP, threshold=0.5),
            T(MM.MISMATCH, VUV), T(MM.MISMATCH, 100, 101, threshold=0.0)]


def used_columns(terms, D, side):
    """Mask (D,) of the columns of x (side "x") or y (side "y") some term reads."""
    used = np.zeros(D, dtype=bool)
    for t in terms:
        used[t[side + "_col"]:t[side + "_col"] + t["width"]] = True
        if t["kind"] == MM.VOICED_SQUARED:
            used[t[side + "_mask_col"]] = True
    return used


def kernel_case(seed, lengths, Tmax, D, dtype_x, dtype_y, terms):
    """(X, Y, lengths int32): pair() with the pad frames and the columns no term reads holding NaN."""
    B = len(lengths)
    X, Y = pair(seed, B, Tmax, D, np.float64, lf0_cols=(LF0,), vuv_cols=(VUV,))
    X, Y = X.astype(dtype_x), Y.astype(dtype_y)
    close_ = np.abs(X[:, :, LF0].astype(np.float64) - Y[:, :, LF0].astype(np.float64)) < 0.1
    Y[:, :, LF0] = np.where(close_, X[:, :, LF0].astype(dtype_y) + dtype_y(0.25), Y[:, :, LF0])
    X[:, :, ~used_columns(terms, D, "x")] = np.nan
    Y[:, :, ~used_columns(terms, D, "y")] = np.nan
    L = np.asarray(lengths, dtype=np.int32)
    live = MM.live_frames(L, B, Tmax)
    return pad_with(X, live), pad_with(Y, live), L


def term_bytes(terms):
    """The terms as an array of nnmk_metrics_term (40 bytes each: seven int32, four bytes of padding, a double)."""
    dt = np.dtype([("kind", "<i4"), ("x_col", "<i4"), ("y_col", "<i4"), ("width", "<i4"), ("x_mask_col", "<i4"), ("y_mask_col", "<i4"),
                   ("flags", "<i4"), ("threshold", "<f8")], align=True)
    assert dt.itemsize == 40
    a = np.zeros(len(terms), dtype=dt)
    for i, t in enumerate(terms):
        for k in dt.names:
            a[i][k] = t[k]
    return a


def check_against_model(totals, per_utt, X, Y, lengths, terms, model=None):
    """Bits of the model's kernel order (terms with the EXP flag: within the two exponentials' share of the bound), counts exact,
    and within bound() of the truth.  Returns the worst error / bound."""
    B, Tmax = X.shape[:2]
    m_per, m_tot = model if model is not None else MM.kernel_order(X, Y, lengths, terms)
    t_per, t_tot = MM.truth(X, Y, lengths, terms)
    worst = 0.0
    for i, t in enumerate(terms):
        rel = MM.bound(B, Tmax, t)
        for got, want, exact in ((totals, m_tot, t_tot), (per_utt, m_per, t_per)):
            if got is None:
                continue
            g, w, e = got[..., i, :], want[..., i, :], exact[..., i, :]
            assert np.array_equal(g[..., 1], e[..., 1]), ("count", i, g[..., 1], e[..., 1])
            if t["flags"] & MM.FLAG_EXP:
                assert close(g[..., 0], w[..., 0], 2 * 21 * 2 * U), ("model, exp", i, g[..., 0], w[..., 0])
            else:
                assert np.array_equal(g[..., 0].view(np.int64), w[..., 0].view(np.int64)), ("model bits", i, g[..., 0], w[..., 0])
            assert close(g[..., 0], e[..., 0], rel), ("truth", i, g[..., 0], e[..., 0], rel)
            with np.errstate(all="ignore"):
                r = np.nanmax(np.where(e[..., 0] > 0, np.abs(g[..., 0] - e[..., 0]) / e[..., 0], 0.0)) / rel
            worst = max(worst, float(r))
    return worst
