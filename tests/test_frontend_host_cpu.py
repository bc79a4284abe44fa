"""The text of csrc/frame_expand.hip run on the CPU (-m "not gpu"): compiled for the host against the shim
tests/gmm_host/common.h plus tests/frontend_host/extras.h into a stand-alone program under the address and undefined-behaviour
sanitizers, run as a child process, and compared with tools/frontend_model.py bit for bit (``np.array_equal``, the contract
tests/test_frontend_gpu.py holds).  This checks the index logic: the int64 scan, the saturated running counts in LDS (an
exact-size heap block), the binary search, the second column pass at Dl + F > 64.  Every array is an exact-size heap block; the
phone matrix is a column slice of wider rows whose other columns hold NaN; phone rows at or past num_phones[b] hold NaN and
durations there NaN or INT32_MAX / INT64_MAX (one such read saturates the sum); the output is pre-filled with -7 and its foreign
columns must still hold it.  Nothing is loaded into Python under a sanitizer.

Two planted defects (and a third) show that the harness bites: see test_planted_*."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frontend_model as FM  # noqa: E402

BLOCK = FM.BLOCK_ROWS
DT_CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}
DUR_DTYPES = (np.int32, np.int64, np.float32, np.float64)
MARKER = "extern __shared__ double fx_lds[];"
SENTINEL = -7
WORST = {"runs": 0, "unequal": 0}


def build(d, edit=None):
    """The host program of the kernel text in directory d; `edit` (old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "frame_expand.hip")).read()
    assert src.count(MARKER) == 1
    src = src.replace(MARKER, "double *fx_lds = g_dyn_lds;")
    if edit is not None:
        assert src.count(edit[0]) == 1, edit[0]
        src = src.replace(edit[0], edit[1])
    os.makedirs(d / "csrc" / "x")
    os.makedirs(d / "include")
    (d / "csrc" / "x" / "frame_expand_host.inc").write_text(src)
    (d / "include" / "nnmnkwii_frontend.h").write_text(open(os.path.join(ROOT, "include", "nnmnkwii_frontend.h")).read())
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/frontend_host", "extras.h"), ("tests/frontend_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "frontend_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("frontend_host"))


def host_expand(program, P, d, n, kind, min_frames, scale, mins, out_dtype, Tmax, ld_p, ld_out, check=True):
    """(out (B, Tmax, ld_out), lengths, counts) of the host build, or the finished process if it failed and check is False.
    P (B, Nmax, Dl) goes in as columns 0 .. Dl - 1 of rows of ld_p elements whose other columns hold NaN."""
    dd, exe = program
    B, Nmax, Dl = P.shape
    S = d.shape[2]
    wide = np.full((B, Nmax, ld_p), np.nan, dtype=P.dtype)
    wide[:, :, :Dl] = P
    arrays = [(n if n is not None else np.zeros(B)).astype(np.int32), wide, d]
    if kind == FM.COARSE_CODING:
        arrays.append(FM.coarse_coding_table())
    if scale is not None:
        arrays += [np.asarray(scale, dtype=np.float64), np.asarray(mins, dtype=np.float64)]
    head = [B, Nmax, S, Dl, ld_p, DT_CODE[P.dtype], DT_CODE[d.dtype], n is not None, min_frames, kind, scale is not None,
            DT_CODE[np.dtype(out_dtype)], ld_out, Tmax]
    with open(dd / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(dd / "in.bin"), str(dd / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dd / "out.bin", "rb").read()
    k = B * Tmax * ld_out * np.dtype(out_dtype).itemsize
    return (np.frombuffer(raw[:k], dtype=out_dtype).reshape(B, Tmax, ld_out), np.frombuffer(raw[k:k + 4 * B], dtype=np.int32),
            np.frombuffer(raw[k + 4 * B:], dtype=np.int64))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def draw_frames(rng, m, S, target):
    """(m, S) frames per state that add up to `target`: small counts, the first state, one in the middle and the last of 0
    frames (and a third of the others), the rest of the target in one state."""
    r = rng.randint(0, 4, size=(m, S))
    r[rng.rand(m, S) < 0.3] = 0
    flat = r.reshape(-1)
    flat[0] = flat[flat.size // 2] = flat[-1] = 0
    k = flat.size
    while flat.sum() > target:
        k -= 1
        flat[k] = 0
    if flat.size > 3:
        flat[1 + rng.randint(flat.size - 2)] += target - flat.sum()
    return r


def encode(rng, r, dtype):
    """Durations of `dtype` that give the frames r with min_frames 0: halves that round to even, quarters, negatives and NaN
    for 0."""
    r = np.asarray(r, dtype=np.int64)
    if np.dtype(dtype).kind == "i":
        d = r.copy()
        d[(r == 0) & (rng.rand(*r.shape) < 0.5)] = -3
        return d.astype(dtype)
    even = r % 2 == 0
    u = rng.rand(*r.shape)
    d = r + np.where(even, np.where(u < 0.4, 0.5, np.where((u < 0.8) & (r > 0), -0.5, 0.0)), np.where(u < 0.5, 0.25, -0.25))
    zero = (r == 0) & (u > 0.8)
    d[zero] = np.where(rng.rand(int(zero.sum())) < 0.5, np.nan, -3.0)
    d = d.astype(dtype)
    assert np.array_equal(FM.frames(d, 0), r)
    return d


def poison(d, P, n):
    """What is never read: phone rows at or past num_phones hold NaN, durations NaN or the type's largest integer."""
    Nmax = d.shape[1]
    for b in range(d.shape[0]):
        m = int(np.clip(n[b], 0, Nmax))
        P[b, m:] = np.nan
        d[b, m:] = np.iinfo(d.dtype).max if d.dtype.kind == "i" else np.nan


def make_case(seed, Nmax, S, Dl, targets, dur_dtype, num_phones):
    rng = np.random.RandomState(seed)
    B = len(targets)
    P = np.round(rng.randn(B, Nmax, Dl) * 4) / 4 + (rng.rand(B, Nmax, Dl) < 0.3) * rng.rand(B, Nmax, Dl)
    n = np.asarray(num_phones, dtype=np.int32)
    r = np.zeros((B, Nmax, S), dtype=np.int64)
    for b in range(B):
        m = int(np.clip(n[b], 0, Nmax))
        if m:
            r[b, :m] = draw_frames(rng, m, S, targets[b])
    d = encode(rng, r, dur_dtype)
    poison(d, P, n)
    return P, d, n


def check(program, P, d, n, kind, min_frames, affine, p_dtype, out_dtype, Tmax, seed=0, model_d=None):
    """One run against the model.  model_d: the durations the model gets instead of d (see test_saturated_running_counts)."""
    B, Nmax, Dl = P.shape
    W = Dl + FM.SIZES[kind]
    P = P.astype(p_dtype)
    rng = np.random.RandomState(seed + 77)
    scale, mins = (rng.rand(W) + 0.5, np.round(rng.randn(W) * 8) / 8) if affine else (None, None)
    ld_p, ld_out = Dl + 2, W + 3
    out, lengths, counts = host_expand(program, P, d, n, kind, min_frames, scale, mins, out_dtype, Tmax, ld_p, ld_out)
    want, want_len, _ = FM.frame_features_batch(P, d if model_d is None else model_d, n, FM.KINDS[kind], min_frames, scale, mins, Tmax,
                                                dtype=out_dtype, cc=FM.coarse_coding_table() if kind == FM.COARSE_CODING else None)
    m = np.full(B, Nmax) if n is None else np.clip(n, 0, Nmax)
    want_counts = np.array([FM.frames(d[b, :m[b]], min_frames).sum() for b in range(B)], dtype=np.int64)
    WORST["runs"] += 1
    ok = (np.array_equal(counts, want_counts) and np.array_equal(lengths, want_len)
          and np.array_equal(out[:, :, :W], want, equal_nan=True)          # live rows, and zeros behind them
          and not np.isnan(out).any()
          and (out[:, :, W:] == SENTINEL).all())                           # foreign columns are not touched
    WORST["unequal"] += not ok
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    assert np.array_equal(lengths, want_len), (lengths, want_len)
    assert (out[:, :, W:] == SENTINEL).all()
    assert not np.isnan(out).any()                                         # nothing past num_phones, no foreign column was read
    for b in range(B):
        assert not out[b, want_len[b]:, :W].any()                          # pad rows: zeros
    assert np.array_equal(out[:, :, :W], want)
    return out, lengths, counts


# (Nmax, S): 12, 256, 300 (two states per thread) and 301 (the last thread with work has one) states at full num_phones
STATE_SHAPES = ((4, 3), (32, 8), (60, 5), (43, 7))


@pytest.mark.parametrize("Tmax", [0, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3])
@pytest.mark.parametrize("min_frames", [0, 1])
def test_block_boundaries_and_num_phones(program, Tmax, min_frames):
    """num_phones 0, inside, equal to, above Nmax and negative; utterances shorter than, as long as and longer than Tmax
    (truncated); 255 (num_phones 51 of 60, S = 5) and 300 states."""
    Nmax, S = 60, 5
    n = [0, 51, Nmax, Nmax + 3, -2, 7]
    targets = [0, Tmax, Tmax + 9, max(Tmax - 1, 0), 0, min(Tmax, 5)]
    P, d, n = make_case(Tmax + min_frames, Nmax, S, 3, targets, DUR_DTYPES[(Tmax + min_frames) % 4], n)
    _, lengths, _ = check(program, P, d, n, FM.FULL, min_frames, False, np.float64, np.float64, Tmax)
    if min_frames == 0:
        assert list(lengths) == [0, Tmax, Tmax, max(Tmax - 1, 0), 0, min(Tmax, 5)]


@pytest.mark.parametrize("kind", range(8))
@pytest.mark.parametrize("Dl", [0, 1, 70])
def test_every_kind_and_width(program, kind, Dl):
    """All eight kinds at Dl 0, 1 and 70 (a second pass over the columns), with and without the fused scaling; the dtypes and
    the state counts of STATE_SHAPES take turns."""
    i = kind * 3 + (Dl % 3)
    Nmax, S = STATE_SHAPES[i % 4]
    T = BLOCK + 7
    for affine in (False, True):
        dur = DUR_DTYPES[(i + affine) % 4]
        P, d, n = make_case(i, Nmax, S, Dl, [T, 20, T + 30], dur, [Nmax, Nmax - 1, Nmax])
        check(program, P, d, n, kind, i % 2 if kind else 0, affine, (np.float32, np.float64)[i % 2], (np.float64, np.float32)[(i // 2) % 2], T,
              seed=i)
    # no num_phones: Nmax each
    P, d, _ = make_case(i, Nmax, S, Dl, [T, 9], DUR_DTYPES[i % 4], [Nmax, Nmax])
    check(program, P, d, None, kind, 0, True, np.float64, np.float32, T)


@pytest.mark.parametrize("dur", DUR_DTYPES)
def test_every_dtype(program, dur):
    for p_dtype in (np.float32, np.float64):
        for out_dtype in (np.float32, np.float64):
            P, d, n = make_case(5, 32, 8, 2, [BLOCK + 1, 3], dur, [32, 9])
            check(program, P, d, n, FM.FULL, 1, True, p_dtype, out_dtype, BLOCK + 1)


@pytest.mark.parametrize("dur", [np.int32, np.int64, np.float64])
def test_saturated_running_counts(program, dur):
    """Durations near 2^31: the running count passes 2^31 - 1 at the second big state and stays saturated; the total is far
    beyond Tmax.  For the kinds `None` and `state_only` a row depends only on which state its frame falls in, so the model is
    given the durations clipped to Tmax: the first Tmax rows are the same.  The counts are compared with the unclipped sum."""
    Tmax, Nmax, S = 2 * BLOCK + 3, 60, 5
    rng = np.random.RandomState(3)
    big = 2 ** 31 - 1
    r = rng.randint(0, 3, size=(2, Nmax, S)).astype(np.int64)
    r[0, 10, 2] = big - 4
    r[0, 11, 0] = big
    r[0, 40, 4] = big
    r[1, 0, 0] = 0
    r[1, 0, 1] = big
    r[1, 30, 0] = 2 ** 30
    d = r.astype(dur)
    if dur != np.int32:
        d[0, 50, 1] = 2.0 ** 40                                          # counts as 2^31 - 1
    assert FM.frames(d, 0).sum() > 3 * big
    P = np.round(rng.randn(2, Nmax, 2) * 4) / 4
    n = np.array([Nmax, 31], dtype=np.int32)
    poison(d, P, n)
    clipped = np.minimum(FM.frames(d, 0), Tmax).astype(np.int64)
    for kind in (FM.NONE, FM.STATE_ONLY):
        _, lengths, counts = check(program, P, d, n, kind, 0, True, np.float64, np.float64, Tmax, model_d=clipped)
        assert list(lengths) == [Tmax, Tmax] and counts[0] > 3 * big


def test_worst_figure(program):
    print("kernel text against the model: %d runs, %d not bit-equal (bound: bit equality, worst error / bound = %d)"
          % (WORST["runs"], WORST["unequal"], WORST["unequal"]))
    assert WORST["unequal"] == 0


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit, n, affine):
    """The outcome of one run on the text with `edit`: "sanitizer", "mismatch" or "passed"."""
    prog = build(tmp_path, edit)
    Nmax, S, Dl, T = 32, 8, 2, BLOCK + 1
    P, d, n = make_case(5, Nmax, S, Dl, [T, 3], np.int32, n)
    W = Dl + 9
    scale, mins = (np.ones(W), np.zeros(W)) if affine else (None, None)
    got = host_expand(prog, P, d, n, FM.FULL, 0, scale, mins, np.float64, T, Dl + 2, W + 3, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return "sanitizer"
    out, lengths, counts = got
    want, want_len, want_counts = FM.frame_features_batch(P, d, n, "full", 0, scale, mins, T)
    same = (np.array_equal(out[:, :, :W], want) and (out[:, :, W:] == SENTINEL).all() and np.array_equal(lengths, want_len)
            and np.array_equal(counts, want_counts))
    return "passed" if same else "mismatch"


def test_planted_read_one_phone_past_num_phones(tmp_path):
    """num_phones + 1 phones: inside Nmax the extra durations are INT32_MAX (the counts show it), at Nmax the reads leave the
    durations' heap block and the running counts the LDS block."""
    edit = ("return n < 0 ? 0 : (n > Nmax ? Nmax : n);", "return n < 0 ? 0 : (n > Nmax ? Nmax : n) + 1;")
    assert planted(tmp_path / "a", edit, [31, 9], False) == "mismatch"
    assert planted(tmp_path / "b", edit, [9, 32], False) == "sanitizer"


def test_planted_lds_one_running_count_short(tmp_path):
    """The LDS block without its last int32: the scan's store of the last state's running count leaves it."""
    edit = ("(size_t)kFxOffCum + (size_t)a.Nmax * a.S * 4;", "(size_t)kFxOffCum + ((size_t)a.Nmax * a.S - 1) * 4;")
    assert planted(tmp_path / "a", edit, [32, 9], False) == "sanitizer"


def test_planted_store_one_column_past_the_width(tmp_path):
    """Column Dl + F is stored: the sentinel of the first foreign column is gone (with the scaling, scale_[Dl + F] is read)."""
    edit = ("for (int c = lane; c < W; c += 64) {", "for (int c = lane; c <= W; c += 64) {")
    assert planted(tmp_path / "a", edit, [32, 9], False) == "mismatch"
    assert planted(tmp_path / "b", edit, [32, 9], True) == "sanitizer"
