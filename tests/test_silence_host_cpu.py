"""The text of csrc/frame_keep.hip run on the CPU (-m "not gpu"): compiled for the host against the shim tests/gmm_host/common.h
plus tests/silence_host/extras.h into a stand-alone program (its own main) under the address and undefined-behaviour sanitizers,
run as a child process, and compared with tools/silence_model.py bit for bit.  This checks the index logic: the two int64 scans,
the saturated running counts in LDS (an exact-size heap block), the binary search on the kept counts, the source frame of a
row, the rows behind K_b.  Every array is an exact-size heap block; the phone matrix is a column slice of wider rows whose other
columns hold NaN; phone rows at or past num_phones[b] hold NaN, durations there NaN or INT32_MAX / INT64_MAX (one such read
saturates the sums) and flags there 1; source rows at or past len_src[b] hold NaN; the outputs are pre-filled with -7 and their
foreign columns must still hold it.  Nothing is loaded into Python under a sanitizer.

The file also ties the device functions that frame_keep.hip restates to frame_expand.hip's: with no phone flagged the host build's
output equals the host build of frame_expand.hip on the same inputs.

Two planted defects show that the harness bites: see test_planted_*."""
import os
import subprocess

import numpy as np
import pytest

import silence_cases as SC
from silence_cases import FM, SM
from test_frontend_host_cpu import build as build_frontend_host, host_expand

ROOT = SC.ROOT
BLOCK = SC.BLOCK
DT_CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}
MARKER = "extern __shared__ double sk_lds[];"
SENTINEL = -7


def build(d, edit=None):
    """The host program of the kernel text in directory d; `edit` (old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "frame_keep.hip")).read()
    assert src.count(MARKER) == 1
    src = src.replace(MARKER, "#define sk_lds g_dyn_lds")
    if edit is not None:
        assert src.count(edit[0]) == 1, edit[0]
        src = src.replace(edit[0], edit[1])
    os.makedirs(d / "csrc" / "x")
    os.makedirs(d / "include")
    (d / "csrc" / "x" / "frame_keep_host.inc").write_text(src)
    for name in ("nnmnkwii_silence.h", "nnmnkwii_frontend.h"):
        (d / "include" / name).write_text(open(os.path.join(ROOT, "include", name)).read())
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/silence_host", "extras.h"), ("tests/silence_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "silence_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("silence_host"))


@pytest.fixture(scope="module")
def frontend_program(tmp_path_factory):
    return build_frontend_host(tmp_path_factory.mktemp("frontend_host_for_silence"))


def host_run(program, P, d, sil, n, kind, min_frames, scale, mins, out_dtype, Tcap, ld_p, ld_out, gather=None, check=True):
    """(out (B, Tcap, ld_out), lengths, counts (B, 2)[, gout (B, Tcap_g, ld_gout), glengths]) of the host build, or the finished
    process if it failed and check is False.  gather: dict(Y (B, Tmax, D), len (B) or None, ld_src, ld_out, Tcap)."""
    dd, exe = program
    B, Nmax, Dl = P.shape
    S = d.shape[2]
    wide = np.full((B, Nmax, ld_p), np.nan, dtype=P.dtype)
    wide[:, :, :Dl] = P
    arrays = [(n if n is not None else np.zeros(B)).astype(np.int32), sil.astype(np.uint8), wide, d]
    if kind == FM.COARSE_CODING:
        arrays.append(FM.coarse_coding_table())
    if scale is not None:
        arrays += [np.asarray(scale, dtype=np.float64), np.asarray(mins, dtype=np.float64)]
    head = [B, Nmax, S, Dl, ld_p, DT_CODE[P.dtype], DT_CODE[d.dtype], n is not None, min_frames, kind, scale is not None,
            DT_CODE[np.dtype(out_dtype)], ld_out, Tcap] + [0] * 8
    if gather is not None:
        Y = gather["Y"]
        Tmax, D = Y.shape[1:]
        src = np.full((B, Tmax, gather["ld_src"]), np.nan, dtype=Y.dtype)
        src[:, :, :D] = Y
        head[14:] = [1, Tmax, D, gather["ld_src"], DT_CODE[Y.dtype], gather["len"] is not None, gather["ld_out"], gather["Tcap"]]
        arrays += [(gather["len"] if gather["len"] is not None else np.zeros(B)).astype(np.int32), src]
    with open(dd / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(dd / "in.bin"), str(dd / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dd / "out.bin", "rb").read()
    isz = np.dtype(out_dtype).itemsize
    k = B * Tcap * ld_out * isz
    res = [np.frombuffer(raw[:k], dtype=out_dtype).reshape(B, Tcap, ld_out), np.frombuffer(raw[k:k + 4 * B], dtype=np.int32),
           np.frombuffer(raw[k + 4 * B:k + 20 * B], dtype=np.int64).reshape(B, 2)]
    if gather is not None:
        k0 = k + 20 * B
        k1 = k0 + B * gather["Tcap"] * gather["ld_out"] * isz
        res += [np.frombuffer(raw[k0:k1], dtype=out_dtype).reshape(B, gather["Tcap"], gather["ld_out"]),
                np.frombuffer(raw[k1:k1 + 4 * B], dtype=np.int32)]
    return res


def check(program, P, d, sil, n, kind, min_frames, with_affine, p_dtype, out_dtype, Tcap, seed=0, gather=None):
    """One run against the model: counts, the kept-frame expansion and (gather: dict(Y, len, Tcap)) the row gather."""
    B, Nmax, Dl = P.shape
    W = Dl + FM.SIZES[kind]
    P = P.astype(p_dtype)
    scale, mins = SC.affine(seed, W) if with_affine else (None, None)
    g = None if gather is None else dict(gather, ld_src=gather["Y"].shape[2] + 2, ld_out=gather["Y"].shape[2] + 3)
    res = host_run(program, P, d, sil, n, kind, min_frames, scale, mins, out_dtype, Tcap, Dl + 2, W + 3, g)
    out, lengths, counts = res[:3]
    cc = FM.coarse_coding_table() if kind == FM.COARSE_CODING else None
    want, want_len, _ = SM.kept_frame_features_batch(P, d, sil, n, FM.KINDS[kind], min_frames, scale, mins, Tcap, dtype=out_dtype, cc=cc)
    assert np.array_equal(counts, SM.frame_counts(d, sil, n, min_frames)), (counts, SM.frame_counts(d, sil, n, min_frames))
    assert np.array_equal(lengths, want_len), (lengths, want_len)
    assert (out[:, :, W:] == SENTINEL).all()                                   # foreign columns are not touched
    assert not np.isnan(out).any()                                             # nothing past num_phones, no foreign column was read
    assert SC.same_bits(out[:, :, :W], want)                                   # kept rows, and zeros behind them
    if gather is not None:
        gout, glen = res[3:]
        D = gather["Y"].shape[2]
        gwant, gwant_len, _ = SM.remove_silence_frames_batch(gather["Y"], d, sil, gather["len"], n, min_frames, gather["Tcap"], out_dtype)
        assert np.array_equal(glen, gwant_len), (glen, gwant_len)
        assert (gout[:, :, D:] == SENTINEL).all() and not np.isnan(gout).any()      # no row at or past len_src was read
        assert SC.same_bits(gout[:, :, :D], gwant)
    return res


def gather_case(seed, plans, Tmax, D, lens, Tcap, dtype=np.float64):
    lens = None if lens is None else np.asarray(lens, dtype=np.int32)
    live = np.full(len(plans), Tmax) if lens is None else np.clip(lens, 0, Tmax)
    return dict(Y=SC.source(seed, len(plans), Tmax, D, live, dtype), len=lens, Tcap=Tcap)


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("kind", range(8))
def test_every_kind_against_the_model(program, kind, S):
    """Both batches of plans (tests/silence_cases.py) at every kind; the duration, phone and output dtypes and the fused scaling
    take turns.  The gather runs beside it: sources shorter than, as long as and longer than the labels' frames."""
    i = kind * 2 + (S == 5)
    for j, plans in enumerate((SC.PLANS_A, SC.PLANS_B)):
        P, d, sil, n, _ = SC.make_batch(i + 40 * j, plans, S, 3, SC.DUR_DTYPES[(i + j) % 4])
        T = SC.all_counts(plans)
        Tmax = int(T.max()) + 70
        lens = [[0, T[1] - 1, T[2], T[3] + 70, T[4] - 7, T[5] + 1], [5, T[1], T[2] - 1, T[3] - 100, T[4] + 70, 0]][j]
        g = gather_case(i, plans, Tmax, (1, 65)[(i + j) % 2], lens, Tmax, (np.float32, np.float64)[i % 2])
        check(program, P, d, sil, n, kind, 0, bool((i + j) % 2), (np.float32, np.float64)[(i // 2) % 2], (np.float64, np.float32)[(i + j) % 2],
              int(SC.kept_counts(plans).max()) + 3, seed=i, gather=g)


@pytest.mark.parametrize("Tcap", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3])
def test_capacity_below_at_and_above_the_kept_frames(program, Tcap):
    P, d, sil, n, _ = SC.make_batch(Tcap, SC.PLANS_A, 5, 2, SC.DUR_DTYPES[Tcap % 4])
    g = gather_case(Tcap, SC.PLANS_A, 150, 2, [150, 3, 73, 76, 150, 131], Tcap)
    _, lengths, counts, _, glen = check(program, P, d, sil, n, FM.FULL, 0, False, np.float64, np.float64, Tcap, gather=g)
    assert list(counts[:, 0]) == list(SC.K_A) and list(lengths) == [min(k, Tcap) for k in SC.K_A]
    assert list(glen) == [min(k, Tcap) for k in (138, 0, 63, 64, 65 + 77, 131)]


def test_no_num_phones_no_lengths_and_min_frames(program):
    """NULL num_phones and len_src (Nmax and Tmax each), and min_frames 1: every state has at least one frame."""
    plans = [[(3, 0), (4, 1), (2, 0)], [(1, 1), (1, 0), (6, 1)]]
    for S in (1, 5):
        P, d, sil, n, _ = SC.make_batch(S, plans, S, 70, np.float64, spare=0)
        g = gather_case(S, plans, 40, 3, None, 40, np.float32)
        check(program, P, d, sil, None, FM.FULL, 1, True, np.float64, np.float32, 40, gather=g)


@pytest.mark.parametrize("dur", [np.int32, np.int64, np.float64])
def test_saturated_running_counts(program, dur):
    """Durations near 2^31 in flagged AND kept phones: both running counts pass 2^31 - 1 and stay saturated.  For the kind
    `state_only` a row depends only on which state its frame falls in, so the model is given the durations clipped to what the
    output can show; the counts are compared with the unclipped sums."""
    Tcap, Nmax, S = 2 * BLOCK + 3, 12, 5
    big = 2 ** 31 - 1
    rng = np.random.RandomState(3)
    r = rng.randint(0, 3, size=(2, Nmax, S)).astype(np.int64)
    sil = np.zeros((2, Nmax), dtype=np.uint8)
    sil[0, 2] = sil[0, 5] = sil[1, 0] = 1
    r[0, 2, 1] = big                       # flagged: the frame count saturates here, the kept count does not
    r[0, 6, 2] = big - 4                   # kept
    r[0, 7, 0] = big
    r[1, 0, 3] = big
    r[1, 4, 4] = 2 ** 30
    d = r.astype(dur)
    P = np.round(rng.randn(2, Nmax, 2) * 4) / 4
    n = np.array([Nmax, 9], dtype=np.int32)
    P[1, 9:] = np.nan
    d[1, 9:] = np.iinfo(d.dtype).max if d.dtype.kind == "i" else np.nan
    clipped = np.minimum(r, Tcap)
    res = host_run(program, P, d, sil, n, FM.STATE_ONLY, 0, None, None, np.float64, Tcap, 4, 6,
                   dict(Y=SC.source(1, 2, 300, 2, [300, 300]), len=None, ld_src=2, ld_out=2, Tcap=300))
    out, lengths, counts, gout, glen = res
    want, want_len, _ = SM.kept_frame_features_batch(P, clipped, sil, n, "state_only", 0, Tcap=Tcap)
    assert np.array_equal(counts, SM.frame_counts(d, sil, n, 0)) and counts[0, 0] > 2 * big and counts[0, 1] > 3 * big
    assert list(lengths) == [Tcap, Tcap] and SC.same_bits(out[:, :, :3], want)
    # the gather: the first flagged frames are dropped, the source ends long before the labels do
    Y = SC.source(1, 2, 300, 2, [300, 300])
    gwant, gwant_len, _ = SM.remove_silence_frames_batch(Y, np.minimum(r, 400), sil, None, n, 0, 300)
    assert np.array_equal(glen, gwant_len) and SC.same_bits(gout, gwant)


def test_restated_device_functions_are_frame_expand_s(program, frontend_program):
    """With no phone flagged the host build of frame_keep.hip gives, bit for bit, what the host build of frame_expand.hip gives:
    the duration rule (every dtype, halves, NaN, negatives, min_frames) and the sub-phone columns of all eight kinds."""
    for kind in range(8):
        for S in (1, 5):
            i = kind * 2 + (S == 5)
            dur = SC.DUR_DTYPES[i % 4]
            P, d, sil, n, _ = SC.make_batch(i, SC.PLANS_A, S, 3, dur)
            sil[:] = 0
            W = 3 + FM.SIZES[kind]
            scale, mins = SC.affine(i, W)
            for mf in (0, 1):
                Tcap = 140
                mine = host_run(program, P, d, sil, n, kind, mf, scale, mins, np.float32, Tcap, 5, W + 3)
                theirs = host_expand(frontend_program, P, d, n, kind, mf, scale, mins, np.float32, Tcap, 5, W + 3)
                assert SC.same_bits(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
                assert np.array_equal(mine[2][:, 0], theirs[2]) and np.array_equal(mine[2][:, 1], theirs[2])


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit, lens, Tmax):
    """The outcome of one run on the text with `edit`: "sanitizer", "mismatch" or "passed"."""
    prog = build(tmp_path, edit)
    P, d, sil, n, _ = SC.make_batch(5, SC.PLANS_A, 5, 2, np.int32)
    W = 2 + 9
    g = gather_case(5, SC.PLANS_A, Tmax, 2, lens, Tmax + 5)
    g.update(ld_src=2, ld_out=2)
    got = host_run(prog, P, d, sil, n, FM.FULL, 0, None, None, np.float64, 140, 4, W + 3, g, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return "sanitizer"
    out, lengths, counts, gout, glen = got
    want, want_len, _ = SM.kept_frame_features_batch(P, d, sil, n, "full", 0, Tcap=140)
    gwant, gwant_len, _ = SM.remove_silence_frames_batch(g["Y"], d, sil, g["len"], n, 0, Tmax + 5)
    same = (SC.same_bits(out[:, :, :W], want) and np.array_equal(lengths, want_len) and SC.same_bits(gout, gwant)
            and np.array_equal(glen, gwant_len))
    return "passed" if same else "mismatch"


def test_planted_off_by_one_in_the_kept_count_search(tmp_path):
    """`>=` for `>`: row r lands in the state whose kept count REACHES r -- the last frame of a state is taken from the next."""
    edit = ("    if (cum[mid] > v)\n", "    if (cum[mid] >= v)\n")
    assert planted(tmp_path / "a", edit, [12, 8, 73, 76, 73, 131], 131) in ("mismatch", "sanitizer")
    assert planted(tmp_path / "ok", None, [12, 8, 73, 76, 73, 131], 131) == "passed"


def test_planted_gather_reads_row_len_src(tmp_path):
    """`<=` for `<`: the row at len_src is read -- NaN inside the source, and past the heap block behind the last utterance."""
    edit = ("rowsrc[tid] = t < (long long)len ? (int)t : -1;", "rowsrc[tid] = t <= (long long)len ? (int)t : -1;")
    assert planted(tmp_path / "a", edit, [12, 8, 73, 76, 73, 100], 131) == "mismatch"
    assert planted(tmp_path / "b", edit, [12, 8, 73, 76, 73, 131], 131) == "sanitizer"
