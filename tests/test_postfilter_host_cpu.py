"""The text of csrc/postfilter.hip run on the CPU (-m "not gpu"): compiled for the host against the shim tests/gmm_host/common.h
plus tests/postfilter_host/extras.h into a stand-alone program under the address and undefined-behaviour sanitizers, run as a
child process, and compared with tools/postfilter_model.py within the BOUND of tests/test_postfilter_gpu.py.  This checks the
MFMA tiles over the B * Tmax axis with a partial last tile, the masking of pad frames (they hold NaN), the staging in LDS and the
typed stores.  The kernel has static LDS only (no ``extern __shared__``: the marker count is 0), which the address sanitizer
guards as globals.  Every array is an exact-size heap block, the table G included; the input is a column slice of wider rows
whose other columns hold NaN; the output is pre-filled with -7.  Nothing is loaded into Python under a sanitizer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import postfilter_model as PM  # noqa: E402

F32, F64 = np.float32, np.float64
BOUND = {F64: 1e-11, F32: 2e-6}
SENTINEL = -7
TILE = 64
WORST = {F32: 0.0, F64: 0.0}


def test_the_bound_is_the_gpu_tests():
    text = open(os.path.join(ROOT, "tests", "test_postfilter_gpu.py")).read()
    line = re.search(r"^BOUND = (\{.*\})$", text, re.M).group(1)
    assert eval(line, {"F32": F32, "F64": F64}) == BOUND
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    assert int(re.search(r"^#define\s+MLPG_HIP_POSTFILTER_FRAME_TILE\s+(\d+)", header, re.M).group(1)) == TILE


def build(d, edit=None):
    """The host program of the kernel text in directory d; `edit` (old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    csrc = os.path.join(ROOT, "nnmnkwii_amd", "csrc")
    src = open(os.path.join(csrc, "postfilter.hip")).read()
    assert src.count("extern __shared__") == 0
    if edit is not None:
        assert src.count(edit[0]) == 1, edit[0]
        src = src.replace(edit[0], edit[1])
    os.makedirs(d / "csrc" / "x")
    (d / "csrc" / "x" / "postfilter_host.inc").write_text(src)
    (d / "csrc" / "x" / "postfilter_table.h").write_text(open(os.path.join(csrc, "postfilter_table.h")).read())
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/postfilter_host", "extras.h"), ("tests/postfilter_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "postfilter_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-DMLPG_HIP_POSTFILTER_FRAME_TILE=%d" % TILE, "-I", str(d),
                        str(d / "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("postfilter_host"))


def mgc_like(rng, T, D):
    x = rng.randn(T, D) / (1.0 + np.arange(D))
    x[:, 0] += rng.uniform(-8.0, 2.0, T)
    return x


def host_filter(program, wide, D, lengths, alpha, order, fftlen, weight, ld_out=None, in_place=False, check=True):
    """out (B, Tmax, ld_out) of the host build; wide (B, Tmax, ld_in) holds the input in its columns 0 .. D - 1."""
    d, exe = program
    B, Tmax, ld_in = wide.shape
    ld_out = ld_in if in_place else ld_out
    L = np.zeros(B, dtype=np.int32) if lengths is None else np.asarray(lengths, dtype=np.int32)
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([B, Tmax, D, ld_in, ld_out, wide.dtype == F64, lengths is not None, in_place, fftlen, order], dtype=np.int64).tobytes())
        f.write(np.array([alpha], dtype=F64).tobytes())
        for a in (L, wide, np.asarray(weight, dtype=F64)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    return np.frombuffer(open(d / "out.bin", "rb").read(), dtype=wide.dtype).reshape(B, Tmax, ld_out)


def case(seed, B, Tmax, D, lengths, dt):
    """(clean (B, Tmax, D) of dt, wide (B, Tmax, D + 2): the foreign columns and the rows at or past lengths[b] hold NaN)."""
    rng = np.random.RandomState(seed)
    clean = np.stack([mgc_like(rng, Tmax, D) for _ in range(B)]).astype(dt).reshape(B, Tmax, D)
    wide = np.full((B, Tmax, D + 2), np.nan, dtype=dt)
    for b in range(B):
        n = Tmax if lengths is None else min(max(lengths[b], 0), Tmax)
        wide[b, :n, :D] = clean[b, :n]
    return clean, wide


def verdict(got, wide, D, ref, lengths, dt, in_place):
    """None if the output is right, else what is wrong with it."""
    B, Tmax = ref.shape[:2]
    if in_place:
        if not np.isnan(got[:, :, D:]).all():
            return "a foreign column of the buffer was written"
    elif not (got[:, :, D:] == SENTINEL).all():
        return "a foreign column of out was written"
    live = got[:, :, :D]
    for b in range(B):
        n = Tmax if lengths is None else min(max(lengths[b], 0), Tmax)
        pad = live[b, n:]
        if pad.any() or np.isnan(pad).any() or np.signbit(pad).any():
            return "pad rows are not exact zeros"
    if not np.isfinite(live).all():
        return "not finite"
    if not np.abs(ref).max() > 0:
        return None
    e = float(np.abs(live.astype(F64) - ref).max() / np.abs(ref).max())
    WORST[dt] = max(WORST[dt], e / BOUND[dt])
    return None if e <= BOUND[dt] else "error %.3e above the bound %.1e" % (e, BOUND[dt])


# (B, Tmax, lengths): B * Tmax one below, at and one above the frame tile; lengths 0, 1 and Tmax
BATCHES = ((3, 21, [21, 1, 0]), (2, 32, [0, 32]), (5, 13, [13, 0, 1, 5, 13]))
ALPHAS = (0.58, 0.35, 0.77, -0.42, 0.0)


@pytest.mark.parametrize("D,order,fftlen", [(1, 15, 32), (2, 31, 32), (3, 2, 32), (25, 24, 32), (1, 511, 1024), (3, 511, 1024), (25, 511, 1024),
                                            (64, 63, 1024)])
@pytest.mark.parametrize("dt", [F32, F64])
def test_kernel_text_on_the_host(program, D, order, fftlen, dt):
    alpha = ALPHAS[(D + fftlen // 32) % len(ALPHAS)]
    for i, (B, Tmax, lengths) in enumerate(BATCHES if fftlen == 32 or D == 3 else BATCHES[2:]):
        clean, wide = case(D * 10 + i, B, Tmax, D, lengths, dt)
        w = PM.default_weight(D) if i != 1 else 1.0 + np.arange(D) / D
        ref = PM.post_filter_batch(clean.astype(F64), alpha, order, fftlen, weight=w, lengths=lengths)
        got = host_filter(program, wide, D, lengths, alpha, order, fftlen, w, ld_out=D + 3)
        assert verdict(got, wide, D, ref, lengths, dt, False) is None
        again = host_filter(program, wide, D, lengths, alpha, order, fftlen, w, in_place=True)
        assert verdict(again, wide, D, ref, lengths, dt, True) is None
        assert again[:, :, :D].tobytes() == np.ascontiguousarray(got[:, :, :D]).tobytes()      # in place: the same bits
    print("kernel text against the model, D=%d fftlen=%d %s: worst error / bound %.3g" % (D, fftlen, dt.__name__, WORST[dt]))


def test_no_lengths_and_two_whole_tiles(program):
    """lengths = NULL: every frame is live; two full tiles and a third of one frame."""
    B, Tmax, D = 3, 43, 5
    clean, wide = case(1, B, Tmax, D, None, F64)
    ref = PM.post_filter_batch(clean, 0.42, 31, 64)
    got = host_filter(program, wide, D, None, 0.42, 31, 64, PM.default_weight(D), ld_out=D)
    assert verdict(got, wide, D, ref, None, F64, False) is None
    print("worst error / bound: float32 %.3g, float64 %.3g" % (WORST[F32], WORST[F64]))


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit):
    prog = build(tmp_path, edit)
    B, Tmax, lengths = BATCHES[2]
    clean, wide = case(4, B, Tmax, 3, lengths, F64)
    ref = PM.post_filter_batch(clean, 0.35, 15, 32, lengths=lengths)
    got = host_filter(prog, wide, 3, lengths, 0.35, 15, 32, PM.default_weight(3), ld_out=6, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return "sanitizer"
    return verdict(got, wide, 3, ref, lengths, F64, False)


def test_planted_read_one_row_past_the_length(tmp_path):
    """Frame lengths[b] counts as live: its NaN comes out where a zero belongs."""
    assert planted(tmp_path / "a", ("mine = t < len;", "mine = t <= len;")) == "pad rows are not exact zeros"


def test_planted_lds_one_element_short(tmp_path):
    """The staged frames without their last element: the staging loop's last store leaves the array."""
    assert planted(tmp_path / "a", ("__shared__ double xs[kPfFrames * kPfLd];", "__shared__ double xs[kPfFrames * kPfLd - 1];")) == "sanitizer"


def test_planted_read_one_column_past_d(tmp_path):
    """Column D of the input is staged (NaN in the wider row) and meets a zero of the table: NaN in every live row."""
    assert planted(tmp_path / "a", ("xs[i] = (c < D && vld[r])", "xs[i] = (c <= D && vld[r])")) == "not finite"
