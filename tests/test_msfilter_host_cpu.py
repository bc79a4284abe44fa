"""The text of csrc/modspec_filter.hip with csrc/modspec_fft.h run on the CPU (-m "not gpu"): compiled for the host against the
shim tests/gmm_host/common.h plus tests/msfilter_host/extras.h into a stand-alone program under the address and
undefined-behaviour sanitizers, run as a child process, and compared with tools/msfilter_model.py within the BOUND of
tests/test_msfilter_gpu.py.  The dynamic LDS -- the padded data block and the twiddle tables behind it -- is an exact-size heap
block, so the largest padded index and the last twiddle are checked against it; every array is an exact-size heap block; x is a
column slice of wider rows whose other columns hold NaN, as do its rows at or past lengths[b]; out is pre-filled with -7.  A
second build sets the grid's workgroup limit to 4, so that three utterances of two column pairs take two launches and the slice
loop's offsets are under the sanitizers too.  A workgroup is 1024 threads: the batches are small.  Nothing is loaded into Python
under a sanitizer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import modspec_batch64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import msfilter_model as MM  # noqa: E402

F32, F64 = np.float32, np.float64
BOUND = {F64: 1e-10, F32: 5e-6}
SENTINEL = -7
MARKER = "extern __shared__ __align__(16) unsigned char smem[];"
WORST = {F32: 0.0, F64: 0.0}


def test_the_bound_is_the_gpu_tests():
    text = open(os.path.join(ROOT, "tests", "test_msfilter_gpu.py")).read()
    assert eval(re.search(r"^BOUND = (\{.*\})$", text, re.M).group(1), {"F32": F32, "F64": F64}) == BOUND


def build(d, edit=None, defs=()):
    """The host program of the kernel text in directory d; `edit` (file, old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    csrc = os.path.join(ROOT, "nnmnkwii_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("modspec_filter.hip", "modspec_fft.h")}
    assert text["modspec_filter.hip"].count(MARKER) == 1 and text["modspec_fft.h"].count("extern __shared__") == 0
    text["modspec_filter.hip"] = text["modspec_filter.hip"].replace(MARKER, "unsigned char *smem = (unsigned char *)g_dyn_lds;")
    if edit is not None:
        assert text[edit[0]].count(edit[1]) == 1, edit[1]
        text[edit[0]] = text[edit[0]].replace(edit[1], edit[2])
    os.makedirs(d / "csrc" / "x")
    (d / "csrc" / "x" / "modspec_filter_host.inc").write_text(text["modspec_filter.hip"])
    (d / "csrc" / "x" / "modspec_fft.h").write_text(text["modspec_fft.h"])
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/msfilter_host", "extras.h"), ("tests/msfilter_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "msfilter_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-Wno-unused-function", *defs, "-I", str(d), str(d / "main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("msfilter_host"))


@pytest.fixture(scope="module")
def sliced(tmp_path_factory):
    return build(tmp_path_factory.mktemp("msfilter_sliced"), defs=("-DSHIM_MAX_WORKGROUPS=4",))


def host_filter(program, wide, D, lengths, n, A, C, limit_bin, log_domain, ortho, ld_out=None, in_place=False, check=True):
    """out (B, T, ld_out) of the host build; wide (B, T, ld_x) holds x in its columns 0 .. D - 1."""
    d, exe = program
    B, T, ld_x = wide.shape
    ld_out = ld_x if in_place else ld_out
    L = np.zeros(B, dtype=np.int32) if lengths is None else np.asarray(lengths, dtype=np.int32)
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([B, T, D, n, ld_x, ld_out, wide.dtype == F64, lengths is not None, A is not None, limit_bin, log_domain, ortho,
                          in_place], dtype=np.int64).tobytes())
        for a in (L, wide) + ((A, C) if A is not None else ()):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    return np.frombuffer(open(d / "out.bin", "rb").read(), dtype=wide.dtype).reshape(B, T, ld_out)


def tables(rng, nb, D):
    """The tables of tests/test_msfilter_gpu.py: A in [0.43, 2.7], gains exp(C / 2) within [1/16, 16]."""
    return rng.uniform(0.43, 2.7, (nb, D)), rng.uniform(-2 * np.log(16.0), 2 * np.log(16.0), (nb, D))


def case(rng, B, T, D, lengths, n, dt):
    """x (B, T, D) of dt with NaN from each length on, and the same as columns 0 .. D - 1 of rows of D + 2 (NaN elsewhere).  The
    GPU test's condition on the inputs holds: every |S| is at least 1e-6 of its column's largest."""
    x = R.make_batch(rng, B, T, D, lengths).astype(dt)
    live = MM.live_frames(lengths, B, T)
    for b in range(B):
        if live[b]:
            mag = np.abs(np.fft.rfft(x[b, :live[b]].astype(F64), n=n, axis=0))
            assert (mag.min(axis=0) / mag.max(axis=0)).min() >= 1e-6
    wide = np.full((B, T, D + 2), np.nan, dtype=dt)
    wide[:, :, :D] = x
    return x, wide, live


def verdict(got, D, ref, live, dt, in_place):
    """None if the output is right, else what is wrong with it."""
    if in_place:
        if not np.isnan(got[:, :, D:]).all():
            return "a foreign column of the buffer was written"
    elif not (got[:, :, D:] == SENTINEL).all():
        return "a foreign column of out was written"
    y = got[:, :, :D]
    for b in range(len(live)):
        pad = y[b, live[b]:]
        if pad.any() or np.isnan(pad).any() or np.signbit(pad).any():
            return "pad rows are not exact zeros"
    if not np.isfinite(y).all():
        return "not finite"
    if not np.abs(ref).max():
        return "not zero" if y.any() else None                                 # every bin removed outside the log domain
    e = float(np.abs(y.astype(F64) - ref).max() / np.abs(ref).max())
    WORST[dt] = max(WORST[dt], e / BOUND[dt])
    return None if e <= BOUND[dt] else "error %.3e above the bound %.1e" % (e, BOUND[dt])


def modes(nb):
    """(tables?, limit_bin, log_domain): tables given and absent, limit_bin 0, inside and n/2 + 1, both domains."""
    return [(tabs, lb, dom) for tabs in (True, False) for dom in (True, False) for lb in (0, (nb + 1) // 2, nb)]


# n: the smallest the FFT route takes, 64 and 4096; T == n and T < n
@pytest.mark.parametrize("n,T", [(2, 2), (2, 1), (64, 64), (64, 61), (4096, 4096), (4096, 4093)])
def test_kernel_text_on_the_host(program, n, T):
    """D 1, 2 and 3; live T, 1 and 0; the twelve modes in turn (four per D); the dtype, the normalisation and in place
    alternate (a launch is 1024 threads on a barrier: one run per mode and D)."""
    nb = n // 2 + 1
    rng = np.random.RandomState(n + T)
    lengths = [T, 1, 0]
    every = modes(nb)
    for D in (1, 2, 3):
        A, C = tables(rng, nb, D)
        for i, (tabs, lb, dom) in enumerate(every[4 * (D - 1):4 * D]):
            dt = (F32, F64)[(i + D + T) % 2]
            x, wide, live = case(rng, 3, T, D, lengths, n, dt)
            norm = "ortho" if (i // 2 + D) % 2 else None
            a, c = (A, C) if tabs else (None, None)
            ref = MM.filter_batch(x, n, norm, lengths, a, c, lb, dom)
            in_place = (i + D) % 3 == 0
            got = host_filter(program, wide, D, lengths, n, a, c, lb, dom, norm == "ortho", ld_out=D + 3, in_place=in_place)
            assert verdict(got, D, ref, live, dt, in_place) is None, (D, tabs, lb, dom, norm, in_place)
    print("kernel text against the model, n=%d T=%d: worst error / bound so far: float32 %.3g, float64 %.3g" % (n, T, WORST[F32], WORST[F64]))


def test_no_lengths(program):
    rng = np.random.RandomState(5)
    x, wide, live = case(rng, 2, 61, 3, None, 64, F64)
    A, C = tables(rng, 33, 3)
    got = host_filter(program, wide, 3, None, 64, A, C, 20, True, False, ld_out=3)
    assert verdict(got, 3, MM.filter_batch(x, 64, None, None, A, C, 20, True), live, F64, False) is None


def test_two_launches_for_three_utterances(sliced, program, dt=F64):
    """The build whose grid takes 4 workgroups: D = 3 is two workgroups per utterance, so utterances 0 and 1 go in one launch and
    utterance 2 in a second, at offset x, out and lengths.  The same bits as the one launch of the other build."""
    rng = np.random.RandomState(9)
    n, T, D, lengths = 64, 61, 3, [5, 0, 61]
    x, wide, live = case(rng, 3, T, D, lengths, n, dt)
    A, C = tables(rng, 33, D)
    ref = MM.filter_batch(x, n, "ortho", lengths, A, C, 9, True)
    got = host_filter(sliced, wide, D, lengths, n, A, C, 9, True, True, ld_out=D + 3)
    assert verdict(got, D, ref, live, dt, False) is None
    assert got.tobytes() == host_filter(program, wide, D, lengths, n, A, C, 9, True, True, ld_out=D + 3).tobytes()
    x, wide, live = case(rng, 3, T, D, lengths, n, F32)
    again = host_filter(sliced, wide, D, lengths, n, A, C, 9, True, True, in_place=True)
    assert verdict(again, D, MM.filter_batch(x, n, "ortho", lengths, A, C, 9, True), live, F32, True) is None
    print("sliced build %s: worst error / bound so far %.3g" % (dt.__name__, WORST[dt]))


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit, lengths=(61, 1, 0)):
    prog = build(tmp_path, edit)
    rng = np.random.RandomState(2)
    n, T, D = 64, 61, 3
    x, wide, live = case(rng, 3, T, D, list(lengths), n, F64)
    ref = MM.filter_batch(x, n, None, list(lengths), None, None, 20, True)
    got = host_filter(prog, wide, D, list(lengths), n, None, None, 20, True, False, ld_out=D + 3, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return "sanitizer"
    return verdict(got, D, ref, live, F64, False)


def test_planted_read_one_row_past_live(tmp_path):
    """Row `live` is loaded: the NaN of utterance 1's row 1 comes out."""
    assert planted(tmp_path / "a", ("modspec_filter.hip", "if (t < live) {", "if (t <= live) {")) == "not finite"


def test_planted_store_one_column_past_d(tmp_path):
    """The last pair of an odd D stores its second column: the sentinel behind column D - 1 is gone (in the last row of the last
    utterance the store leaves the heap block when ld_out == D)."""
    assert planted(tmp_path / "a", ("modspec_filter.hip", "const bool two = d + 1 < p.D;", "const bool two = d + 1 <= p.D;")) in (
        "a foreign column of out was written", "not finite")


def test_planted_data_block_against_padded_len(tmp_path):
    """padded_len(n) leaves two spare slots behind the largest padded index, n + n/16 - 2; three fewer and element n - 1 lies on
    the first twiddle: whichever of the two stores comes second, the result is wrong."""
    edit = ("modspec_fft.h", "constexpr int padded_len(int n) { return n + (n >> 4) + 1; }",
            "constexpr int padded_len(int n) { return n + (n >> 4) - 2; }")
    assert str(planted(tmp_path / "a", edit)).startswith(("error", "sanitizer", "not finite"))


def test_planted_lds_one_element_short_of_the_last_twiddle(tmp_path):
    """n = 4096 needs 32 + 128 + 512 + 2048 = 2720 twiddles of the 4096 the block has room for; a block that ends one element
    short of the last of them is an overrun the sanitizer sees."""
    edit = ("modspec_filter.hip", "((size_t)padded_len(p.n) + (size_t)p.n);", "((size_t)padded_len(p.n) + (size_t)(p.n == 4096 ? 2719 : p.n));")
    prog = build(tmp_path / "a", edit)
    rng = np.random.RandomState(2)
    x, wide, live = case(rng, 1, 4096, 1, [7], 4096, F64)
    got = host_filter(prog, wide, 1, [7], 4096, None, None, 20, True, False, ld_out=1, check=False)
    assert isinstance(got, subprocess.CompletedProcess) and "AddressSanitizer" in got.stderr
