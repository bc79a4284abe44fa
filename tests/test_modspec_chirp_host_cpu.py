"""The text of csrc/modspec_chirp.hip with csrc/modspec_fft.h run on the CPU (-m "not gpu"): compiled for the host against the
shim tests/gmm_host/common.h plus tests/chirp_host/extras.h into a stand-alone program under the address and undefined-behaviour
sanitizers, run as a child process, and compared with tools/chirp_model.py within the figures tests/test_modspec_chirp_gpu.py
asks of the device.  The dynamic LDS of every launch (sized by the host from M) and the scratch that holds the two tables are
exact-size heap blocks, the scratch filled with 0xFF bytes (NaN), so the largest padded index, the last twiddle, w[n - 1] and
F[M - 1] are checked against their blocks and a read of a table entry nobody wrote shows as NaN.  The entries are float64 and
dense (no row stride, no lengths): every input and output is an exact-size heap block, outputs pre-filled with -7.  A workgroup
is 1024 threads and every call launches three kernels: the batches are small.  Nothing is loaded into Python under a sanitizer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chirp_model as CM  # noqa: E402

# relative to the reference's largest element, as tests/test_modspec_chirp_gpu.py::test_parity_and_route: spectrum, inverse,
# smoothing, gradient; the phase absolutely, at the bins above 1e-6 of the largest power
BOUND = {"spectrum": 1e-11, "inverse": 1e-11, "smoothing": 1e-9, "gradient": 1e-10, "phase": 1e-8}
MARKER = "extern __shared__ __align__(16) unsigned char smem[];"
SENTINEL = -7
WORST = dict.fromkeys(BOUND, 0.0)


def test_the_bounds_are_the_gpu_tests():
    text = open(os.path.join(ROOT, "tests", "test_modspec_chirp_gpu.py")).read()
    for what, before in (("spectrum", "_close(ms, mo, "), ("inverse", "OM.inv_modspec(m, p, norm=norm), mo, po), "),
                         ("smoothing", "_close(y, yo, "), ("gradient", "OM.modspec_grad(x[b], w[b], n, norm), "),
                         ("phase", "assert np.abs(ph - po)[big].max() < ")):
        assert text.count(before) == 1, before
        assert float(re.match(r"[0-9.e+-]+", text[text.index(before) + len(before):]).group(0)) == BOUND[what], what
    assert text.count("big = mo > 1e-6 * mo.max()") == 1


def build(d, edit=None):
    """The host program of the kernel text in directory d; `edit` (file, old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    csrc = os.path.join(ROOT, "nnmnkwii_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("modspec_chirp.hip", "modspec_fft.h")}
    assert text["modspec_chirp.hip"].count(MARKER) == 2 and text["modspec_chirp.hip"].count("extern __shared__") == 2   # two kernels
    assert text["modspec_fft.h"].count("extern __shared__") == 0
    text["modspec_chirp.hip"] = text["modspec_chirp.hip"].replace(MARKER, "unsigned char *smem = (unsigned char *)g_dyn_lds;")
    if edit is not None:
        assert text[edit[0]].count(edit[1]) == 1, edit[1]
        text[edit[0]] = text[edit[0]].replace(edit[1], edit[2])
    os.makedirs(d / "csrc" / "x")
    (d / "csrc" / "x" / "modspec_chirp_host.inc").write_text(text["modspec_chirp.hip"])
    (d / "csrc" / "x" / "modspec_fft.h").write_text(text["modspec_fft.h"])
    for sub, name, to in (("tests/gmm_host", "common.h", "common.h"), ("tests/msfilter_host", "extras.h", "fft_extras.h"),
                          ("tests/chirp_host", "extras.h", "extras.h"), ("tests/chirp_host", "main.cpp", "main.cpp")):
        (d / to).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "chirp_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-Wno-unused-function", "-I", str(d), str(d / "main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("chirp_host"))


def host_chirp(program, mode, n, arrays, B, T, D, ortho=False, limit_bin=0, log_domain=True, want_phase=False, check=True):
    """The output file as float64, or the finished process if it failed and check is False."""
    d, exe = program
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([mode, B, T, D, n, ortho, limit_bin, log_domain, want_phase], dtype=np.int64).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    return np.frombuffer(open(d / "out.bin", "rb").read())


def traj(rng, B, T, D):
    return 0.1 * np.cumsum(rng.randn(B, T, D), axis=1) + rng.rand(B, T, D)


def rel(what, got, ref):
    """The error relative to the reference's largest element, or inf if an element is not finite or still the sentinel."""
    if got.shape != ref.shape or not np.isfinite(got).all():
        return np.inf
    e = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
    WORST[what] = max(WORST[what], e / BOUND[what])
    return e


def run_mode(program, mode, rng, n, B, T, D, ortho, check=True):
    """One call of `mode` against the model: {figure: error}, or the failed process."""
    nb = n // 2 + 1
    x = traj(rng, B, T, D)
    errs = {}
    if mode == CM.MODE_SPEC:
        raw = host_chirp(program, mode, n, [x], B, T, D, ortho, want_phase=True, check=check)
        if isinstance(raw, subprocess.CompletedProcess):
            return raw
        ms = raw[:B * nb * D].reshape(B, nb, D)
        ph = raw[B * nb * D:].reshape(B, nb, D, 2)
        want = [CM.modspec(x[b], n, ortho) for b in range(B)]
        mo = np.stack([w[0] for w in want])
        po = np.stack([w[1] for w in want])
        errs["spectrum"] = rel("spectrum", ms, mo)
        big = mo > 1e-6 * mo.max()
        e = float(np.abs((ph[..., 0] + 1j * ph[..., 1]) - po)[big].max()) if np.isfinite(ph).all() else np.inf
        WORST["phase"] = max(WORST["phase"], e / BOUND["phase"])
        errs["phase"] = e
        if n == 100:   # without the phase: the same bits
            assert host_chirp(program, mode, n, [x], B, T, D, ortho).tobytes() == ms.tobytes()
    elif mode == CM.MODE_INVERSE:
        S = np.fft.rfft(traj(rng, B, n, D), n=n, axis=1)
        ms, ph = np.abs(S) ** 2, CM.unit_phasor(S)
        raw = host_chirp(program, mode, n, [ms, np.stack([ph.real, ph.imag], axis=-1)], B, T, D, ortho, check=check)
        if isinstance(raw, subprocess.CompletedProcess):
            return raw
        errs["inverse"] = rel("inverse", raw.reshape(B, n, D), np.stack([CM.inv_modspec(ms[b], ph[b], n, ortho) for b in range(B)]))
    elif mode == CM.MODE_SMOOTH:
        # limit_bin 0, inside and n/2 + 1 and the two domains take turns over the calls (a call is three launches of 1024 threads)
        for limit_bin, log_domain in (((0, True), (nb // 2, False), (nb, True), (nb // 2, True))[(n + D) % 4],):
            raw = host_chirp(program, mode, n, [x], B, T, D, ortho, limit_bin, log_domain, check=check)
            if isinstance(raw, subprocess.CompletedProcess):
                return raw
            want = np.stack([CM.modspec_smoothing(x[b], n, limit_bin, log_domain, ortho) for b in range(B)])
            errs["smoothing"] = max(errs.get("smoothing", 0.0), rel("smoothing", raw.reshape(B, T, D), want))
    else:
        g = rng.rand(B, nb, D)
        raw = host_chirp(program, mode, n, [x, g], B, T, D, ortho, check=check)
        if isinstance(raw, subprocess.CompletedProcess):
            return raw
        errs["gradient"] = rel("gradient", raw.reshape(B, T, D), np.stack([CM.modspec_backward(x[b], g[b], n, ortho) for b in range(B)]))
    return errs


@pytest.mark.parametrize("n", [3, 5, 100, 1000, 2047])
@pytest.mark.parametrize("mode", range(4))
def test_kernel_text_on_the_host(program, n, mode):
    """T below n with D = 3 (a pair and a lone column) in a batch of two, and T == n with D = 1; the normalisations in turn."""
    rng = np.random.RandomState(10 * n + mode)
    for B, T, D, ortho in ((2, max(1, n - 2 if n < 100 else n // 3), 3, mode % 2 == 0), (1, n, 1, mode % 2 == 1)):
        errs = run_mode(program, mode, rng, n, B, T, D, ortho)
        for what, e in errs.items():
            assert e <= BOUND[what], (what, n, B, T, D, ortho, e)
    print("kernel text against the model, n=%d mode %d: worst error / bound so far: %s"
          % (n, mode, ", ".join("%s %.3g" % kv for kv in WORST.items())))


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit, mode=CM.MODE_SPEC, n=100, T=33):
    prog = build(tmp_path, edit)
    got = run_mode(prog, mode, np.random.RandomState(1), n, 1, T, 3, False, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return "sanitizer"
    return "passed" if all(e <= BOUND[k] for k, e in got.items()) else "mismatch"


def test_planted_read_one_row_past_t(tmp_path):
    """Row T of x is loaded: behind the last utterance it lies outside the heap block."""
    assert planted(tmp_path / "a", ("modspec_chirp.hip", "if (t < T) {", "if (t <= T) {")) == "sanitizer"


def test_planted_scratch_one_table_entry_short(tmp_path):
    """The scratch without its last double2: chirp_filter's store of F[M - 1] leaves it."""
    edit = ("modspec_chirp.hip", "w_bytes + (size_t)p.M * sizeof(double2));", "w_bytes + (size_t)(p.M - 1) * sizeof(double2));")
    assert planted(tmp_path / "a", edit) == "sanitizer"


def test_planted_table_entry_nobody_wrote(tmp_path):
    """chirp_table stops one entry early: w[n - 1] is still the scratch's 0xFF bytes, a NaN that T == n brings into the result."""
    edit = ("modspec_chirp.hip", "if (j >= n) return;", "if (j >= n - 1) return;")
    assert planted(tmp_path / "a", edit, T=100) == "mismatch"


def test_planted_data_block_against_padded_len(tmp_path):
    """padded_len(M) leaves two spare slots behind the largest padded index, M + M/16 - 2; three fewer and element M - 1 lies on
    the first twiddle: whichever store comes second, the result is wrong."""
    edit = ("modspec_fft.h", "constexpr int padded_len(int n) { return n + (n >> 4) + 1; }",
            "constexpr int padded_len(int n) { return n + (n >> 4) - 2; }")
    assert planted(tmp_path / "a", edit, mode=CM.MODE_SMOOTH) in ("mismatch", "sanitizer")
