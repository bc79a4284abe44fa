"""The text of csrc/f0_interp.hip run on the CPU (-m "not gpu"): compiled for the host against the shim tests/gmm_host/common.h
plus tests/f0_host/extras.h into a stand-alone program under the address and undefined-behaviour sanitizers, run as a child
process, and compared with tools/f0_model.py bit for bit (integer views: NaNs and -0.0 count), the contract tests/test_f0_gpu.py
holds.  This checks the index logic: the two scans, the carry, the look-ahead and what is kept of it, the edge holds, the
slices of a batch over the grid's limit.  Every array is an exact-size heap block; x is a column slice of wider rows whose other
columns hold NaN; rows at or past lengths[b] hold NaN; the outputs are pre-filled with -7, which their foreign columns and
nothing else must still hold.  Nothing is loaded into Python under a sanitizer.  The case list is tests/f0_cases.py.

Three planted defects show that the harness bites: see test_planted_*."""
import os
import subprocess

import numpy as np
import pytest

import f0_cases as FC
from f0_cases import F0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
MODE_CODE = {"both": 0, "y": 1, "vuv": 2, "inplace": 3, "inplace_y": 4}
CASES = FC.cases()
WORST = {"runs": 0, "unequal": 0}


def build(d, edit=None, flags=()):
    """The host program of the kernel text in directory d; `edit` (old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "f0_interp.hip")).read()
    if edit is not None:
        assert src.count(edit[0]) == 1, edit[0]
        src = src.replace(edit[0], edit[1])
    os.makedirs(d / "csrc" / "x")
    os.makedirs(d / "include")
    (d / "csrc" / "x" / "f0_interp_host.inc").write_text(src)
    (d / "include" / "nnmnkwii_f0.h").write_text(open(os.path.join(ROOT, "include", "nnmnkwii_f0.h")).read())
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/f0_host", "extras.h"), ("tests/f0_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "f0_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", *flags, "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("f0_host"))


@pytest.fixture(scope="module")
def sliced_program(tmp_path_factory):
    """At most four workgroups per launch: a batch of fifteen (utterance, column) pairs goes in four slices."""
    return build(tmp_path_factory.mktemp("f0_host_sliced"), flags=("-DSHIM_MAX_WORKGROUPS=4",))


def host_run(program, case, check=True):
    """(x after the call, y, vuv), each (B, Tmax, ld) with the batch in columns off .. off + C - 1, or the finished process if
    it failed and check is False."""
    dd, exe = program
    dx, dy, dv = (np.dtype(t) for t in case["dtypes"])
    X = case["X"].astype(dx)
    B, Tmax, C = X.shape
    (ld_x, off_x), (ld_y, off_y), (ld_v, off_v) = (C + 2, 1), (C + 3, 2), (C + 1, 0)
    wide = np.full((B, Tmax, ld_x), np.nan, dtype=dx)
    wide[:, :, off_x:off_x + C] = X
    lengths = case["lengths"]
    head = [B, Tmax, C, ld_x, off_x, ld_y, off_y, ld_v, off_v, DT_CODE[dx], DT_CODE[dy], DT_CODE[dv], F0.kind_of(case["kind"]),
            lengths is not None, MODE_CODE[case["mode"]]]
    with open(dd / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        f.write((lengths if lengths is not None else np.zeros(B)).astype(np.int32).tobytes())
        f.write(wide.tobytes())
    r = subprocess.run([exe, str(dd / "in.bin"), str(dd / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    assert "launches 1" in r.stderr
    raw = open(dd / "out.bin", "rb").read()
    res, k = [], 0
    for dt, ld in ((dx, ld_x), (dy, ld_y), (dv, ld_v)):
        n = B * Tmax * ld * dt.itemsize
        res.append(np.frombuffer(raw[k:k + n], dtype=dt).reshape(B, Tmax, ld))
        k += n
    assert k == len(raw)
    return res[0], res[1], res[2], wide, (off_x, off_y, off_v)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_text_equals_the_model(program, case):
    fails = FC.verdict(case, host_run(program, case))
    WORST["runs"] += 1
    WORST["unequal"] += bool(fails)
    assert fails == []


def test_a_batch_over_the_grid_limit_goes_in_slices(sliced_program):
    case = next(c for c in CASES if c["name"] == "clamped-lengths")          # B = 5, C = 3: fifteen pairs, four to a launch
    assert FC.verdict(case, host_run(sliced_program, case)) == []
    case = next(c for c in CASES if c["name"] == "lengths-nearest")
    assert FC.verdict(case, host_run(sliced_program, case)) == []


def test_worst_figure(program):
    print("kernel text against the model: %d runs, %d not bit-equal (bound: bit equality, worst error / bound = %d)"
          % (WORST["runs"], WORST["unequal"], WORST["unequal"]))
    assert WORST["runs"] == len(CASES) and WORST["unequal"] == 0


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit, name):
    """What fails in one run of case `name` on the text with `edit` ([]: the defect went unseen)."""
    prog = build(tmp_path, edit)
    case = next(c for c in CASES if c["name"] == name)
    got = host_run(prog, case, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return ["sanitizer"]
    return FC.verdict(case, got)


def test_planted_carry_dropped_across_a_tile_without_a_voiced_frame(tmp_path):
    edit = ("      if (last >= 0) {\n        carry_idx", "      carry_idx = -1;\n      if (last >= 0) {\n        carry_idx")
    assert "y" in planted(tmp_path, edit, "structural-slinear-both")


def test_planted_look_ahead_stops_one_tile_early(tmp_path):
    edit = ("tm < L && !found; tm += kF0Tile)", "tm + kF0Tile < L && !found; tm += kF0Tile)")
    assert "y" in planted(tmp_path, edit, "structural-slinear-both")


def test_planted_flag_taken_after_the_edge_hold(tmp_path):
    edit = ("(TV)(voiced ? 1 : 0)", "(TV)(r > 0.0 ? 1 : 0)")
    assert planted(tmp_path, edit, "structural-slinear-both") == ["vuv"]
