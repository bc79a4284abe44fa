"""The text of csrc/joint_rows.hip run on the CPU (-m "not gpu"): compiled for the host against the shim tests/gmm_host/common.h
plus tests/joint_host/extras.h into a stand-alone program under the address and undefined-behaviour sanitizers, run as a child
process, and compared with tools/joint_model.py bit for bit (byte views: NaNs and -0.0 count), `offsets` included -- the contract
tests/test_joint_gpu.py holds.  This checks the index logic: the tiles, the masks, the scan with its carry, the ranks, the clamp
of the neighbour reads, `cap`, the slices of more tiles than a grid takes.  Every array is an exact-size heap block; the sources
are column slices of wider rows whose other columns hold NaN; rows at or past a length hold NaN; `out` is pre-filled with -7,
which its foreign columns and the rows past min(N, cap) must still hold; the workspace has exactly the bytes the library asks
for.  Nothing is loaded into Python under a sanitizer.  The case list is tests/joint_cases.py.

Three planted defects show that the harness bites: see test_planted_*."""
import os
import subprocess

import numpy as np
import pytest

import joint_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
CASES = JC.cases()
WORST = {"runs": 0, "unequal": 0}


def build(d, edit=None, flags=()):
    """The host program of the kernel text in directory d; `edit` (old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "joint_rows.hip")).read()
    if edit is not None:
        assert src.count(edit[0]) == 1, edit[0]
        src = src.replace(edit[0], edit[1])
    os.makedirs(d / "csrc" / "x")
    os.makedirs(d / "include")
    (d / "csrc" / "x" / "joint_rows_host.inc").write_text(src)
    (d / "include" / "nnmnkwii_joint.h").write_text(open(os.path.join(ROOT, "include", "nnmnkwii_joint.h")).read())
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/joint_host", "extras.h"), ("tests/joint_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "joint_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", *flags, "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("joint_host"))


@pytest.fixture(scope="module")
def sliced_program(tmp_path_factory):
    """At most four workgroups per launch: the nine tiles of a batch of three utterances go in three slices."""
    return build(tmp_path_factory.mktemp("joint_host_sliced"), flags=("-DSHIM_MAX_WORKGROUPS=4",))


def host_run(program, case, check=True):
    """(out (cap, ld_out), offsets, off_out), or the finished process if it failed and check is False."""
    dd, exe = program
    X, Y = JC.typed(case)
    dx, dy, do = (np.dtype(t) for t in case["dtypes"])
    B, Tmax, Dx = X.shape
    Dy = 0 if Y is None else Y.shape[2]
    W, cap = JC.width(case), JC.capacity(case)
    (ld_x, off_x), (ld_y, off_y) = (Dx + 2, 1), (Dy + 3, 2)
    ld_out, off_out = W + case["pad"] + 2, 1
    lx, ly = case["len_x"], case["len_y"]
    wl, wu, wc = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32), np.zeros(136)
    k = 0
    for w, (l, u, c) in enumerate(case["wins"]):
        wl[w], wu[w] = l, u
        wc[k:k + l + u + 1] = c
        k += l + u + 1
    head = [B, Tmax, Dx, Dy, ld_x, off_x, ld_y, off_y, DT_CODE[dx], DT_CODE[dy], DT_CODE[do], len(case["wins"]), case["keep"], lx is not None,
            ly is not None, cap, ld_out, off_out]
    with open(dd / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        f.write(np.array([case["eps"]], dtype=np.float64).tobytes())
        f.write(wl.tobytes() + wu.tobytes() + wc.tobytes())
        for n in (lx, ly):
            f.write((n if n is not None else np.zeros(B)).astype(np.int32).tobytes())
        f.write(JC.wide_source(X, lx, 2, off_x).tobytes())
        if Y is not None:
            f.write(JC.wide_source(Y, ly, 3, off_y).tobytes())
    r = subprocess.run([exe, str(dd / "in.bin"), str(dd / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    assert "launches %d" % (0 if B * Tmax * W == 0 else 1 + (cap > 0)) in r.stderr        # one count, one write
    raw = open(dd / "out.bin", "rb").read()
    offsets = np.frombuffer(raw[:8 * (B + 1)], dtype=np.int64)
    out = np.frombuffer(raw[8 * (B + 1):], dtype=do).reshape(cap, ld_out)
    return out, offsets, off_out


def run_verdict(program, case, check=True):
    got = host_run(program, case, check)
    if isinstance(got, subprocess.CompletedProcess):
        return got
    out, offsets, off = got
    return JC.verdict(case, out, offsets, off=off)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_text_equals_the_model(program, case):
    fails = run_verdict(program, case)
    WORST["runs"] += 1
    WORST["unequal"] += bool(fails)
    assert fails == []


def test_more_tiles_than_a_grid_go_in_slices(sliced_program):
    for name in ("t131-b3-d65-130-w3-f32", "cap-below", "live-w3"):
        case = next(c for c in CASES if c["name"] == name)
        assert run_verdict(sliced_program, case) == []


def test_worst_figure(program):
    print("kernel text against the model: %d runs, %d not bit-equal (bound: bit equality, worst error / bound = %d)"
          % (WORST["runs"], WORST["unequal"], WORST["unequal"]))
    assert WORST["runs"] == len(CASES) and WORST["unequal"] == 0


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit, name):
    """What fails in one run of case `name` on the text with `edit` ([]: the defect went unseen)."""
    prog = build(tmp_path, edit)
    case = next(c for c in CASES if c["name"] == name)
    got = run_verdict(prog, case, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return ["sanitizer"]
    return got


def test_planted_rank_off_by_one(tmp_path):
    edit = ("__popcll(m & ((1ull << f) - 1))", "__popcll(m & ((2ull << f) - 1))")
    assert planted(tmp_path, edit, "t63-b3-d5-5-w3") != []


def test_planted_keep_rule_takes_the_threshold_itself(tmp_path):
    edit = ("if (s > a.eps) bits", "if (s >= a.eps) bits")
    assert "offsets" in planted(tmp_path, edit, "threshold-1e-7")


def test_planted_neighbour_read_not_clamped_at_the_length(tmp_path):
    edit = ("if (tt >= 0 && tt < len) acc", "if (tt >= 0 && tt < a.Tmax) acc")
    assert planted(tmp_path, edit, "mix-float64-float32-float64") != []
