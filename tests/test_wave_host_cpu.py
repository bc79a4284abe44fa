"""The text of csrc/wave_codec.hip run on the CPU (-m "not gpu"): compiled for the host against the shim tests/gmm_host/common.h
plus tests/wave_host/extras.h into a stand-alone program under the address and undefined-behaviour sanitizers, run as a child
process, and compared with tools/wave_model.py -- bit for bit (integer views: NaNs and -0.0 count) wherever no transcendental is
involved, which is every de-emphasis, table and pre-emphasis case: the contract tests/test_wave_gpu.py holds for the device.  This
checks the index logic: 4 samples per thread with and without the 16-byte accesses (the sanitizer sees a misaligned one), the left
neighbour, the local recurrence, the scan and its multipliers, the carry, the segments and their warm-up, the padding, the
slices of a batch over the grid's limit.  Every array is an exact-size heap block; the batch sits inside wider rows ("wide") or
fills them ("dense"); samples at or past lengths[b] hold NaN or classes far outside the table.  Nothing is loaded into Python
under a sanitizer.  The case list is tests/wave_cases.py.

Three planted defects show that the harness bites: see test_planted_*."""
import os
import subprocess

import numpy as np
import pytest

import wave_cases as WC
from wave_cases import WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = WC.cases()
WORST = {"runs": 0, "failed": 0}


def build(d, edit=None, flags=()):
    """The host program of the kernel text in directory d; `edit` (old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "wave_codec.hip")).read()
    if edit is not None:
        assert src.count(edit[0]) == 1, edit[0]
        src = src.replace(edit[0], edit[1])
    os.makedirs(d / "csrc" / "x")
    os.makedirs(d / "include")
    (d / "csrc" / "x" / "wave_codec_host.inc").write_text(src)
    (d / "include" / "nnmnkwii_wave.h").write_text(open(os.path.join(ROOT, "include", "nnmnkwii_wave.h")).read())
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/wave_host", "extras.h"), ("tests/wave_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "wave_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", *flags, "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wave_host"))


@pytest.fixture(scope="module")
def sliced_program(tmp_path_factory):
    """At most five workgroups per launch."""
    return build(tmp_path_factory.mktemp("wave_host_sliced"), flags=("-DSHIM_MAX_WORKGROUPS=5",))


def host_run(program, case, check=True):
    """(rc, x after the call, y after it), or the finished process if it failed and check is False."""
    dd, exe = program
    x, y = WC.buffers(case)
    B, Lmax = case["X"].shape
    ld_x, off_x, ld_y, off_y = WC.layout_of(case)
    lengths = case["lengths"]
    table = WM.inv_mulaw_table(case["mu"]) if case["op"] == "decode" and case["stage"] == WM.QUANTIZE else np.zeros(0, np.float32)
    in_place = case["mode"] in ("inplace", "refused")           # (what is refused here is y being x)
    head = [case["op"] == "decode", B, Lmax, ld_x, off_x, ld_y, off_y, WM.CODE[x.dtype], WM.CODE[y.dtype], lengths is not None, in_place,
            case["coef"] is not None, case["stage"], case["mu"], min(case["segment"], 1 << 40), len(table)]
    with open(dd / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        f.write(np.array([case["coef"] if case["coef"] is not None else 0.0]).tobytes())
        f.write((lengths if lengths is not None else np.zeros(B)).astype(np.int32).tobytes())
        f.write(table.tobytes())
        f.write(x.tobytes())
        f.write(y.tobytes())
    r = subprocess.run([exe, str(dd / "in.bin"), str(dd / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dd / "out.bin", "rb").read()
    rc, launches = np.frombuffer(raw[:16], dtype=np.int64)
    assert launches == (rc == 0)
    xa = np.frombuffer(raw[16:16 + x.nbytes], dtype=x.dtype).reshape(x.shape)
    ya = np.frombuffer(raw[16 + x.nbytes:], dtype=y.dtype).reshape(y.shape)
    return int(rc), xa, ya


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_text_equals_the_model(program, case):
    fails = WC.verdict(case, host_run(program, case))
    WORST["runs"] += 1
    WORST["failed"] += bool(fails)
    assert fails == []


def test_a_batch_over_the_grid_limit_goes_in_slices(sliced_program):
    for name in ("deemph-seg2048-f64", "preemph-quantize-i32", "table-uint8"):
        case = next(c for c in CASES if c["name"] == name)          # 12 utterances of up to 4 segments or 7 tiles, five to a launch
        assert WC.verdict(case, host_run(sliced_program, case)) == []


def test_worst_figure(program):
    print("kernel text against the model: %d runs, %d with a difference (bound: bit equality where no transcendental is involved, "
          "worst error / bound = %d)" % (WORST["runs"], WORST["failed"], WORST["failed"]))
    assert WORST["runs"] == len(CASES) and WORST["failed"] == 0


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit, name):
    """What fails in one run of case `name` on the text with `edit` ([]: the defect went unseen)."""
    prog = build(tmp_path, edit)
    case = next(c for c in CASES if c["name"] == name)
    got = host_run(prog, case, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return ["sanitizer"]
    return WC.verdict(case, got)


def test_planted_tile_carry_dropped(tmp_path):
    edit = ("if (tid == 0) v[0] = v[0] + c * carry;", "if (tid == 0) v[0] = v[0] + c * 0.0;")
    assert any(f.startswith("result") for f in planted(tmp_path, edit, "deemph-none-f64"))


def test_planted_scan_multiplier_off_by_a_power(tmp_path):
    edit = ("const double p1 = t1w + a.pw[6] * t0w;", "const double p1 = t1w + a.pw[5] * t0w;")
    assert any(f.startswith("result") for f in planted(tmp_path, edit, "deemph-none-f64"))


def test_planted_warm_up_one_tile_short(tmp_path):
    edit = ("seg > 0 && lo < L ? lo - a.W : lo;", "seg > 0 && lo < L ? lo - a.W + kWaveTile : lo;")
    assert any(f.startswith("result") for f in planted(tmp_path, edit, "deemph-seg2048-f64"))
    # the same text is clean where nothing is split
    assert planted(tmp_path / "again", edit, "deemph-none-f32") == []
