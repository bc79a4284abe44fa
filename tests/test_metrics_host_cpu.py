"""The text of csrc/frame_metrics.hip run on the CPU (-m "not gpu"): compiled for the host against the shim
tests/gmm_host/common.h plus tests/metrics_host/extras.h into a stand-alone program under the address and undefined-behaviour
sanitizers, run as a child process, and compared with tools/metrics_model.py: bit for bit with the model's kernel order (the
partition into workgroups, waves and lanes, the staging of a frame's columns, the partials in the workspace, the finish step),
and with the truth within the model's bound.  Pad frames and the columns no term reads hold NaN, and every array is an
exact-size heap block.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import metrics_cases as C
from metrics_cases import MM

ROOT = C.ROOT
BLOCK = C.BLOCK


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from nnmnkwii_amd.csrc import build as hip_build
    d = tmp_path_factory.mktemp("metrics_host")
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "frame_metrics.hip")).read()
    marker = "extern __shared__ double lds[];"
    assert src.count(marker) == 1
    os.makedirs(d / "csrc" / "x")
    os.makedirs(d / "include")
    (d / "csrc" / "x" / "frame_metrics_host.inc").write_text(src.replace(marker, "double *lds = g_dyn_lds;"))
    (d / "include" / "nnmnkwii_metrics.h").write_text(open(os.path.join(ROOT, "include", "nnmnkwii_metrics.h")).read())
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/metrics_host", "extras.h"), ("tests/metrics_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "metrics_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def host_metrics(program, X, Y, lengths, terms, per_utt=True):
    """(totals, per_utt, partials) of the host build; X and Y as they are (their last dimension is the row stride)."""
    d, exe = program
    B, Tmax = X.shape[:2]
    n = len(terms)
    L = lengths if lengths is not None else np.zeros(B, dtype=np.int32)
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([B, Tmax, X.shape[2], Y.shape[2], X.dtype == np.float64, Y.dtype == np.float64, lengths is not None, n, per_utt],
                         dtype=np.int64).tobytes())
        for a in (L.astype(np.int32), X, Y, C.term_bytes(terms)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = np.frombuffer(open(d / "out.bin", "rb").read())
    k = 2 * n + (2 * n * B if per_utt else 0)
    return raw[:2 * n].reshape(n, 2), (raw[2 * n:k].reshape(B, n, 2) if per_utt else None), raw[k:].reshape(-1, n, 2)


@pytest.mark.parametrize("dtype_x,dtype_y", [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)])
def test_eight_terms_kernel_text_on_the_host(program, dtype_x, dtype_y):
    terms = C.eight_terms()
    lengths = [BLOCK + 3, 0, 5]
    X, Y, L = C.kernel_case(21, lengths, BLOCK + 3, 140 + (dtype_x == np.float64), dtype_x, dtype_y, terms)
    Y = np.concatenate([Y, np.full(Y.shape[:2] + (3,), np.nan, dtype=Y.dtype)], axis=2)          # another row stride
    totals, per_utt, parts = host_metrics(program, X, Y, L, terms)
    m_parts = MM.partials(X, Y, L, terms)
    assert parts.shape == m_parts.shape
    plain = [i for i, t in enumerate(terms) if not t["flags"] & MM.FLAG_EXP]
    assert np.array_equal(parts[:, plain].view(np.int64), m_parts[:, plain].view(np.int64))
    worst = C.check_against_model(totals, per_utt, X, Y, L, terms)
    print("kernel text against the truth: worst error / bound %.3f" % worst)
    assert np.array_equal(per_utt[1], np.zeros((8, 2))) and not parts[2:4].any()     # the empty utterance: zeros


def test_no_lengths_one_term_and_totals_only(program):
    terms = [MM.term(MM.SQUARED, 2, 0, width=3)]
    X, Y = C.pair(5, 2, 6, 5, np.float64)
    totals, per_utt, parts = host_metrics(program, X, Y[:, :, :4].copy(), None, terms, per_utt=False)
    assert per_utt is None and parts.shape == (2, 1, 2)
    C.check_against_model(totals, None, X, Y[:, :, :4], None, terms)
    assert totals[0, 1] == 2 * 6 * 3


def test_no_live_frame_and_lengths_past_the_batch(program):
    terms = C.eight_terms()[:3]
    X, Y, L = C.kernel_case(3, [2, 4], 4, 140, np.float32, np.float32, terms)
    totals, per_utt, parts = host_metrics(program, X, Y, np.array([0, -3], dtype=np.int32), terms)
    assert not totals.any() and not per_utt.any() and not parts.any()
    totals, per_utt, _ = host_metrics(program, X[:, :2], Y[:, :2], np.array([1000, 2], dtype=np.int32), terms)   # clamped to Tmax
    C.check_against_model(totals, per_utt, X[:, :2], Y[:, :2], np.array([2, 2]), terms)
    totals, per_utt, parts = host_metrics(program, X[:0], Y[:0], L[:0], terms)                                      # B == 0
    assert totals.shape == (3, 2) and not totals.any() and parts.size == 0


def test_the_widest_span_the_entry_accepts(program):
    """1000 float64 columns of x and of y: NNMK_METRICS_MAX_ROW_BYTES, one frame staged per wave."""
    terms = [MM.term(MM.FRAME_L2, 0, width=1000), MM.term(MM.SQUARED, 0, width=1000)]
    X, Y = C.pair(9, 1, 6, 1000, np.float64)
    totals, per_utt, _ = host_metrics(program, X, Y, None, terms)
    C.check_against_model(totals, per_utt, X, Y, None, terms)
