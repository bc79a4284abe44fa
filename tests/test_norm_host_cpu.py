"""The text of csrc/colstats.hip run on the CPU (-m "not gpu"): compiled for the host against the shim tests/gmm_host/common.h
plus tests/norm_host/extras.h into a stand-alone program under the address and undefined-behaviour sanitizers, run as a child
process, and compared with tools/norm_model.py.  This checks the partition into workgroups, waves and chunks, the masking of pad
frames (they hold NaN, and every array is an exact-size heap block), the partials in the workspace, the finish step and the apply
kernel's strides.  Nothing is loaded into Python under a sanitizer.

The bound of device against truth (tests/norm_cases.py) comes from here: the worst |mean - truth| / S_mean and
|var - truth| / S_var of the kernel text over HOST_SHAPES is printed, and asserted to be at most the recorded WORST_RATIO."""
import os
import re
import subprocess

import numpy as np
import pytest

import norm_cases as C
from norm_cases import NM

ROOT = C.ROOT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from nnmnkwii_amd.csrc import build as hip_build
    d = tmp_path_factory.mktemp("norm_host")
    (d / "colstats_host.inc").write_text(open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "colstats.hip")).read())
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/norm_host", "extras.h"), ("tests/norm_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    defs = ["-D%s=%s" % (n, re.search(r"^#define\s+%s\s+(\d+)" % n, header, re.M).group(1))
            for n in ("MLPG_HIP_COLSTATS_CHUNK_ROWS", "MLPG_HIP_COLSTATS_BLOCK_ROWS")]
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "norm_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", *defs, "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def _run(program, head, arrays):
    d, exe = program
    with open(d / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(d / "out.bin", "rb").read()


def _wide(X, ld, fill):
    """X as columns 0 .. D - 1 of a (B, Tmax, ld) array whose other columns hold `fill`."""
    W = np.full(X.shape[:2] + (ld,), fill, dtype=X.dtype)
    W[:, :, :X.shape[2]] = X
    return W


def host_stats(program, X, lengths, state=None, ld=None, in_place=False):
    B, Tmax, D = X.shape
    ld = D if ld is None else ld
    L = lengths if lengths is not None else np.zeros(B, dtype=np.int32)
    arrays = [L.astype(np.int32), _wide(X, ld, np.nan)] + ([state.astype(np.float64)] if state is not None else [])
    raw = _run(program, [0, B, Tmax, D, ld, int(X.dtype == np.float64), lengths is not None, state is not None, in_place, 0, 0, 0], arrays)
    out = np.frombuffer(raw[:40 * D]).reshape(5, D)
    return out, np.frombuffer(raw[40 * D:]).reshape(-1, 5, D)


def host_affine(program, X, lengths, a, c, mode, out_dtype, ld_x=None, ld_y=None, in_place=False):
    B, Tmax, D = X.shape
    ld_x = D if ld_x is None else ld_x
    ld_y = ld_x if in_place else (D if ld_y is None else ld_y)
    L = lengths if lengths is not None else np.zeros(B, dtype=np.int32)
    od = X.dtype if in_place else np.dtype(out_dtype)
    raw = _run(program, [1, B, Tmax, D, ld_x, int(X.dtype == np.float64), lengths is not None, 0, in_place, int(od == np.float64), ld_y, mode],
               [L.astype(np.int32), _wide(X, ld_x, 3.0), a.astype(np.float64), c.astype(np.float64)])
    return np.frombuffer(raw, dtype=od).reshape(B, Tmax, ld_y)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize("B,D", C.HOST_SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_statistics_kernel_text_on_the_host(program, B, D, dtype):
    lengths = C.LENGTHS[B]
    X, L = C.padded(B * 100 + D, lengths, D, dtype)
    use_lengths = not (B == 1)                   # B == 1: lengths = NULL, every frame live
    state, parts = host_stats(program, X, L if use_lengths else None, ld=D + (B % 3))
    m_parts = NM.partials(X, L if use_lengths else None)
    m_state = NM.finish(m_parts, D)
    # the compiler of the host build rounds every operation as numpy does: the model's bits, partials included
    assert parts.shape == m_parts.shape and same_bits(parts, m_parts)
    assert same_bits(state, m_state)
    if sum(lengths) == 0:
        return
    truth = NM.exact(X, L if use_lengths else None)
    count, mean, var, mn, mx = NM.stats_of(state)
    live = [X[b, :max(n, 0)] for b, n in enumerate(lengths)]
    assert count == truth["count"]
    assert np.array_equal(mn, np.concatenate(live).min(axis=0)) and np.array_equal(mx, np.concatenate(live).max(axis=0))
    for k, const in C.CONSTANT.items():          # constant columns: exact
        for d in range(k, D, len(C.COLUMNS)):
            assert mean[d] == dtype(const) and var[d] == 0.0
    r = NM.ratios(mean, var, truth)
    print("kernel text against the truth: mean %.3f S_mean, var %.3f S_var (recorded worst %.2f)" % (r[0], r[1], C.WORST_RATIO))
    assert max(r) <= C.WORST_RATIO


def test_incoming_state_in_place_and_streaming(program):
    lengths = C.LENGTHS[5]
    X, L = C.padded(7, lengths, 12)
    whole, _ = host_stats(program, X, L)
    first, _ = host_stats(program, X[:2], L[:2])
    both, _ = host_stats(program, X[2:], L[2:], state=first, in_place=True)
    assert same_bits(both, NM.kernel_state(X[2:], L[2:], NM.kernel_state(X[:2], L[:2])))
    truth = NM.exact(X, L)
    assert C.stats_ok(whole, truth, C.WORST_RATIO) and C.stats_ok(both, truth, 2 * C.WORST_RATIO)
    assert np.array_equal(both[3:], whole[3:]) and np.array_equal(both[0], whole[0])
    # no live frame: the incoming state, or the empty one
    none, _ = host_stats(program, X, np.zeros(5, dtype=np.int32), state=first)
    assert same_bits(none, first)
    none, _ = host_stats(program, X, np.zeros(5, dtype=np.int32))
    assert same_bits(none, NM.empty_state(12))


def test_nan_and_inf_columns(program):
    X, L = C.padded(3, [40, 3], 4)
    X[0, 17, 1] = np.nan
    X[1, 2, 2] = np.inf
    state, _ = host_stats(program, X, L)
    assert same_bits(state, NM.kernel_state(X, L))
    count, mean, var, mn, mx = NM.stats_of(state)
    assert count == 43 and np.isnan(mean[[1, 2]]).all() and np.isnan(var[[1, 2]]).all() and np.isfinite(mean[[0, 3]]).all()
    assert np.isnan(mn[1]) and np.isnan(mx[1]) and mx[2] == np.inf and np.isfinite(mn[2])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt_in,dt_out", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)])
def test_apply_kernel_text_on_the_host(program, mode, dt_in, dt_out):
    D = 65
    X, L = C.padded(11, [0, 70, 33], D, dt_in)
    rng = np.random.RandomState(mode)
    a, c = rng.rand(D) + 0.5, rng.randn(D)
    y = host_affine(program, X, L, a, c, mode, dt_out, ld_x=D + 2, ld_y=D + 3)
    assert same_bits(y[:, :, :D], NM.affine(X, a, c, mode, L, dt_out))
    assert (y[:, :, D:] == -7).all()                         # columns past D are not touched
    if dt_in == dt_out:
        z = host_affine(program, X, L, a, c, mode, dt_out, ld_x=D + 2, in_place=True)
        assert same_bits(z[:, :, :D], NM.affine(X, a, c, mode, L, dt_out)) and (z[:, :, D:] == 3).all()
    y = host_affine(program, X[2:3], None, a, c, mode, dt_out)      # lengths = NULL (the pad frames' NaN goes through)
    assert np.array_equal(np.isnan(y[0, :, 0]), np.arange(70) >= 33)
