"""The text of csrc/kmeans.hip run on the CPU (-m "not gpu"): the file is compiled for the host against tests/gmm_host/common.h --
workgroups as threads on a barrier -- into a stand-alone program (tests/kmeans_host/main.cpp) under the address and
undefined-behaviour sanitizers, and the seed step and the Lloyd step are compared with tests/kmeans64.py.  This checks the index
arithmetic, the row tails, the slice and workspace layout, the LDS layout and every bound of an array, at N = 65601 with two
64-row tiles per slice and trailing slices without rows; the bounds are those of the GPU test (tests/test_kmeans_gpu.py): 1e-10
of the reference's maximum, counts and labels exact."""
import os
import subprocess

import numpy as np
import pytest

import kmeans64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from nnmnkwii_amd.csrc import build as hip_build
    d = tmp_path_factory.mktemp("kmeans_host")
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "kmeans.hip")).read()
    marker = "extern __shared__ double lds[];"
    assert src.count(marker) == 2
    (d / "kmeans_host.inc").write_text(src.replace(marker, "double *lds = g_dyn_lds;"))
    (d / "common.h").write_text(open(os.path.join(ROOT, "tests", "gmm_host", "common.h")).read())
    (d / "main.cpp").write_text(open(os.path.join(ROOT, "tests", "kmeans_host", "main.cpp")).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "kmeans_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.mark.parametrize("N,F,K", [(1, 1, 1), (63, 2, 3), (65, 17, 16), (130, 50, 16), (67, 128, 2), (20, 5, 64), (65601, 1, 2)])
def test_kernel_text_on_the_host(program, N, F, K):
    d, exe = program
    C = 1 + (N + F + K) % 8
    case = R.step_case(N, F, K, C, N + F + K)
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([N, F, K, C], dtype=np.int64).tobytes())
        for name in ("X", "shift", "closest", "centers"):
            f.write(np.ascontiguousarray(case[name], dtype=np.float64).tobytes())
        for name in ("cand", "prev"):
            f.write(np.ascontiguousarray(case[name], dtype=np.int64).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.fromfile(d / "out.bin")
    pos = [0]

    def take(*shape):
        n = int(np.prod(shape))
        a = out[pos[0]:pos[0] + n].reshape(shape)
        pos[0] += n
        return a
    d0, p0, d1, p1 = take(C, N), take(C), take(C, N), take(C)
    labels, min_dist, sums, counts, centers, st1 = take(N), take(N), take(K, F), take(K), take(K, F), take(4)
    labels2, st2 = take(N), take(4)
    assert pos[0] == len(out)
    Xc = case["X"] - case["shift"]
    for got_d, got_p, closest in ((d0, p0, None), (d1, p1, case["closest"])):
        d_r, p_r = R.seed_step(Xc, case["cand"], closest)
        assert R.dist(got_d, d_r) <= 1e-10 and R.dist(got_p, p_r) <= 1e-10, (R.dist(got_d, d_r), R.dist(got_p, p_r))
    ref = R.step_expected(case)
    R.check_step(case, ref, dict(labels=labels.astype(np.int32), min_dist=min_dist, sums=sums, counts=counts, centers=centers,
                                 shift=st1[0], inertia=st1[1], changed=int(st1[2]), empty=int(st1[3])))
    # the centre update turned off, started from the labels just found: nothing changed, no shift
    assert np.array_equal(labels2, labels) and st2[2] == 0 and st2[0] == 0.0 and st2[3] == ref["empty"]
    assert R.dist(st2[1], ref["inertia"]) <= 1e-10
