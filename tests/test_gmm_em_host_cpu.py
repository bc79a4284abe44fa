"""The text of csrc/gmm_em.hip run on the CPU (-m "not gpu"): the file is compiled for the host against tests/gmm_host/common.h --
workgroups as threads on a barrier, the f64 MFMA and the xor shuffle emulated with the lane maps of DESIGN.md K6 -- into a
stand-alone program under the address and undefined-behaviour sanitizers, and its three entry points are compared with
tests/gmm_em64.py.  This checks the index arithmetic, the masking of partial tiles and row tails, the slice and workspace
layout and every bound of an array (at N = 16449 with more than one partial per thread in the mean's finalisation); it cannot check that the hardware's lane maps are the documented ones
(tests/test_gmm_em_gpu.py does).  Bounds as in the GPU test: 1e-10 of the reference's maximum, max(1e-10, 8 eps cond) for U."""
import os
import subprocess

import numpy as np
import pytest

import gmm_em64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from nnmnkwii_amd.csrc import build as hip_build
    d = tmp_path_factory.mktemp("gmm_host")
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "gmm_em.hip")).read()
    marker = "extern __shared__ double lds[];"
    assert src.count(marker) == 2
    (d / "gmm_em_host.inc").write_text(src.replace(marker, "double *lds = g_dyn_lds;"))
    for name in ("common.h", "main.cpp"):
        (d / name).write_text(open(os.path.join(ROOT, "tests", "gmm_host", name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "gmm_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.mark.parametrize("N,F,K", [(1, 1, 1), (17, 2, 3), (65, 16, 1), (70, 17, 3), (130, 33, 16), (67, 128, 2), (20, 5, 64), (16449, 1, 1)])
def test_kernel_text_on_the_host(program, N, F, K):
    d, exe = program
    rng = np.random.RandomState(N + F + K)
    scales = rng.permutation(np.linspace(0.5, 3.0, F))
    A = rng.randn(K, F, F) / np.sqrt(F)
    cov = (A @ A.transpose(0, 2, 1) + 0.5 * np.eye(F)) * np.outer(scales, scales)
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    means = 2.0 * rng.randn(K, F) / np.sqrt(F) * scales
    w = rng.dirichlet(np.full(K, 5.0))
    lab = rng.randint(K, size=N)
    X = means[lab] + np.einsum("nfg,ng->nf", np.linalg.cholesky(cov)[lab], rng.randn(N, F))
    resp_in = rng.dirichlet(np.full(K, 0.7), size=N)
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([N, F, K], dtype=np.int64).tobytes())
        f.write(np.array([1e-6]).tobytes())
        for a in (X, w, means, cov, resp_in):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.fromfile(d / "out.bin")
    pos = [0]

    def take(*shape):
        n = int(np.prod(shape))
        a = out[pos[0]:pos[0] + n].reshape(shape)
        pos[0] += n
        return a
    U, log_det, resp, lpn, mean = take(K, F, F), take(K), take(N, K), take(N), take(1)
    w2, mu2, cov2, status, labels = take(K), take(K, F), take(K, F, F), take(K), take(N)
    assert pos[0] == len(out)
    U_r, log_det_r = R.precisions(cov)
    resp_r, lpn_r, labels_r, mean_r = R.e_step(X, w, means, U_r, log_det_r)
    w_r, mu_r, cov_r = R.m_step(X, resp_in, 1e-6)
    assert not status.any() and np.array_equal(U, np.triu(U)) and np.array_equal(cov2, cov2.transpose(0, 2, 1))
    assert R.dist(U, U_r) <= max(1e-10, 8 * EPS * R.cond(cov))
    for name, got, ref in (("log_det", log_det, log_det_r), ("resp", resp, resp_r), ("log_prob_norm", lpn, lpn_r), ("mean", mean, mean_r),
                           ("weights", w2, w_r), ("means", mu2, mu_r), ("covariances", cov2, cov_r)):
        assert R.dist(got, ref) <= 1e-10, (name, R.dist(got, ref))
    top = np.sort(resp_r, axis=1)[:, ::-1]
    clear = np.ones(N, bool) if K == 1 else top[:, 0] - top[:, 1] > 1e-9
    assert (~clear).mean() <= 0.01 and np.array_equal(labels[clear], labels_r[clear])
