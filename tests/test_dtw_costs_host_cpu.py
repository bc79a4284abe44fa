"""The texts of csrc/dtw_costs.hip and of the trim / gather kernels of csrc/dtw.hip run on the CPU (-m "not gpu"): compiled for
the host against the shim tests/gmm_host/common.h plus tests/dtw_costs_host/extras.h into a stand-alone program under the address
and undefined-behaviour sanitizers and run as a child process, once per launch.  The level walk of
``nnmnkwii_amd._hip.fastdtw_callable`` is restated here around the two launchers (windows from the coarser path, the local costs of
the window's cells evaluated in Python, the recurrence and the back-trace), and the paths are compared index for index -- the
distances to 1e-12, the figure of tests/test_dtw_costs_gpu.py -- with the literal restatement ``oracle.dtw.fastdtw_py``, the
reference that test uses.  One lane per pair walks raw offsets: every array is an exact-size heap block; the path entries past
path_len and the window rows past a pair's length hold INT32_MAX; the workspace from scratch() (cfirst / clast, the D rows, the
back-pointers) is a fresh exact-size block of 0xFF bytes (-1, NaN) in every launch, so a read of an entry the launch did not
write first shows in the path.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import dtw as OD  # noqa: E402

COST_BOUND = 1e-12
BIG = np.iinfo(np.int32).max
WORST = {"cost": 0.0, "pairs": 0}


def test_the_bound_is_the_gpu_tests():
    text = open(os.path.join(ROOT, "tests", "test_dtw_costs_gpu.py")).read()
    assert text.count("assert abs(cost[n] - d) <= %r * max(d, 1e-300)" % COST_BOUND) == 1


def build(d, edit=None):
    """The host program of the kernel texts in directory d; `edit` (file, old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    csrc = os.path.join(ROOT, "nnmnkwii_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("dtw_costs.hip", "dtw.hip")}
    assert all(t.count("extern __shared__") == 0 for t in text.values())
    if edit is not None:
        assert text[edit[0]].count(edit[1]) == 1, edit[1]
        text[edit[0]] = text[edit[0]].replace(edit[1], edit[2])
    os.makedirs(d / "csrc" / "x")
    for name in text:
        (d / "csrc" / "x" / name.replace(".hip", "_host.inc")).write_text(text[name])
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/dtw_costs_host", "extras.h"), ("tests/dtw_costs_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "dtw_costs_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-Wno-unused-function", "-I", str(d), str(d / "main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("dtw_costs_host"))


class Failed(Exception):
    pass


def call(program, head, arrays, eps=0.0):
    d, exe = program
    with open(d / "in.bin", "wb") as f:
        f.write(np.array(list(head) + [0] * (8 - len(head)), dtype=np.int64).tobytes())
        f.write(np.array([eps]).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    if r.returncode != 0:
        raise Failed(r.stderr[:1500] + " ... " + r.stderr[-1500:])        # (a sanitizer report names itself in its first line)
    return open(d / "out.bin", "rb").read()


def split(raw, *specs):
    out, at = [], 0
    for dtype, shape in specs:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out.append(np.frombuffer(raw[at:at + n], dtype=dtype).reshape(shape).copy())
        at += n
    assert at == len(raw)
    return out


def host_fastdtw(program, xs, ys, radius, dist, tie):
    """The level walk of _hip.fastdtw_callable around the host build: (path_i, path_j, path_len, cost)."""
    N, r = len(xs), int(radius)
    px, py, Kn = [], [], []
    for x, y in zip(xs, ys):
        lx, ly = [np.asarray(x, dtype=np.float64)], [np.asarray(y, dtype=np.float64)]
        while not (len(lx[-1]) < r + 2 or len(ly[-1]) < r + 2):
            for l in (lx, ly):
                a = l[-1]
                h = len(a) // 2
                l.append((a[0:2 * h:2] + a[1:2 * h:2]) / 2)
        px.append(lx)
        py.append(ly)
        Kn.append(len(lx) - 1)
    tx0 = np.array([len(l[0]) for l in px], dtype=np.int64)
    ty0 = np.array([len(l[0]) for l in py], dtype=np.int64)
    rs, max_ty, ps = int(tx0.max()), int(ty0.max()), int((tx0 + ty0).max())
    # what no launch has written yet holds INT32_MAX (the product's buffers start as zeros)
    path_i, path_j = np.full((N, ps), BIG, dtype=np.int32), np.full((N, ps), BIG, dtype=np.int32)
    path_len, cost = np.zeros(N, dtype=np.int32), np.zeros(N)
    row_lo, row_hi = np.full((N, rs), BIG, dtype=np.int32), np.full((N, rs), BIG, dtype=np.int32)
    row_off = np.full((N, rs + 1), np.iinfo(np.int64).max, dtype=np.int64)
    for k in range(max(Kn), -1, -1):
        ltx = np.array([(int(tx0[n]) >> k) if k <= Kn[n] else 0 for n in range(N)], dtype=np.int32)
        lty = np.array([(int(ty0[n]) >> k) if k <= Kn[n] else 0 for n in range(N)], dtype=np.int32)
        full = np.array([1 if k == Kn[n] else 0 for n in range(N)], dtype=np.int32)
        for n in range(N):                                       # the rows past this level's length: poison again
            row_lo[n, ltx[n]:] = row_hi[n, ltx[n]:] = BIG
        raw = call(program, [0, N, r, ps, rs], [ltx, lty, full, path_i, path_j, path_len, row_lo, row_hi, row_off])
        row_lo, row_hi, row_off = split(raw, (np.int32, (N, rs)), (np.int32, (N, rs)), (np.int64, (N, rs + 1)))
        ncell = np.array([int(row_off[n, ltx[n]]) if ltx[n] > 0 else 0 for n in range(N)], dtype=np.int64)
        base = np.concatenate([[0], np.cumsum(ncell)]).astype(np.int64)
        costs = np.empty(int(base[-1]))
        for n in range(N):
            q = int(base[n])
            for i in range(int(ltx[n])):
                assert 0 <= row_lo[n, i] <= row_hi[n, i] < lty[n], (k, n, i)
                for j in range(int(row_lo[n, i]), int(row_hi[n, i]) + 1):
                    costs[q] = dist(px[n][k][i], py[n][k][j])
                    q += 1
            assert q == base[n + 1]
        raw = call(program, [1, N, tie, ps, rs, max_ty, int(base[-1])],
                   [ltx, lty, row_lo, row_hi, row_off, costs, base[:N], path_i, path_j, path_len, cost])
        path_i, path_j, path_len, cost = split(raw, (np.int32, (N, ps)), (np.int32, (N, ps)), (np.int32, (N,)), (np.float64, (N,)))
        for n in range(N):                                       # nothing is written past the path
            assert (path_i[n, path_len[n]:] == BIG).all() and (path_j[n, path_len[n]:] == BIG).all()
    return path_i, path_j, path_len, cost


def sq(a, b):
    return float(np.sum((a - b) ** 2))


def verdict(got, pairs, radius, dist, tie):
    """None if every pair's path and distance are the reference's, else what is wrong."""
    pi, pj, pl, cost = got
    for n, (x, y) in enumerate(pairs):
        d, path = OD.fastdtw_py(x, y, radius, dist, tie)
        path = np.asarray(path)
        if pl[n] != len(path) or not (np.array_equal(pi[n, :pl[n]], path[:, 0]) and np.array_equal(pj[n, :pl[n]], path[:, 1])):
            return "pair %d: another path" % n
        e = abs(cost[n] - d) / max(d, 1e-300)
        WORST["cost"] = max(WORST["cost"], e / COST_BOUND)
        WORST["pairs"] += 1
        if e > COST_BOUND:
            return "pair %d: distance off by %.3e" % (n, e)
    return None


# (tx, ty): 1, 2, 3, odd and even, unequal, one pair long enough for three levels
SHAPES = [(1, 1), (1, 4), (2, 3), (3, 2), (3, 3), (7, 12), (12, 7), (9, 9), (16, 5), (5, 16), (23, 30)]


def make_pairs(seed, shapes, D=2, ties=False):
    rng = np.random.RandomState(seed)
    out = []
    for tx, ty in shapes:
        x, y = np.cumsum(rng.randn(tx, D), 0), np.cumsum(rng.randn(ty, D), 0)
        if ties:
            x, y = np.round(x), np.round(y)                     # quantised: equal candidates, the tie rule decides
        out.append((x, y))
    return out


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("tie", [0, 1])
def test_levels_on_the_host(program, radius, tie):
    """Every shape in one batch (pairs that have not started at the coarse levels next to pairs with the full window there),
    then the longest pair alone (N = 1); quantised data, where the tie rule decides."""
    pairs = make_pairs(10 * radius + tie, SHAPES, ties=True)
    got = host_fastdtw(program, [p[0] for p in pairs], [p[1] for p in pairs], radius, sq, tie)
    assert verdict(got, pairs, radius, sq, tie) is None
    one = make_pairs(radius, [(23, 30)])
    assert verdict(host_fastdtw(program, [one[0][0]], [one[0][1]], radius, sq, tie), one, radius, sq, tie) is None
    print("paths exact over %d pairs so far; worst distance error / bound %.3g" % (WORST["pairs"], WORST["cost"]))


def test_65_pairs_a_second_workgroup_with_one_live_lane(program):
    shapes = [SHAPES[n % len(SHAPES)] for n in range(65)]
    pairs = make_pairs(3, shapes)
    got = host_fastdtw(program, [p[0] for p in pairs], [p[1] for p in pairs], 1, OD.l2, 0)
    assert verdict(got, pairs, 1, OD.l2, 0) is None
    print("paths exact over %d pairs so far; worst distance error / bound %.3g" % (WORST["pairs"], WORST["cost"]))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_trim_on_the_host(program, dt):
    """All-silent and no-silent utterances, the last loud frame in every position of the first and second sweep of 64 frames."""
    for T in (1, 63, 64, 65, 130):
        rng = np.random.RandomState(T)
        lens = sorted({0, 1, T, T // 2, max(T - 64, 0), max(T - 65, 0), min(T, 64)})
        X = np.zeros((len(lens), T, 3), dtype=dt)
        for n, L in enumerate(lens):
            X[n, :L] = rng.randn(L, 3)
            X[n, :L][np.abs(X[n, :L]).sum(axis=1) < 1e-3] = 1.0
            X[n, L:] = 1e-9 * rng.rand(T - L, 3)                # below eps: silent
        raw = call(program, [2, len(lens), T, 3, dt == np.float64], [X, np.full(len(lens), -7, dtype=np.int32)], eps=1e-7)
        got = np.frombuffer(raw, dtype=np.int32)
        assert list(got) == lens == [len(OD.trim_zeros_frames(X[n].astype(np.float64), 1e-7)) for n in range(len(lens))], (T, got)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_gather_on_the_host(program, dt):
    """path_len 0, inside and at path_stride; Tout below, at and above path_len; the entries past path_len hold INT32_MAX."""
    rng = np.random.RandomState(1)
    N, Tsrc, ps, D = 4, 9, 12, 3
    src = rng.randn(N, Tsrc, D).astype(dt)
    pl = np.array([0, 5, ps, 1], dtype=np.int32)
    path = np.full((N, ps), BIG, dtype=np.int32)
    for n in range(N):
        path[n, :pl[n]] = np.sort(rng.randint(0, Tsrc, pl[n]))
    for Tout in (1, 5, ps, ps + 3, 90):                           # (90 x 3 elements: a second workgroup per utterance)
        raw = call(program, [3, N, Tsrc, ps, D, Tout, dt == np.float64], [src, path, pl, np.full((N, Tout, D), -7, dtype=dt)])
        got = np.frombuffer(raw, dtype=dt).reshape(N, Tout, D)
        want = np.zeros((N, Tout, D), dtype=dt)
        for n in range(N):
            k = min(pl[n], Tout)
            want[n, :k] = src[n, path[n, :k]]
        assert np.array_equal(got, want), Tout


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted_levels(tmp_path, edit):
    prog = build(tmp_path, edit)
    pairs = make_pairs(5, [(7, 12), (23, 30)])
    try:
        got = host_fastdtw(prog, [p[0] for p in pairs], [p[1] for p in pairs], 1, sq, 0)
    except Failed as e:
        assert "Sanitizer" in str(e) or "runtime error" in str(e), str(e)
        return "sanitizer"
    except AssertionError:
        return "mismatch"
    return verdict(got, pairs, 1, sq, 0)


def test_planted_read_one_path_entry_past_path_len(tmp_path):
    """The window kernel takes the coarse path's entry path_len: INT32_MAX as a row index."""
    assert planted_levels(tmp_path / "a", ("dtw_costs.hip", "for (int q = 0; q < pn; ++q) {", "for (int q = 0; q <= pn; ++q) {")) == "sanitizer"


def test_planted_workspace_without_its_last_back_pointer(tmp_path):
    """The scratch of the cost kernel one byte short of the last window cell's back-pointer (and without its 64 spare bytes)."""
    assert planted_levels(tmp_path / "a", ("dtw_costs.hip", "dbytes + (size_t)total_cells + 64);", "dbytes + (size_t)total_cells - 1);")) == "sanitizer"


def test_planted_d_row_read_that_nobody_wrote(tmp_path):
    """The row above is trusted one column past its window: a D entry that is still the scratch's 0xFF bytes (NaN) wins or loses
    every comparison, and the path is another."""
    got = planted_levels(tmp_path / "a", ("dtw_costs.hip", "up = (j >= plo && j <= phi) ? d0[j] : INF;", "up = (j >= plo && j <= phi + 1) ? d0[j] : INF;"))
    assert got is not None


def test_planted_gather_stores_one_element_past_the_batch(tmp_path):
    prog = build(tmp_path / "a", ("dtw.hip", "if (e >= (long)Tout * D) return;", "if (e > (long)Tout * D) return;"))
    with pytest.raises(Failed, match="AddressSanitizer"):
        call(prog, [3, 1, 2, 2, 3, 2, 1], [np.zeros((1, 2, 3)), np.zeros((1, 2), dtype=np.int32), np.array([2], dtype=np.int32), np.zeros((1, 2, 3))])
