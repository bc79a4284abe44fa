"""The strip kernel's standard-window instantiations (strip_kernel<..., STD>, csrc/mlpg_strip_impl.h) against the general ones.

Every coefficient of the standard set -- [1], [-0.5, 0, 0.5], [1, -2, 1] -- and every product of two of them is 0, +-1 or a
power of two.  A product with such a value is exact, an fma with it rounds like the add it becomes, and a dropped zero term
would have added +-0: the STD kernels must return the general kernels' arrays, equal as numbers (torch.equal: a -0 for a
+0 is no difference, anything else is).  MLPG_STRIP_STDWIN is read once per process, so each side runs in a child of its own
(tests/strip_stdwin_worker.py) that dumps outputs and status."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(out_path, stdwin):
    env = dict(os.environ)
    env.pop("MLPG_STRIP_STDWIN", None)
    if stdwin is not None:
        env["MLPG_STRIP_STDWIN"] = stdwin
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(HERE, "strip_stdwin_worker.py"), out_path]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out_path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("stdwin")
    on = _child(str(d / "on.npz"), None)
    off = _child(str(d / "off.npz"), "0")
    assert sorted(on) == sorted(off)
    return on, off


def _keys(dumps, case):
    return [k for k in sorted(dumps[0]) if k.startswith(case + "/")]


@pytest.mark.parametrize("case", ["c2", "ragged", "tight"])
def test_std_kernels_equal_general_kernels(dumps, case):
    """Config-2 slice (32 utterances); ragged lengths (Tmax = 300, T from 300 down to 1: both EDGE copies, strips of padding);
    dynamic variances 100 x / 1000 x tighter (the other rungs of level 3) -- forward and backward, float32 and float64 inputs,
    float32 and float64 gradients."""
    import torch
    on, off = dumps
    keys = _keys(dumps, case)
    assert len(keys) == 2 * 6  # two input dtypes x (forward + two gradients) x (values, status)
    for k in keys:
        a, b = torch.from_numpy(on[k]), torch.from_numpy(off[k])
        assert a.dtype == b.dtype and torch.equal(a, b), (k, float((a.double() - b.double()).abs().max()))
        if k.endswith("_status"):
            assert int(a.abs().max()) == 0, k
        else:
            assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, k


def test_std_kernels_fail_like_general_kernels(dumps):
    """Variances that are negative, 0, -0, Inf, -Inf or NaN, scattered over a launch (see failure_case): the same status words and the
    same zero columns from both builds -- every lane the general kernel marks (also through the 0 * Inf = NaN of a zero term) is
    marked by the STD kernel (pivot test on the refined reciprocal) -- and the other columns equal as numbers."""
    import torch
    on, off = dumps
    keys = _keys(dumps, "fail")
    assert len(keys) == 12
    for k in keys:
        a, b = torch.from_numpy(on[k]), torch.from_numpy(off[k])
        assert torch.equal(a, b), k
    for dt in ("float64", "float32"):
        st = on["fail/%s/fwd_status" % dt].reshape(32, -1)
        assert (st != 0).sum() >= 50, dt                      # the failures were met
        y = on["fail/%s/fwd" % dt]
        assert np.isfinite(y).all()
        assert not (y != 0)[np.broadcast_to((st != 0)[:, None, :], y.shape)].any()
        assert (np.abs(y).max(axis=1) > 0)[st == 0].all()     # ... and only they were zeroed
        for od in ("float64", "float32"):
            g = on["fail/%s/bwd_%s" % (dt, od)].reshape(32, 1000, 3, -1)
            sb = on["fail/%s/bwd_%s_status" % (dt, od)].reshape(32, -1)
            assert np.isfinite(g).all()
            assert not (g != 0)[np.broadcast_to((sb != 0)[:, None, None, :], g.shape)].any()


@pytest.mark.parametrize("wname", ["near_half", "scaled", "reordered"])
def test_near_standard_windows_take_the_general_kernel(dumps, wname):
    """-0.5000001 for -0.5, a delta window scaled by 2, delta-delta before delta: not the standard set, so the general kernel runs
    -- the result matches the oracle for THOSE windows to 1e-9 (the standard set's result is 1e-7 or more away) -- with the
    switch on or off, bit for bit."""
    import torch
    on, off = dumps
    for d in (on, off):
        assert float(d["near_%s/oracle_err" % wname]) < 1e-9
        assert float(d["near_%s/distance_to_std" % wname]) > 1e-8
    for k in _keys(dumps, "near_" + wname):
        a, b = on[k], off[k]
        assert a.tobytes() == b.tobytes() or k.endswith(("oracle_err", "distance_to_std")), k


def test_std_launches_count_as_strip_launches(dumps):
    """Routing as before: a launch of the STD instantiation is a strip-kernel launch (mlpg_hip_launch_count(2)): three per case
    and dtype (forward, two gradients), switch on or off."""
    on, off = dumps
    keys = [k for k in on if k.startswith("count/")]
    assert len(keys) == 4 * 2 + 3
    for k in keys:
        assert int(on[k]) == 3 and int(off[k]) == 3, k
