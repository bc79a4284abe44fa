"""GPU tests (-m gpu) of nnmk_traj_nll and autograd.trajectory_nll (csrc/mlpg_trajcov.hip): the likelihood and both
gradients against tools/trajcov_model.py BIT FOR BIT given the device's own band and logdet (they are + - x / alone); the autograd
node against torch's float64 autograd of the dense expression; the reduction modes; the global-variance gradient as the sum of
the per-frame one; and paramgen.mlpg_variance against the reference's own composition for unit variances."""
import numpy as np
import pytest
import torch

import trajcov_cases as C
from trajcov_cases import TM

pytestmark = pytest.mark.gpu


def device_case(seed, B, Tmax, sd, wname, mode, dtype, lengths):
    """Inputs on the device, cbar from the library's own forward pass."""
    from nnmnkwii_amd import _hip
    win = C.WINDOWS[wname]
    D = len(win) * sd
    var = C.variances(seed, B, Tmax, sd, wname, mode, dtype)
    mean, target = C.features(seed + 1, B, Tmax, D, dtype), C.features(seed + 2, B, Tmax, sd, dtype)
    m, c = torch.from_numpy(mean).cuda(), torch.from_numpy(target).cuda()
    v = None if var is None else torch.from_numpy(var).cuda()
    L = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    cbar, status = _hip.forward(m, v, win, L)
    assert not status.any()
    return dict(win=win, var=var, mean=mean, target=target, m=m, c=c, v=v, L=L, cbar=cbar, lengths=lengths, B=B, Tmax=Tmax, sd=sd, D=D,
                mode=mode)


def check_against_model(k):
    from nnmnkwii_amd import _trajectory_calls as TC
    band, logdet, status = TC.covariance(k["v"], k["win"], k["L"], k["B"], k["Tmax"], k["D"], dtype=k["m"].dtype, device=k["m"].device)
    nll, gm, gv = TC.nll(k["m"], k["v"], k["win"], k["cbar"], k["c"], k["L"], band, logdet)
    torch.cuda.synchronize()
    want = TM.nll_batch(k["mean"], k["var"], k["win"], k["cbar"].cpu().numpy(), k["target"], k["lengths"], band.cpu().numpy(),
                        logdet.cpu().numpy())
    assert C.same_bits(nll.cpu().numpy(), want[0])
    assert C.same_bits(gm.cpu().numpy(), want[1])
    if k["mode"] == TM.VAR_UNIT:
        assert gv is None
    else:
        assert C.same_bits(gv.cpu().numpy(), want[2])
    # without the gradients: the same likelihood bits, no band needed
    alone = TC.nll(k["m"], k["v"], k["win"], k["cbar"], k["c"], k["L"], None, logdet, want_grad_means=False, want_grad_vars=False)
    assert alone[1] is None and alone[2] is None and C.same_bits(alone[0].cpu().numpy(), want[0])
    return nll, gm, gv


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sd", [1, 3, 60, 64, 65, 130])
def test_static_dims_across_lane_and_wavefront_boundaries(sd, dtype):
    for i, (wname, mode) in enumerate([("std3", TM.VAR_FRAME), ("std2", TM.VAR_GLOBAL), ("asym", TM.VAR_UNIT)]):
        check_against_model(device_case(sd + i, 3, 9, sd, wname, mode, dtype, [9, 0, 4]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 63, 64, 65])
def test_lengths_around_the_edge_rule_and_the_partition(T, dtype):
    for i, wname in enumerate(C.WINDOWS):
        mode = C.MODES[(i + T) % 3]
        check_against_model(device_case(T + i, 3, T, 3, wname, mode, dtype, [T, 0, max(T - 1, 0)]))
    check_against_model(device_case(T, 1, T, 2, "std3", TM.VAR_FRAME, dtype, None))


def dense_reference(mean, var, win, target, lengths, mode):
    """nll (B, sd) and the gradients by torch float64 autograd of the dense expression, utterance by utterance (CPU tensors)."""
    B, Tmax, D = mean.shape
    nw = len(win)
    sd = D // nw
    ws, _, mw = TM.window_set(win)
    m = torch.tensor(mean, dtype=torch.float64, requires_grad=True)
    v = None if var is None else torch.tensor(var, dtype=torch.float64, requires_grad=True)
    rows = []
    for b in range(B):
        T = int(lengths[b])
        edge = torch.ones((nw, T), dtype=torch.float64)
        for w in range(1, nw):
            for t in range(T):
                if mw == 0 or t < mw or t >= T - mw:
                    edge[w, t] = 0.0
        row = []
        for d in range(sd):
            cols = [w * sd + d for w in range(nw)]
            tau = edge.clone() if v is None else edge * ((1.0 / v[cols])[:, None] if mode == TM.VAR_GLOBAL else (1.0 / v[b, :T, cols]).T)
            row.append(TM.nll_dense(tau, m[b, :T, cols].T, ws, torch.tensor(target[b, :T, d], dtype=torch.float64)))
        rows.append(torch.stack(row))
    return torch.stack(rows), m, v


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_node_against_float64_autograd_of_the_dense_expression(mode, reduction):
    """B = 2, T = 17, sd = 3.  Tolerance: the model-against-truth bound c 2^-53 cond_2(R) max|.| with the measured c of
    tools/trajcov_model.py."""
    from nnmnkwii_amd import autograd
    B, Tmax, sd, lengths, win = 2, 17, 3, [17, 11], C.WINDOWS["std3"]
    var = C.variances(4, B, Tmax, sd, "std3", mode)
    mean, target = C.features(5, B, Tmax, 3 * sd), C.features(6, B, Tmax, sd)
    ref, m_ref, v_ref = dense_reference(mean, var, win, target, lengths, mode)
    weights = torch.tensor(np.random.RandomState(1).rand(B, sd))
    total = {"none": (ref * weights).sum(), "sum": ref.sum(), "mean": ref.sum() / (sum(lengths) * sd)}[reduction]
    total.backward()
    m = torch.tensor(mean, device="cuda", requires_grad=True)
    v = None if var is None else torch.tensor(var, device="cuda", requires_grad=True)
    out = autograd.trajectory_nll(m, v, win, torch.tensor(target, device="cuda"), lengths, reduction)
    (out * weights.cuda()).sum().backward() if reduction == "none" else out.backward()
    cond = max(C.cond2(TM.dense_definition(var if mode != TM.VAR_FRAME else var[b], win, lengths[b], sd)[0][d])
               for b in range(B) for d in range(sd))
    tol = TM.BOUND_C * C.EPS * cond
    want = {"none": ref, "sum": ref.sum(), "mean": ref.sum() / (sum(lengths) * sd)}[reduction].detach()
    assert out.shape == want.shape and out.dtype == torch.float64
    for name, got, exp in (("value", out.detach().cpu(), want), ("grad_means", m.grad.cpu(), m_ref.grad)) + \
            ((("grad_vars", v.grad.cpu(), v_ref.grad),) if v is not None else ()):
        err = float((got - exp).abs().max())
        print("%s: %.3g of the bound" % (name, err / (tol * max(1.0, float(exp.abs().max())))))
        assert err <= tol * max(1.0, float(exp.abs().max())), name
    if mode == TM.VAR_FRAME:
        assert (m.grad[1, 11:] == 0).all() and (v.grad[1, 11:] == 0).all() and (v.grad[0, [0, 16], sd:] == 0).all()
    # nothing requires a gradient: the same value, from the forward sweep alone (no band is made)
    from nnmnkwii_amd import _trajectory_hip as TH
    plain = autograd.trajectory_nll(m.detach(), None if v is None else v.detach(), win, torch.tensor(target, device="cuda"), lengths, reduction)
    assert torch.equal(plain, out.detach()) and TH.lib().nnmk_traj_launch_count() > 0


def test_global_variance_gradient_is_the_sum_of_the_per_frame_one():
    from nnmnkwii_amd import autograd
    B, Tmax, sd, lengths, win = 3, 9, 65, [9, 0, 5], C.WINDOWS["std3"]
    g = C.variances(2, 1, 1, sd, "std3", TM.VAR_GLOBAL)
    mean, target = torch.tensor(C.features(3, B, Tmax, 3 * sd), device="cuda"), torch.tensor(C.features(4, B, Tmax, sd), device="cuda")
    vg = torch.tensor(g, device="cuda", requires_grad=True)
    vf = torch.tensor(np.broadcast_to(g, (B, Tmax, 3 * sd)).copy(), device="cuda", requires_grad=True)
    a = autograd.trajectory_nll(mean, vg, win, target, lengths, "sum")
    b = autograd.trajectory_nll(mean, vf, win, target, lengths, "sum")
    a.backward()
    b.backward()
    assert torch.equal(a, b)
    s = vf.grad.sum(dim=(0, 1))
    assert float((vg.grad - s).abs().max()) <= 4 * B * Tmax * C.EPS * float(vf.grad.abs().sum(dim=(0, 1)).max())


def test_target_gradient_raises_and_two_dimensional_input():
    from nnmnkwii_amd import autograd
    win = C.WINDOWS["std2"]
    m = torch.tensor(C.features(1, 1, 8, 4)[0], device="cuda", requires_grad=True)
    v = torch.tensor(C.variances(2, 1, 8, 2, "std2", TM.VAR_FRAME)[0], device="cuda", requires_grad=True)
    c = torch.tensor(C.features(3, 1, 8, 2)[0], device="cuda")
    with pytest.raises(ValueError, match="out of scope"):
        autograd.trajectory_nll(m, v, win, c.clone().requires_grad_())
    out = autograd.trajectory_nll(m, v, win, c, reduction="none")
    out.sum().backward()
    both = autograd.trajectory_nll(m.detach()[None], v.detach()[None], win, c[None], reduction="none")
    assert out.shape == (2,) and torch.equal(out.detach(), both[0]) and m.grad.shape == (8, 4) and v.grad.shape == (8, 4)


def test_unit_variance_consistency_with_the_reference_composition():
    """The reference composes its MLPG matrix as R^-1 [W~_0' W~_1' ...] (float32), W~_w the window matrices with the edge rows of
    the dynamic ones zeroed: restricted to the static window -- its T columns times the static block of full_window_mat, the
    identity -- unit_variance_mlpg_matrix(windows, T) @ full_window_mat(...) is R^-1 itself.  Its diagonal is mlpg_variance for
    unit variances, at T = 9, within float32's rounding of that matrix (half a unit in its last place) plus the float64 error of
    the solve behind it (a few eps cond_2(R))."""
    from nnmnkwii_amd import paramgen
    T, win = 9, C.WINDOWS["std3"]
    M = paramgen.unit_variance_mlpg_matrix(win, T)                                 # (T, nw T) float32
    W = paramgen.full_window_mat(paramgen.build_win_mats(win, T), T)               # (nw T, T)
    assert M.dtype == np.float32 and np.array_equal(W[:T], np.eye(T))
    S = M[:, :T].astype(np.float64) @ W[:T]
    got = paramgen.mlpg_variance(np.ones((T, 3)), win)
    assert got.shape == (T, 1) and got.dtype == np.float64
    R = TM.dense_definition(None, win, T, 1)[0][0]
    tol = 2.0 ** -24 * np.abs(np.diag(S)) + TM.BOUND_C * C.EPS * C.cond2(R) * np.abs(S).max()
    assert (np.abs(got[:, 0] - np.diag(S)) <= tol).all()
    assert C.same_bits(got, TM.covariance(None, win, T, 1)[0][0])
