"""GPU tests (-m gpu) of include/nnmnkwii_sample.h (csrc/mlpg_trajsample.hip) against tools/trajsample_model.py: the
factor BIT FOR BIT (it is made of + - x / alone), logdet within trajcov_cases.logdet_bound, the draws and the whitened rows within
the K20 bound of the model's (float32: the model in float64 on the float32-rounded inputs, one float32 rounding on top) -- how many
of them are bit-equal is printed, not asserted --, NaN in every padded input row, a planted non-positive pivot, the same bits on a
repeated call, under a permutation of the batch, with more padding and for a draw alone, the round trip, the likelihood from the
whitened target, the paramgen layer and the counters.  Shapes: T around the ring of kTcAhead = 4, static dims around the lane group,
K around the draw group, B = 3 with lengths (Tmax, 0, 5), row strides above sd."""
import numpy as np
import pytest
import torch

import trajcov_cases as C
import trajsample_cases as S
from trajcov_cases import TM
from trajsample_cases import SM

pytestmark = pytest.mark.gpu
WNAMES = list(C.WINDOWS)


def group():
    from nnmnkwii_amd import _sample_hip
    return _sample_hip.draw_group()


def device_run(var, noise, mean, wname, lengths, slack=0):
    """factor, sample and whiten (of the draws, NaN planted in their rows at or past T) on the device: numpy (fac, logdet, status,
    out, z)."""
    from nnmnkwii_amd import _sample_calls as SC
    K, B, Tmax, sd = noise.shape
    win = C.WINDOWS[wname]
    L = S.dev_lengths(lengths)
    fac_out = None
    if slack:
        Q = TM.window_set(win)[1]
        fac_out = torch.full((Q + 1, B, Tmax, sd + slack), -7.0, dtype=torch.float64, device="cuda")[..., 1:1 + sd]
    fac, logdet, status = SC.factor(S.dev(var, slack), win, L, B, Tmax, len(win) * sd, dtype=torch.from_numpy(noise).dtype,
                                    device=torch.device("cuda", 0), factor=fac_out)
    m = S.dev(mean, slack)
    out = SC.sample(fac, status, L, S.dev(noise, slack), m)
    xin = out.clone()
    for b, T in enumerate(TM.live_frames(lengths, B, Tmax)):
        xin[:, b, int(T):] = float("nan")
    z = SC.whiten(fac, status, L, xin, m)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (fac, logdet, status, out, z))


def model64(var, noise, mean, wname, lengths):
    """The model in float64 on the inputs as given (float32 inputs are widened exactly; the reciprocals stay in their dtype)."""
    K, B, Tmax, sd = noise.shape
    fac, logdet, status = SM.factor_batch(var, C.WINDOWS[wname], lengths, B, Tmax, sd)
    m = None if mean is None else mean.astype(np.float64)
    out = SM.sample_batch(fac, status, lengths, noise.astype(np.float64), m)
    return fac, logdet, status, out, m


def check(seed, K, B, Tmax, sd, wname, mode, dtype, lengths, slack=0, has_mean=True, tight=False):
    var, noise, mean = S.inputs(seed, K, B, Tmax, sd, wname, mode, dtype, lengths, tight)
    mean = mean if has_mean else None
    fac, logdet, status, out, z = device_run(var, noise, mean, wname, lengths, slack)
    mfac, mlogdet, mstatus, mout, m64 = model64(var, noise, mean, wname, lengths)
    assert np.array_equal(status, mstatus) and not status.any()
    assert C.same_bits(fac, mfac), (wname, np.abs(fac - mfac).max())              # the live rows AND the zeros at or past T
    live = TM.live_frames(lengths, B, Tmax)
    for b in range(B):
        v = None if var is None else (var if var.ndim == 1 else var[b])
        assert (np.abs(logdet[b] - mlogdet[b]) <= C.logdet_bound(v, wname, int(live[b]), sd)).all()
    unit = S.units(var, wname, lengths, B, Tmax, sd)
    is_f32 = dtype == np.float32
    worst = S.within_bound(out, mout, unit, lengths, is_f32)
    # the whitened rows: the model on the device's own draws
    mz = SM.whiten_batch(mfac, mstatus, lengths, np.nan_to_num(out).astype(np.float64), None if m64 is None else np.nan_to_num(m64))
    worst_z = S.within_bound(z, mz, unit, lengths, is_f32)
    same = C.same_bits(out, SM.sample_batch(mfac, mstatus, lengths, noise, mean))
    print("%s T=%d sd=%d K=%d: draws %.3g, whitened %.3g of the bound; draws bit-equal to the model: %s" % (wname, Tmax, sd, K, worst, worst_z, same))
    assert not np.isnan(out).any() and not np.isnan(z).any() and not np.isnan(fac).any() and not np.isnan(logdet).any()
    return out, z


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [0, 1, 2, 3, 4, 5, 6, 9])
def test_lengths_around_the_ring_dims_around_the_lane_group(T, dtype):
    G = group()
    for i, sd in enumerate([1, 3, 64, 65]):
        K = (1, G, G + 1)[(i + T) % 3]
        check(T + sd, K, 3, T or 3, sd, WNAMES[(i + T) % 4], C.MODES[(i + T // 4) % 3], dtype, [T, 0, 5], slack=(i + T) % 2 * 3,
              has_mean=(i + T) % 5 != 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_window_set_and_variance_mode(dtype):
    G = group()
    for wname in WNAMES:
        for mode in C.MODES:
            check(7, G + 1, 3, 9, 3, wname, mode, dtype, [9, 0, 5], slack=2)
    check(3, 2, 1, 9, 3, "std3", TM.VAR_FRAME, dtype, None, tight=True)


def test_non_positive_pivot_sets_status_and_spares_the_neighbours():
    from nnmnkwii_amd import paramgen
    K, B, Tmax, sd, lengths = group() + 1, 2, 9, 3, [9, 6]
    var, noise, mean = S.inputs(5, K, B, Tmax, sd, "std3", TM.VAR_FRAME, np.float64, lengths)
    clean = device_run(var, noise, mean, "std3", lengths)
    var[0, 5, 1] = -1e-3
    fac, logdet, status, out, z = device_run(var, noise, mean, "std3", lengths)
    mfac, mlogdet, mstatus = SM.factor_batch(var, C.WINDOWS["std3"], lengths, B, Tmax, sd)
    assert np.array_equal(status, mstatus) and status[0, 1] == 6 and status.sum() == 6
    assert C.same_bits(fac, mfac) and np.isnan(logdet[0, 1])
    for got, ref in ((fac, clean[0]), (out, clean[3]), (z, clean[4])):
        assert np.isnan(got[:, 0, :, 1]).all()
        keep = np.ones(got.shape, dtype=bool)
        keep[:, 0, :, 1] = False
        assert C.same_bits(got[keep], ref[keep])                                  # every other system bit for bit, the pad rows zero
    means = np.zeros((B, Tmax, 3 * sd))
    with pytest.raises(np.linalg.LinAlgError, match=r"6-th leading minor not positive definite \(utterance 0, dim 1, frame 5\)"):
        paramgen.mlpg_sample_batch(means, np.nan_to_num(var, nan=1.0), C.WINDOWS["std3"], lengths)
    with pytest.raises(np.linalg.LinAlgError, match=r"utterance 0, dim 1, frame 5"):
        paramgen.mlpg_whiten_batch(np.zeros((B, Tmax, sd)), means, np.nan_to_num(var, nan=1.0), C.WINDOWS["std3"], lengths)


def test_same_bits_repeated_permuted_padded_and_alone():
    G = group()
    K, B, Tmax, sd, lengths = 2 * G + 1, 3, 17, 5, [17, 3, 9]
    var, noise, mean = S.inputs(2, K, B, Tmax, sd, "std3", TM.VAR_FRAME, np.float32, lengths)
    first = device_run(var, noise, mean, "std3", lengths)
    again = device_run(var, noise, mean, "std3", lengths)
    assert all(C.same_bits(a, b) for a, b in zip(first, again))
    perm = [2, 0, 1]
    p = device_run(np.ascontiguousarray(var[perm]), np.ascontiguousarray(noise[:, perm]), np.ascontiguousarray(mean[perm]), "std3",
                   [lengths[i] for i in perm])
    assert C.same_bits(p[0], np.ascontiguousarray(first[0][:, perm])) and C.same_bits(p[3], np.ascontiguousarray(first[3][:, perm]))
    assert C.same_bits(p[4], np.ascontiguousarray(first[4][:, perm]))
    # more padding: four more rows of NaN
    pad = lambda a, ax: np.concatenate([a, np.full(a.shape[:ax] + (4,) + a.shape[ax + 1:], np.nan, dtype=a.dtype)], axis=ax)  # noqa: E731
    w = device_run(pad(var, 1), pad(noise, 2), pad(mean, 1), "std3", lengths)
    for i in (0, 3, 4):
        assert C.same_bits(np.ascontiguousarray(w[i][:, :, :Tmax]), first[i]) and (w[i][:, :, Tmax:] == 0).all()
    # draw i of K against the same noise alone with K = 1: first, last of a group, first of the next, the one of the short group
    for i in (0, G - 1, G, 2 * G):
        alone = device_run(var, np.ascontiguousarray(noise[i:i + 1]), mean, "std3", lengths)
        assert C.same_bits(alone[3][0], first[3][i]) and C.same_bits(alone[4][0], first[4][i])


def test_round_trip_and_the_likelihood_from_the_whitened_target():
    from nnmnkwii_amd import _trajectory_calls as TC, paramgen
    K, B, Tmax, sd, lengths, wname = 3, 3, 9, 65, [9, 0, 5], "std3"
    win = C.WINDOWS[wname]
    var, noise, _ = S.inputs(4, K, B, Tmax, sd, wname, TM.VAR_FRAME, np.float64, lengths)
    var = np.nan_to_num(var, nan=1.0)
    means = np.nan_to_num(C.features(6, B, Tmax, 3 * sd))
    z0 = np.nan_to_num(noise)
    x = paramgen.mlpg_sample_batch(means, var, win, lengths, K, noise=z0)
    cbar = paramgen.mlpg_batch(means, var, win, lengths)
    back = paramgen.mlpg_whiten_batch(x, means, var, win, lengths)
    unit = S.units(var, wname, lengths, B, Tmax, sd)
    live = TM.live_frames(lengths, B, Tmax)
    for b, T in enumerate(live):
        z0[:, b, T:] = 0
    # twice the bound: one application for the draw, one for the inverse map (|z| is of order 1)
    err = np.abs(back - z0)
    assert (err <= 2 * SM.BOUND_C * unit[None, :, None, :] * max(1.0, np.abs(z0).max())).all(), err.max()
    # 1/2 sum z^2 - 1/2 logdet + T/2 log 2 pi for z = whiten(target) against nnmk_traj_nll
    target = x[0]
    zt = paramgen.mlpg_whiten_batch(target, means, var, win, lengths, cbar=cbar)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    L = S.dev_lengths(lengths)
    _, logdet, _ = TC.covariance(d(var), win, L, B, Tmax, 3 * sd, want_band=False)
    nll, _, _ = TC.nll(d(means), d(var), win, d(cbar), d(target), L, None, logdet, want_grad_means=False, want_grad_vars=False)
    quad = 0.5 * (zt * zt).sum(axis=1)
    mine = quad - 0.5 * logdet.cpu().numpy() + 0.5 * live[:, None] * TM.LOG_2PI
    ref = nll.cpu().numpy()
    assert (np.abs(mine - ref) <= 4 * SM.BOUND_C * unit * np.maximum(1.0, np.maximum(quad, np.abs(ref)))).all(), np.abs(mine - ref).max()


def test_paramgen_interfaces_generator_and_detached_results():
    from nnmnkwii_amd import paramgen
    win = C.WINDOWS["std3"]
    T, sd, K = 9, 3, 3
    rng = np.random.RandomState(1)
    mean_frames, var_frames = rng.randn(T, 3 * sd).astype(np.float32), (0.5 + rng.rand(T, 3 * sd)).astype(np.float32)
    noise = rng.randn(K, T, sd).astype(np.float32)
    one = paramgen.mlpg_sample(mean_frames, var_frames, win, K, noise=noise)
    batch = paramgen.mlpg_sample_batch(mean_frames[None], var_frames[None], win, None, K, noise=noise[:, None])
    assert one.shape == (K, T, sd) and one.dtype == np.float32 and C.same_bits(one, np.ascontiguousarray(batch[:, 0]))
    # against the model, with the mean trajectory handed in (which kernel gives cbar is the forward routes' business)
    fac, _, status = SM.factor_batch(var_frames[None], win, None, 1, T, sd)
    cbar = paramgen.mlpg_batch(mean_frames[None], var_frames[None], win)
    given = paramgen.mlpg_sample_batch(mean_frames[None], var_frames[None], win, None, K, noise=noise[:, None], cbar=cbar)
    want = SM.sample_batch(fac, status, None, noise[:, None].astype(np.float64), cbar.astype(np.float64))
    S.within_bound(given, want, S.units(var_frames[None], "std3", None, 1, T, sd), None, True)
    assert np.allclose(batch, given, rtol=1e-5, atol=1e-5)
    # global variances
    g = paramgen.mlpg_sample(mean_frames, var_frames[0], win, 2, noise=noise[:2])
    assert g.shape == (2, T, sd) and np.isfinite(g).all()
    # tensors: the generator path is reproducible, a different seed differs, gradients are not tracked
    m = torch.from_numpy(mean_frames[None]).cuda().requires_grad_()
    v = torch.from_numpy(var_frames[None]).cuda().requires_grad_()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    a, ld = paramgen.mlpg_sample_batch(m, v, win, None, K, generator=gen, return_logdet=True)
    gen.manual_seed(7)
    b = paramgen.mlpg_sample_batch(m, v, win, None, K, generator=gen)
    gen.manual_seed(8)
    c = paramgen.mlpg_sample_batch(m, v, win, None, K, generator=gen)
    assert a.is_cuda and a.shape == (K, 1, T, sd) and a.dtype == torch.float32 and not a.requires_grad and torch.equal(a, b) and not torch.equal(a, c)
    assert ld.shape == (1, sd) and ld.dtype == torch.float64
    w = paramgen.mlpg_whiten_batch(a, m, v, win)
    assert w.is_cuda and not w.requires_grad and w.shape == a.shape
    out = torch.full((K, 1, T, sd), -7.0, dtype=torch.float32, device="cuda")
    gen.manual_seed(7)
    assert paramgen.mlpg_sample_batch(m, v, win, None, K, generator=gen, out=out) is out and torch.equal(out, a)
    assert paramgen.mlpg_sample_batch(m, v, win, None, 0).shape == (0, 1, T, sd)


def test_one_launch_per_entry_and_refusals_launch_nothing():
    from nnmnkwii_amd import _hip, _sample_calls as SC, _sample_hip as SH, _trajectory_hip as TH
    L, LT = SH.lib(), TH.lib()
    win = C.WINDOWS["std3"]
    var = torch.from_numpy(C.variances(1, 2, 9, 3, "std3", TM.VAR_FRAME)).cuda()
    noise = torch.randn((2, 2, 9, 3), dtype=torch.float64, device="cuda")
    n0, t0 = L.nnmk_draw_launch_count(), LT.nnmk_traj_launch_count()
    fac, logdet, status = SC.factor(var, win, None, 2, 9, 9)
    assert L.nnmk_draw_launch_count() == n0 + 1
    out = torch.full((2, 2, 9, 3), -7.0, dtype=torch.float64, device="cuda")
    SC.sample(fac, status, None, noise, None, out=out)
    assert L.nnmk_draw_launch_count() == n0 + 2
    SC.whiten(fac, status, None, out, None)
    assert L.nnmk_draw_launch_count() == n0 + 3 and LT.nnmk_traj_launch_count() == t0
    keep = out.clone()
    wide = [(0, 0, np.array([1.0])), (2, 2, np.array([1.0, -8.0, 0.0, 8.0, -1.0]) / 12)]
    with pytest.raises(_hip.HipExtensionError, match="extents"):
        SC.factor(var[:, :, :6], wide, None, 2, 9, 6, factor=torch.full((5, 2, 9, 3), -7.0, dtype=torch.float64, device="cuda"))
    with pytest.raises(_hip.HipExtensionError, match="overlap"):
        SC.factor(var, win, None, 2, 9, 9, factor=var.view(-1)[:162].view(3, 2, 9, 3))
    with pytest.raises(_hip.HipExtensionError, match="overlaps the factor"):
        SC.sample(fac, status, None, noise[:1], None, out=fac[:1])
    with pytest.raises(_hip.HipExtensionError, match="overlaps x"):
        SC.whiten(fac, status, None, out, None, out=out)
    with pytest.raises(ValueError):
        SC.sample(fac, status, None, noise, None, out=out[:1])
    torch.cuda.synchronize()
    assert L.nnmk_draw_launch_count() == n0 + 3 and torch.equal(out, keep)
