"""autograd.modspec_batch / autograd.modspec_mse_loss and the entry points under them against the float64 reference of
tests/modspec_batch64.py (numpy rfft / irfft per utterance, pinned on the CPU by tests/test_modspec_batch64_cpu.py).

Inputs: trajectories 0.1 * cumsum(randn) + rand, distinct lengths with len == Tmax, len < Tmax, len > n and len == 0, NaN in the
padding, eps = 1e-10.  Tolerances, relative to the reference array's maximum (tests/test_modspec_gpu.py's): float64 spectrum
1e-11, gradients 1e-10, loss 1e-11; float32 -- the reference evaluated in float64 on the same float32-rounded inputs --
spectrum and loss 2e-6, gradients 5e-6."""
import numpy as np
import pytest
import torch

import modspec_batch64 as R

pytestmark = pytest.mark.gpu

TOL = {torch.float64: dict(ms=1e-11, grad=1e-10, loss=1e-11), torch.float32: dict(ms=2e-6, grad=5e-6, loss=2e-6)}
NORMS = (None, "ortho")
FFT_N, DIRECT_N = (16, 256, 1024, 4096), (100, 1000, 2047, 5000)


def _close(a, b, rel, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / scale
    print("%s rel err %.3g (bound %.3g)" % (what, err, rel))
    assert err <= rel, (what, err)


def _counts():
    from nnmnkwii_amd import _hip
    return [_hip.lib().mlpg_hip_launch_count(k) for k in range(20)]


def _case(n, D, dtype, with_lengths, seed):
    """(x float64 rounded to dtype, lengths | None, Tmax): Tmax = n + 8 > n, so that len == Tmax is the len > n case too."""
    rng = np.random.RandomState(seed)
    T = n + 8
    lengths = [T, n // 2 + 1, 0, (3 * n) // 4] if with_lengths else None
    x = R.make_batch(rng, 4, T, D, lengths)
    if dtype == torch.float32:
        x = x.astype(np.float32).astype(np.float64)
    return x, lengths, T


def _round(a, dtype):
    return a.astype(np.float32).astype(np.float64) if dtype == torch.float32 else a


@pytest.mark.parametrize("with_lengths", [True, False], ids=["lengths", "full"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", FFT_N + DIRECT_N)
def test_spectrum_and_gradient_parity_and_routes(n, dtype, with_lengths):
    from nnmnkwii_amd import autograd as AF
    tol = TOL[dtype]
    for D in (5, 4):
        for norm in NORMS:
            x, lengths, T = _case(n, D, dtype, with_lengths, n + D)
            w = _round(np.random.RandomState(n).rand(4, n // 2 + 1, D), dtype)
            y = torch.from_numpy(x).to(dtype).cuda().requires_grad_()
            c0 = _counts()
            ms = AF.modspec_batch(y, n=n, norm=norm, lengths=lengths)
            assert ms.shape == (4, n // 2 + 1, D) and ms.dtype == dtype and ms.device == y.device
            (ms * torch.from_numpy(w).to(dtype).cuda()).sum().backward()
            c1 = _counts()
            moved = [k for k in range(20) if c1[k] != c0[k]]
            assert moved == ([17] if n in FFT_N else [18]) and c1[moved[0]] == c0[moved[0]] + 2, (moved, c0, c1)
            assert torch.isfinite(ms).all() and torch.isfinite(y.grad).all()
            _close(ms.detach().cpu().numpy(), R.modspec(x, n, norm, lengths), tol["ms"], "ms n=%d D=%d %s" % (n, D, norm))
            ref = R.modspec_grad(x, w, n, norm, lengths)
            g = y.grad.cpu().numpy()
            _close(g, ref, tol["grad"], "grad n=%d D=%d %s" % (n, D, norm))
            live = R.live_frames(lengths, 4, T, n)
            for b in range(4):
                assert not g[b, live[b]:].any()                # exactly 0.0 at and past min(len, n)


def test_nan_padding_cpu_tensors_2d_input_and_bad_arguments():
    from nnmnkwii_amd import autograd as AF
    n, D = 64, 3
    x, lengths, T = _case(n, D, torch.float64, True, 1)
    # a lengths tensor on the GPU, and CPU tensors staged through the GPU
    yc = torch.from_numpy(x).requires_grad_()
    ms = AF.modspec_batch(yc, n=n, lengths=torch.tensor(lengths).cuda())
    assert ms.device.type == "cpu" and ms.dtype == torch.float64 and torch.isfinite(ms).all()
    ms.sum().backward()
    assert yc.grad.device.type == "cpu" and torch.isfinite(yc.grad).all()
    _close(ms.detach().numpy(), R.modspec(x, n, None, lengths), 1e-11)
    _close(yc.grad.numpy(), R.modspec_grad(x, np.ones((4, n // 2 + 1, D)), n, None, lengths), 1e-10)
    # (T, D) in, (n//2+1, D) out
    y2 = torch.from_numpy(x[0]).cuda().requires_grad_()
    ms2 = AF.modspec_batch(y2, n=n, norm="ortho")
    assert ms2.shape == (n // 2 + 1, D)
    _close(ms2.detach().cpu().numpy(), R.modspec(x[:1], n, "ortho")[0], 1e-11)
    ms2.sum().backward()
    assert y2.grad.shape == y2.shape
    with pytest.raises(TypeError):
        AF.modspec_batch(torch.zeros(2, 8, 3, dtype=torch.float16, device="cuda"), n=16)
    with pytest.raises(TypeError):
        AF.modspec_mse_loss(torch.zeros(2, 8, 3, dtype=torch.int32, device="cuda"), torch.zeros(2, 9, 3, device="cuda"), n=16)
    with pytest.raises(ValueError):
        AF.modspec_batch(torch.zeros(2, 8, 3, device="cuda"), n=16, lengths=[9, 1])
    with pytest.raises(ValueError):
        AF.modspec_batch(torch.zeros(8, device="cuda"), n=16)


@pytest.mark.parametrize("n", [16, 12])
def test_gradcheck_with_lengths(n):
    from nnmnkwii_amd import autograd as AF
    gen = torch.Generator(device="cuda").manual_seed(3)
    y = torch.rand(3, 20, 3, dtype=torch.float64, device="cuda", generator=gen, requires_grad=True)   # 20 > n: the crop too
    for norm in NORMS:
        assert torch.autograd.gradcheck(lambda t: AF.ModSpecBatch.apply(t, n, norm, [20, 7, 0]), (y,), eps=1e-6, atol=1e-6)
        assert torch.autograd.gradcheck(lambda t: AF.modspec_mse_loss(t, torch.ones(3, n // 2 + 1, 3, dtype=torch.float64, device="cuda"),
                                                                      n=n, norm=norm, lengths=[20, 7, 0]), (y,), eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("T,n", [(40, 64), (100, 64), (70, 100), (300, 1024)])
def test_batch_equals_the_stack_of_the_2d_node(T, n):
    from nnmnkwii_amd import autograd as AF
    x = R.make_batch(np.random.RandomState(T), 3, T, 5)
    w = torch.from_numpy(np.random.RandomState(n).rand(3, n // 2 + 1, 5)).cuda()
    for norm in NORMS:
        yb = torch.from_numpy(x).cuda().requires_grad_()
        msb = AF.modspec_batch(yb, n=n, norm=norm)
        (msb * w).sum().backward()
        ys = [torch.from_numpy(x[b]).cuda().requires_grad_() for b in range(3)]
        mss = torch.stack([AF.modspec(y, n=n, norm=norm) for y in ys])
        (mss * w).sum().backward()
        _close(msb.detach().cpu().numpy(), mss.detach().cpu().numpy(), 1e-12)
        _close(yb.grad.cpu().numpy(), torch.stack([y.grad for y in ys]).cpu().numpy(), 1e-12)


def _loss_case(n, dtype, seed=0, D=5):
    x, lengths, T = _case(n, D, dtype, True, seed)
    tgt = R.modspec(R.make_batch(np.random.RandomState(seed + 1000), 4, T, D, lengths), n, None, lengths)
    return x, lengths, T, _round(tgt, dtype)


@pytest.mark.parametrize("log_domain", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [16, 256, 2048, 4096])
def test_loss_step_value_gradient_and_repeatability(n, dtype, log_domain):
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    tol = TOL[dtype]
    for D in (5, 4):
        for norm in NORMS:
            x, lengths, T, tgt = _loss_case(n, dtype, n, D)
            if norm == "ortho":
                tgt = _round(tgt / n, dtype)
            want, wgrad = R.loss_and_grad(x, tgt, n, norm, lengths, log_domain, 1e-10)
            y = torch.from_numpy(x).to(dtype).cuda().requires_grad_()
            tm = torch.from_numpy(tgt).to(dtype).cuda()
            assert _hip.modspec_loss_form(n) == 1
            c0 = _counts()
            loss = AF.modspec_mse_loss(y, tm, n=n, norm=norm, lengths=lengths, log_domain=log_domain, eps=1e-10)
            c1 = _counts()
            assert [k for k in range(20) if c1[k] != c0[k]] == [19] and c1[19] == c0[19] + 1
            assert loss.dim() == 0 and loss.dtype == dtype and loss.device == y.device
            loss.backward()
            assert torch.isfinite(y.grad).all()
            what = "n=%d D=%d %s log=%d" % (n, D, norm, log_domain)
            # the float64 value of the step itself, then the node's value in y.dtype
            l64, g = _hip.modspec_loss_step(y.detach(), tm, n, norm == "ortho", torch.tensor(lengths, dtype=torch.int32).cuda(),
                                            log_domain, 1e-10)
            _close(np.array([l64.item()]), np.array([want]), tol["loss"], "loss " + what)
            _close(np.array([loss.item()]), np.array([want]), tol["loss"], "loss(node) " + what)
            _close(y.grad.cpu().numpy(), wgrad, tol["grad"], "grad " + what)
            live = R.live_frames(lengths, 4, T, n)
            for b in range(4):
                assert not y.grad[b, live[b]:].any()
            # bitwise equal on a second call
            l2, g2 = _hip.modspec_loss_step(y.detach(), tm, n, norm == "ortho", torch.tensor(lengths, dtype=torch.int32).cuda(),
                                            log_domain, 1e-10)
            assert torch.equal(l64, l2) and torch.equal(g, g2) and torch.equal(g, y.grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_composed_route_agrees_with_the_fused_one(dtype):
    """Forced two ways: by a target that requires a gradient (same n, same data: against the fused node), and by a DFT length the
    fused step does not take (against the reference)."""
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    tol = TOL[dtype]
    n = 256
    for log_domain in (True, False):
        for norm in NORMS:
            x, lengths, T, tgt = _loss_case(n, dtype, 5)
            y1 = torch.from_numpy(x).to(dtype).cuda().requires_grad_()
            y2 = torch.from_numpy(x).to(dtype).cuda().requires_grad_()
            tm = torch.from_numpy(tgt).to(dtype).cuda()
            fused = AF.modspec_mse_loss(y1, tm, n=n, norm=norm, lengths=lengths, log_domain=log_domain)
            c0 = _counts()
            tm2 = tm.clone().requires_grad_()
            comp = AF.modspec_mse_loss(y2, tm2, n=n, norm=norm, lengths=lengths, log_domain=log_domain)
            fused.backward()
            comp.backward()
            c1 = _counts()
            assert c1[19] == c0[19] and c1[17] == c0[17] + 2       # the composed route: spectrum + gradient, no fused launch
            _close(np.array([comp.item()]), np.array([fused.item()]), tol["loss"])
            _close(y2.grad.cpu().numpy(), y1.grad.cpu().numpy(), tol["grad"])
            assert tm2.grad is not None and torch.isfinite(tm2.grad).all()
    for n in (100, 1000):
        assert _hip.modspec_loss_form(n) == 0
        x, lengths, T, tgt = _loss_case(n, dtype, 6)
        want, wgrad = R.loss_and_grad(x, tgt, n, None, lengths, True, 1e-10)
        y = torch.from_numpy(x).to(dtype).cuda().requires_grad_()
        c0 = _counts()
        loss = AF.modspec_mse_loss(y, torch.from_numpy(tgt).to(dtype).cuda(), n=n, lengths=lengths)
        loss.backward()
        c1 = _counts()
        assert c1[19] == c0[19] and c1[18] == c0[18] + 2
        assert loss.dim() == 0 and loss.dtype == dtype
        _close(np.array([loss.item()]), np.array([want]), tol["loss"])
        _close(y.grad.cpu().numpy(), wgrad, tol["grad"])
    # the direct-transform switch turns the fused form off for every n: the public function follows
    _hip.lib().mlpg_hip_modspec_set_direct(1)
    try:
        assert _hip.modspec_loss_form(256) == 0
        x, lengths, T, tgt = _loss_case(256, dtype, 5)
        y = torch.from_numpy(x).to(dtype).cuda().requires_grad_()
        c0 = _counts()
        AF.modspec_mse_loss(y, torch.from_numpy(tgt).to(dtype).cuda(), n=256, lengths=lengths).backward()
        c1 = _counts()
        assert c1[19] == c0[19] and c1[18] == c0[18] + 2 and c1[17] == c0[17]
        want, wgrad = R.loss_and_grad(x, tgt, 256, None, lengths, True, 1e-10)
        _close(y.grad.cpu().numpy(), wgrad, tol["grad"])
    finally:
        _hip.lib().mlpg_hip_modspec_set_direct(0)


def test_incoming_gradient_scales_and_side_streams():
    from nnmnkwii_amd import autograd as AF
    n = 256
    x, lengths, T, tgt = _loss_case(n, torch.float64, 9)
    tm = torch.from_numpy(tgt).cuda()
    y1 = torch.from_numpy(x).cuda().requires_grad_()
    y2 = torch.from_numpy(x).cuda().requires_grad_()
    AF.modspec_mse_loss(y1, tm, n=n, lengths=lengths).backward()
    (AF.modspec_mse_loss(y2, tm, n=n, lengths=lengths) * -2.5).backward()
    assert torch.equal(y2.grad, y1.grad * -2.5)
    # a side stream (its own workspace), CPU tensors, a 2-D input
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y3 = torch.from_numpy(x).cuda().requires_grad_()
        l3 = AF.modspec_mse_loss(y3, tm, n=n, lengths=lengths)
        l3.backward()
    s.synchronize()
    assert torch.equal(y3.grad, y1.grad)
    yc = torch.from_numpy(x[0, :100]).requires_grad_()
    lc = AF.modspec_mse_loss(yc, torch.from_numpy(tgt[0]), n=n, norm="ortho", log_domain=False)
    lc.backward()
    want, wgrad = R.loss_and_grad(x[:1, :100], tgt[:1], n, "ortho", None, False)
    assert lc.device.type == "cpu" and yc.grad.device.type == "cpu"
    _close(np.array([lc.item()]), np.array([want]), 1e-11)
    _close(yc.grad.numpy(), wgrad[0], 1e-10)


def test_full_size():
    """Config-2 sized batch, 256 x 1000 x 60, n = 4096, float32, lengths in [600, 1000]: parity on 4 utterances, Parseval on all
    (tests/test_modspec_gpu.py::test_full_size_properties), the loss step's gradient on the same 4."""
    from nnmnkwii_amd import autograd as AF
    B, T, D, n = 256, 1000, 60, 4096
    rng = np.random.RandomState(2)
    lengths = rng.randint(600, 1001, size=B)
    lengths[0], lengths[1] = 1000, 600
    x = R.make_batch(rng, B, T, D, lengths).astype(np.float32)
    y = torch.from_numpy(x).cuda().requires_grad_()
    L = torch.from_numpy(lengths.astype(np.int32)).cuda()
    ms = AF.modspec_batch(y, n=n, lengths=L)
    assert ms.shape == (B, n // 2 + 1, D) and ms.dtype == torch.float32 and torch.isfinite(ms).all()
    pick = [0, 1, 100, 255]
    x64 = x[pick].astype(np.float64)
    _close(ms[pick].detach().cpu().numpy(), R.modspec(x64, n, None, lengths[pick]), 2e-6, "full-size ms")
    # Parseval for a real signal: sum_{t < len} x^2 = (ms[0] + 2 sum_{0<k<n/2} ms[k] + ms[n/2]) / n
    live = (torch.arange(T, device="cuda")[None, :, None] < L[:, None, None])
    xx = torch.where(live, y.detach().double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    lhs = (xx * xx).sum(dim=1)
    m = ms.detach().double()
    rhs = (m[:, 0] + 2.0 * m[:, 1:n // 2].sum(dim=1) + m[:, n // 2]) / n
    assert torch.allclose(lhs, rhs, rtol=2e-6, atol=0)
    # the loss step on the whole batch; its gradient for utterance b depends on b's rows and n_elems alone
    tgt = R.make_batch(rng, B, T, D, lengths).astype(np.float32)
    tm = AF.modspec_batch(torch.from_numpy(tgt).cuda(), n=n, lengths=L).detach()
    loss = AF.modspec_mse_loss(y, tm, n=n, lengths=L)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(y.grad).all()
    _, wgrad = R.loss_and_grad(x64, tm[pick].cpu().numpy().astype(np.float64), n, None, lengths[pick], True, 1e-10,
                               n_elems=float(B * (n // 2 + 1) * D))
    _close(y.grad[pick].cpu().numpy(), wgrad, 5e-6, "full-size loss grad")
    for b in pick:
        assert not y.grad[b, lengths[b]:].any()
