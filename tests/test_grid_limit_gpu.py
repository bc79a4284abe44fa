"""GPU tests (-m gpu): every entry whose launch is one workgroup (or a fixed number of them) per batch item, on a batch a few items
over what ONE grid takes.  A grid is 32 bits of threads: workgroups * threads per workgroup < 2^32, and a larger launch runs the
threads that remain modulo 2^32 and reports nothing (profiles/grid_limit_notes.md).  So the limit is 2^22 - 1 workgroups of 1024
threads, 2^23 - 1 of 512, 2^24 - 1 of 256 and 2^26 - 1 of 64, and the batches here are `limit + 3` to `limit + 8` items of the
smallest shape the entry takes (T 1 or 2, n = 2 or 3, D 1 or 2): 64 MiB to 1 GiB per array.

Entries with lengths: all items are dead (length 0, NaN in the inputs, the byte 0xA5 in the outputs) except five -- item 0, the last
item a truncated launch would still run, the first it would not, item `limit - 1` and the last item of the batch.  Asserted: return
code 0; the live items' outputs equal, bit for bit, the same entry on the compact batch of the five; the compact result meets the
entry's own bound against its own float64 reference (both imported from the entry's GPU test file); a dead item's output is what the
header promises, checked whole on the device; the launch counter moved as for a small call.  Entries without lengths: every item is
live and the whole output is compared on the device with a closed form in torch float64.  A loss, which reduces over the batch, is
held to the entry's bound against the float64 reference of the live items.

Where an entry refuses such a batch instead (the fused training step, the FIR form by name), the test asserts MLPG_HIP_EINVAL, a
message that names the limit, no counter moved and no output byte changed, and that the call AT the limit returns 0 and is right.

The last test prints the table entry -> workgroups asked, limit, outcome and fails unless every row is there."""
import collections

import numpy as np
import pytest
import torch

import modspec_batch64 as R64
from cases import WINDOW_SETS
from test_far_batch_gpu import counts, lib_call, moved, win_args
from test_far_rows_gpu import far_test

pytestmark = pytest.mark.gpu

F32, F64 = 0, 1                                       # MLPG_HIP_F32, MLPG_HIP_F64
EINVAL = -1
TDT = {F32: torch.float32, F64: torch.float64}
NDT = {F32: np.float32, F64: np.float64}
POISON = 0xA5
LIMIT = {1024: (1 << 22) - 1, 512: (1 << 23) - 1, 256: (1 << 24) - 1, 64: (1 << 26) - 1}   # workgroups one launch takes
TABLE = collections.OrderedDict()                     # row -> (workgroups asked, limit, outcome)
ROWS = ("modspec_batch", "modspec_batch_backward", "modspec_loss_step", "modspec_filter", "modspec (fft)", "inv_modspec (fft)",
        "modspec_smoothing (fft)", "modspec_backward (fft)", "modspec (chirp-z)", "inv_modspec (chirp-z)", "modspec_smoothing (chirp-z)",
        "modspec_backward (chirp-z)", "forward (wave)", "backward (wave)", "forward (auto)", "backward (auto)",
        "unit_mse_step (fused wave)", "forward (fir)", "backward (auto, fir shape)", "unit_mse_step (fir shape)", "trim_lengths",
        "gather_path", "fastdtw")


def row(name, asked, threads, outcome):
    assert name in ROWS and asked > LIMIT[threads], (name, asked)
    TABLE[name] = (asked, LIMIT[threads], outcome)


def five(B, still_run, limit_items):
    """Item 0, the last a truncated launch still runs, the first it does not, item limit - 1, the last of the batch."""
    idx = [0, still_run - 1, still_run, limit_items - 1, B - 1]
    assert sorted(set(idx)) == idx and limit_items < B
    return torch.tensor(idx, dtype=torch.int64, device="cuda")


def poison(shape, dtype):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), POISON, dtype=torch.uint8, device="cuda").view(dtype).view(*shape)


def nans(shape, dtype):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def lengths_for(B, idx, lens):
    L = torch.zeros(B, dtype=torch.int32, device="cuda")
    L[idx] = dev(np.asarray(lens, dtype=np.int32))
    return L


def put(full, idx, live):
    full[idx] = dev(live).to(full.dtype)
    return full


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def rest_is(out, idx, byte):
    """Every byte of `out` outside the items idx is `byte` (on the device; the live items are put back after)."""
    rows = out.view(out.shape[0], -1)
    saved = rows[idx].clone()
    rows[idx] = poison(saved.shape, out.dtype) if byte == POISON else torch.zeros_like(saved)
    ok = bool((out.view(-1).view(torch.uint8) == byte).all())
    rows[idx] = saved
    return ok


def close(got, ref, rel, what):
    got, ref = np.asarray(got.cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert err <= rel, (what, err)


# ---------------------------------------------------------------------------------------------------- modulation spectrum, padded

MS_B = (1 << 22) + 3                                  # ceil(D / 2) = 1 workgroup of 1024 threads per utterance: 3 over


@far_test
def test_modspec_batch_backward_and_loss_step():
    """float32, B = 2^22 + 3, Tmax = n = 2, D = 2: 64 MiB per array.  A truncated launch runs utterances 0, 1 and 2."""
    from test_modspec_batch_gpu import TOL
    tol = TOL[torch.float32]
    L, di, stream = lib_call()
    B, Tm, n, D, nb, ortho, norm = MS_B, 2, 2, 2, 2, 1, "ortho"
    idx = five(B, 3, LIMIT[1024])
    lens = np.array([2, 1, 2, 2, 1], dtype=np.int32)
    rng = np.random.RandomState(3)
    X = R64.make_batch(rng, 5, Tm, D, lens).astype(np.float32)                      # NaN from each length on
    Gm = rng.rand(5, nb, D).astype(np.float32)
    Tg = (R64.modspec(R64.make_batch(rng, 5, Tm, D, lens, pad=0.0), n, None, lens) + 0.01).astype(np.float32)
    X64, Gm64, Tg64 = X.astype(np.float64), Gm.astype(np.float64), Tg.astype(np.float64)
    x, Ld = put(nans((B, Tm, D), torch.float32), idx, X), lengths_for(B, idx, lens)
    xc, Lc = dev(X), dev(lens)

    def both(entry, kind, call):
        """The entry on the large batch and on the compact one; (large output, compact output)."""
        outs = []
        for big in (True, False):
            c0 = counts()
            rc, out = call(big)
            torch.cuda.synchronize()
            assert rc == 0 and moved(c0) == {kind: 1}, (entry, big, rc, L.mlpg_hip_last_error(), moved(c0))
            outs.append(out)
        return outs

    # the spectrum; a dead utterance's is that of no frames: zeros
    def spec(big):
        out = poison((B if big else 5, nb, D), torch.float32)
        a, l = (x, Ld) if big else (xc, Lc)
        return L.mlpg_hip_modspec_batch(di, stream, F32, a.data_ptr(), l.data_ptr(), out.shape[0], Tm, D, n, ortho, out.data_ptr()), out
    ms, msc = both("modspec_batch", 17, spec)
    close(msc, R64.modspec(X64, n, norm, lens), tol["ms"], "ms")
    assert same_bits(ms[idx], msc), "modspec_batch: a live utterance differs from the compact batch"
    assert rest_is(ms, idx, 0), "modspec_batch: a dead utterance's spectrum is not zero"
    row("modspec_batch", B, 1024, "complete")
    del ms

    # the gradient (NaN in the dead utterances' grad_ms: their grad_x is zero whatever it holds)
    gms, gmc = put(nans((B, nb, D), torch.float32), idx, Gm), dev(Gm)

    def back(big):
        out = poison((B if big else 5, Tm, D), torch.float32)
        a, g, l = (x, gms, Ld) if big else (xc, gmc, Lc)
        return L.mlpg_hip_modspec_batch_backward(di, stream, F32, a.data_ptr(), g.data_ptr(), l.data_ptr(), out.shape[0], Tm, D, n, ortho,
                                                 out.data_ptr()), out
    gx, gxc = both("modspec_batch_backward", 17, back)
    got = gxc.cpu().numpy()
    assert all(not got[i, lens[i]:].any() for i in range(5))
    close(got, R64.modspec_grad(X64, Gm64, n, norm, lens), tol["grad"], "grad")
    assert same_bits(gx[idx], gxc), "modspec_batch_backward: a live utterance differs from the compact batch"
    assert rest_is(gx, idx, 0), "modspec_batch_backward: a dead utterance's gradient is not zero"
    row("modspec_batch_backward", B, 1024, "complete")
    del gx, gms

    # the fused loss step.  A dead utterance has the spectrum 0 and the target 0: f(0) - f(0) adds nothing in either domain, so
    # the float64 loss of the five live utterances is the whole loss; it reduces over the batch and is held to the entry's bound.
    tg, tgc = put(torch.zeros((B, nb, D), dtype=torch.float32, device="cuda"), idx, Tg), dev(Tg)
    n_elems = float(5 * nb * D)
    for log_domain in (1, 0):
        losses = []

        def step(big):
            nB = B if big else 5
            out = poison((nB, Tm, D), torch.float32)
            ws_bytes = int(L.mlpg_hip_modspec_loss_workspace_bytes(nB, D))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            loss = nans((1,), torch.float64)
            losses.append(loss)
            a, t, l = (x, tg, Ld) if big else (xc, tgc, Lc)
            return L.mlpg_hip_modspec_loss_step(di, stream, F32, a.data_ptr(), t.data_ptr(), l.data_ptr(), nB, Tm, D, n, ortho, log_domain,
                                                1e-10, n_elems, out.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws_bytes), out
        gx, gxc = both("modspec_loss_step", 19, step)
        want, wgrad = R64.loss_and_grad(X64, Tg64, n, norm, lens, bool(log_domain), 1e-10, n_elems)
        print("modspec_loss_step log_domain=%d: loss %.17g (large) %.17g (compact) %.17g (float64)" % (log_domain, float(losses[0][0]), float(losses[1][0]), want))
        close(losses[1], [want], tol["loss"], "loss, compact")
        close(losses[0], [want], tol["loss"], "loss, large batch")
        close(gxc, wgrad, tol["grad"], "loss grad")
        assert same_bits(gx[idx], gxc), "modspec_loss_step: a live utterance differs from the compact batch"
        assert rest_is(gx, idx, 0), "modspec_loss_step: a dead utterance's gradient is not zero"
        del gx
    row("modspec_loss_step", B, 1024, "complete")


@far_test
def test_modspec_filter():
    """float32, B = 2^22 + 3, Tmax = n = 2, D = 2, both tables and bin 1 removed in the log domain."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import msfilter_model as MM
    from test_msfilter_gpu import BOUND, _tables
    L, di, stream = lib_call()
    B, Tm, n, D, nb = MS_B, 2, 2, 2, 2
    idx = five(B, 3, LIMIT[1024])
    lens = [2, 1, 2, 2, 1]
    rng = np.random.RandomState(4)
    X = R64.make_batch(rng, 5, Tm, D, lens).astype(np.float32)
    A, C = _tables(rng, nb, D)
    Ad, Cd = dev(A), dev(C)
    x, Ld = put(nans((B, Tm, D), torch.float32), idx, X), lengths_for(B, idx, lens)
    outs = []
    for a, l in ((x, Ld), (dev(X), dev(np.asarray(lens, dtype=np.int32)))):
        out = poison(a.shape, torch.float32)
        c0 = counts()
        rc = L.mlpg_hip_modspec_filter(di, stream, F32, a.data_ptr(), D, l.data_ptr(), a.shape[0], Tm, D, n, 1, Ad.data_ptr(), Cd.data_ptr(), 1, 1,
                                       out.data_ptr(), D)
        torch.cuda.synchronize()
        assert rc == 0 and moved(c0) == {31: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
        outs.append(out)
    big, compact = outs
    got = compact.cpu().numpy()
    assert all(not got[i, lens[i]:].any() for i in range(5))
    close(got, MM.filter_batch(X, n, "ortho", lens, A, C, 1, True), BOUND[np.float32], "filtered")
    assert same_bits(big[idx], compact), "modspec_filter: a live utterance differs from the compact batch"
    assert rest_is(big, idx, 0), "modspec_filter: a dead utterance's rows are not zero"
    row("modspec_filter", B, 1024, "complete")


# ---------------------------------------------------------------------------------------------------- modulation spectrum, plain

def _two_point(x, ortho):
    """(s0, s1) of the 2-point DFT of (x0, x1), scaled as the entry scales: times 1 / sqrt(2) with "ortho"."""
    a = 2.0 ** -0.5 if ortho else 1.0
    return (x[:, 0] + x[:, 1]) * a, (x[:, 0] - x[:, 1]) * a


def _all_close(got, want, rel, what):
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= rel, (what, err)


@pytest.mark.parametrize("ortho", [0, 1])
@far_test
def test_modspec_entries_without_lengths_fft_route(ortho):
    """float64, B = 2^22 + 3, T = n = 2, D = 2: every sequence is live, every output element is compared on the device with the
    closed form at n = 2 -- s0 = x0 + x1, s1 = x0 - x1 (times 1 / sqrt(2) with "ortho"), power s^2, phase sign(s); the inverse
    (s0 +- s1) * (1 / 2 | 1 / sqrt(2)); smoothing with bin 1 removed: both frames (x0 + x1) / 2; the gradient
    (g0 s0 +- g1 s1) * (2 | 2 / sqrt(2)).  Bounds, of the largest value: those of tests/test_modspec_gpu.py -- power and inverse 1e-12,
    phase and smoothing 1e-11, gradient 1e-10."""
    L, di, stream = lib_call()
    B, T, n, D, nb = MS_B, 2, 2, 2, 2
    assert L.mlpg_hip_modspec_route(n) == 0
    g = torch.Generator(device="cuda").manual_seed(5 + ortho)
    x = torch.rand((B, T, D), dtype=torch.float64, device="cuda", generator=g) + 0.5
    x[:, 1] *= 0.25 - 1.25 * (torch.rand((B, D), dtype=torch.float64, device="cuda", generator=g) < 0.5).double()   # times -1 or 1 / 4: s0 and s1 of either sign
    s0, s1 = _two_point(x, ortho)
    inv, osc = (2.0 ** -0.5, 2.0 / 2.0 ** 0.5) if ortho else (0.5, 2.0)
    ms, ph = poison((B, nb, D), torch.float64), poison((B, nb, D, 2), torch.float64)
    c0 = counts()
    rc = L.mlpg_hip_modspec(di, stream, x.data_ptr(), B, T, D, n, ortho, ms.data_ptr(), ph.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and moved(c0) == {}, (rc, L.mlpg_hip_last_error(), moved(c0))
    _all_close(ms, torch.stack([s0 * s0, s1 * s1], dim=1), 1e-12, "power")
    want_ph = torch.stack([torch.stack([torch.sign(s0), torch.zeros_like(s0)], dim=-1), torch.stack([torch.sign(s1), torch.zeros_like(s1)], dim=-1)], dim=1)
    _all_close(ph, want_ph, 1e-11, "phase")
    row("modspec (fft)", B, 1024, "complete")
    out = poison((B, n, D), torch.float64)
    rc = L.mlpg_hip_inv_modspec(di, stream, ms.data_ptr(), ph.data_ptr(), B, n, D, ortho, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    _all_close(out, x, 1e-12, "inverse of the spectrum")
    _all_close(out, torch.stack([(s0 + s1) * inv, (s0 - s1) * inv], dim=1), 1e-12, "inverse, closed form")
    row("inv_modspec (fft)", B, 1024, "complete")
    del ph, want_ph
    out = poison((B, T, D), torch.float64)
    rc = L.mlpg_hip_modspec_smoothing(di, stream, x.data_ptr(), B, T, D, n, ortho, 1, 0, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    half = (x[:, 0] + x[:, 1]) * 0.5
    _all_close(out, torch.stack([half, half], dim=1), 1e-11, "smoothing")
    row("modspec_smoothing (fft)", B, 1024, "complete")
    gm = torch.rand((B, nb, D), dtype=torch.float64, device="cuda", generator=g) + 0.1
    out = poison((B, T, D), torch.float64)
    rc = L.mlpg_hip_modspec_backward(di, stream, x.data_ptr(), gm.data_ptr(), B, T, D, n, ortho, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    a, b = gm[:, 0] * s0 * osc, gm[:, 1] * s1 * osc
    _all_close(out, torch.stack([a + b, a - b], dim=1), 1e-10, "gradient")
    row("modspec_backward (fft)", B, 1024, "complete")


@far_test
def test_modspec_entries_without_lengths_chirp_route():
    """float64, B = 2^22 + 3, T = 2, n = 3 (chirp-z), D = 2.  Closed form of the 3-point DFT of (x0, x1, 0): power (x0 + x1)^2 at bin
    0 and x0^2 + x1^2 - x0 x1 at bin 1; its gradient for g: g0 2 (x0 + x1) + g1 (2 x0 - x1) and g0 2 (x0 + x1) + g1 (2 x1 - x0); the
    inverse of spectrum and phases: the THREE frames (x0, x1, 0); smoothing with bin 1 removed: both frames (x0 + x1) / 3.
    Bounds, of the largest value: those of tests/test_modspec_chirp_gpu.py -- power and inverse 1e-11, gradient 1e-10, smoothing
    1e-10 (its bound against the direct transform)."""
    L, di, stream = lib_call()
    B, T, n, D, nb = MS_B, 2, 3, 2, 2
    assert L.mlpg_hip_modspec_route(n) == 2
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.randn((B, T, D), dtype=torch.float64, device="cuda", generator=g)
    x0, x1 = x[:, 0], x[:, 1]
    ms, ph = poison((B, nb, D), torch.float64), poison((B, nb, D, 2), torch.float64)
    c0 = counts()
    rc = L.mlpg_hip_modspec(di, stream, x.data_ptr(), B, T, D, n, 0, ms.data_ptr(), ph.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and moved(c0) == {20: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
    _all_close(ms, torch.stack([(x0 + x1) ** 2, x0 * x0 + x1 * x1 - x0 * x1], dim=1), 1e-11, "power")
    row("modspec (chirp-z)", B, 1024, "complete")
    # the inverse writes n = 3 frames per sequence where the other modes write T = 2 (or nb = 2 bins): a slice offset by the
    # wrong one of them lands on other sequences' rows.  Of the spectrum and phases above it is (x0, x1, 0).
    out = poison((B, n, D), torch.float64)
    c0 = counts()
    rc = L.mlpg_hip_inv_modspec(di, stream, ms.data_ptr(), ph.data_ptr(), B, n, D, 0, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and moved(c0) == {20: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
    _all_close(out, torch.stack([x0, x1, torch.zeros_like(x0)], dim=1), 1e-11, "inverse of the spectrum")
    row("inv_modspec (chirp-z)", B, 1024, "complete")
    del ph, ms
    # smoothing with every bin but 0 removed (plain domain): both frames (x0 + x1) / 3
    out = poison((B, T, D), torch.float64)
    c0 = counts()
    rc = L.mlpg_hip_modspec_smoothing(di, stream, x.data_ptr(), B, T, D, n, 0, 1, 0, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and moved(c0) == {20: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
    third = (x0 + x1) / 3.0
    _all_close(out, torch.stack([third, third], dim=1), 1e-10, "smoothing")
    row("modspec_smoothing (chirp-z)", B, 1024, "complete")
    del third
    gm = torch.rand((B, nb, D), dtype=torch.float64, device="cuda", generator=g) + 0.1
    out = poison((B, T, D), torch.float64)
    c0 = counts()
    rc = L.mlpg_hip_modspec_backward(di, stream, x.data_ptr(), gm.data_ptr(), B, T, D, n, 0, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and moved(c0) == {20: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
    a = gm[:, 0] * 2.0 * (x0 + x1)
    _all_close(out, torch.stack([a + gm[:, 1] * (2.0 * x0 - x1), a + gm[:, 1] * (2.0 * x1 - x0)], dim=1), 1e-10, "gradient")
    row("modspec_backward (chirp-z)", B, 1024, "complete")


# ---------------------------------------------------------------------------------------------------- MLPG: the wave kernel

WINDOWS = WINDOW_SETS["std3"]
WAVE_B = (1 << 24) + 8                                 # 8 workgroups of 256 threads per block of 8 utterances (sd = 1): 8 over
WAVE_LIMIT_B = ((1 << 24) - 1) // 8 * 8                # the utterances one launch takes: 2^24 - 8


def _solve_inputs(B, idx, lens, dt, cols, seed):
    rng = np.random.RandomState(seed)
    live = rng.randn(5, 1, cols).astype(NDT[dt])
    for i, n in enumerate(lens):
        live[i, n:] = np.nan
    return live, put(nans((B, 1, cols), TDT[dt]), idx, live), lengths_for(B, idx, lens)


@pytest.mark.parametrize("algo,name,wname", [(2, "forward (wave)", "std3"), (0, "forward (auto)", "std2")], ids=["wave", "auto"])
@far_test
def test_forward_wave_kernel(algo, name, wname):
    """float32, B = 2^24 + 8, Tmax = 1, one static dim, unit variances, lengths: mean 192 (128) MiB, out and status 64 MiB.  By name
    with three windows, and where AUTO picks the kernel: with TWO windows (static and delta) no other kernel wants a batch of
    one-frame utterances of one dim -- the FIR form takes no lengths, the transposed strip form wants three windows (with three AUTO
    takes it, a persistent grid), the constant-coefficient and strip kernels want wide streams.  The row is recorded only when the
    wave kernel's counter moved, in the large call and in the compact one."""
    from oracle import mlpg as O
    import test_stream_routes_gpu as R
    windows = WINDOW_SETS[wname]
    nw = len(windows)
    L, di, stream = lib_call()
    keep, win = win_args(windows)
    B, dt = WAVE_B, F32
    idx = five(B, 8, WAVE_LIMIT_B)
    lens = np.array([1, 1, 1, 1, 1], dtype=np.int32)
    M, mean, Ld = _solve_inputs(B, idx, lens, dt, nw, 21)
    outs = []
    for m, l in ((mean, Ld), (dev(M), dev(lens))):
        nB = m.shape[0]
        out = poison((nB, 1, 1), torch.float32)
        status = torch.full((nB,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        c0 = counts()
        rc = L.mlpg_hip_forward(di, stream, dt, algo, m.data_ptr(), None, 2, l.data_ptr(), nB, 1, nw, *win, out.data_ptr(), status.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and moved(c0) == {1: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
        assert not bool(status.any()), "a status cell is not zero"
        outs.append(out)
    big, compact = outs
    ref, st, orc = O.mlpg_batch(M.astype(np.float64), np.ones(nw), windows, lens)
    assert orc == 0
    got = compact.cpu().numpy().astype(np.float64)
    e, scale = np.abs(got - ref).max(axis=(1, 2)), np.abs(ref).max(axis=(1, 2))
    assert (e <= R.TOL[np.float32] * scale).all(), (e / scale).tolist()
    assert same_bits(big[idx], compact), name + ": a live utterance differs from the compact batch"
    assert rest_is(big, idx, 0), name + ": a dead utterance's rows are not zero"
    row(name, (B + 7) // 8 * 8, 256, "complete (kind [1])")


@pytest.mark.parametrize("algo,name", [(2, "backward (wave)"), (0, "backward (auto)")], ids=["wave", "auto"])
@far_test
def test_backward_wave_kernel(algo, name):
    """float32 grad_out (B, 1, 1) -> grad_mean (B, 1, 3), B = 2^24 + 8, unit variances, lengths: by name, and AUTO, which has no
    other kernel for a backward pass of one-frame utterances of one dim (the transposed strip form is forward only, the FIR form
    takes no lengths).  The wave kernel's counter moves once in either."""
    from oracle.grad64 import mlpg_grad64
    from test_backward_routes_gpu import _check_grad
    L, di, stream = lib_call()
    keep, win = win_args(WINDOWS)
    B, dt = WAVE_B, F32
    idx = five(B, 8, WAVE_LIMIT_B)
    lens = np.array([1, 1, 1, 1, 1], dtype=np.int32)
    GO, go, Ld = _solve_inputs(B, idx, lens, dt, 1, 22)
    outs = []
    for g, l in ((go, Ld), (dev(GO), dev(lens))):
        nB = g.shape[0]
        out = poison((nB, 1, 3), torch.float32)
        status = torch.full((nB,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        c0 = counts()
        rc = L.mlpg_hip_backward(di, stream, dt, dt, algo, None, 2, g.data_ptr(), l.data_ptr(), nB, 1, 3, *win, out.data_ptr(), status.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and moved(c0) == {1: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
        assert not bool(status.any()), "a status cell is not zero"
        outs.append(out)
    big, compact = outs
    _check_grad(compact.cpu().numpy().astype(np.float64), mlpg_grad64(None, GO.astype(np.float64), WINDOWS, lens), lens, 3e-6, "wave")
    assert same_bits(big[idx], compact), name + ": a live utterance differs from the compact batch"
    assert rest_is(big, idx, 0), name + ": a dead utterance's rows are not zero"
    row(name, (B + 7) // 8 * 8, 256, "complete (kind [1])")


def _mse_step(L, di, stream, win, B, mean, target, Ld, y, grad, loss, status, n_elems):
    ws_bytes = int(L.mlpg_hip_unit_mse_workspace_bytes(B, 3, 3))
    ws = torch.zeros(ws_bytes + 128, dtype=torch.uint8, device="cuda")
    ws_ptr = -(-ws.data_ptr() // 128) * 128
    rc = L.mlpg_hip_unit_mse_step(di, stream, F32, mean.data_ptr(), target.data_ptr(), Ld.data_ptr(), B, 1, 3, *win, n_elems, y.data_ptr(),
                                  grad.data_ptr(), loss.data_ptr(), status.data_ptr(), ws_ptr, ws_bytes)
    torch.cuda.synchronize()
    return rc, ws


@far_test
def test_unit_mse_step_refuses_over_the_limit_and_is_right_at_it():
    """The fused training step is ONE launch (an arrival counter, the last workgroup adds the partial sums): over 2^24 - 1
    workgroups it refuses with nothing written; at 2^24 - 8 utterances (2^24 - 8 workgroups, the most whole blocks of 8 under the
    limit) it runs and is right.  float32, Tmax = 1, one static dim with three windows."""
    from oracle.mse64 import unit_mse_step64
    from test_mse_routes_gpu import TOL, _check_rows
    L, di, stream = lib_call()
    keep, win = win_args(WINDOWS)
    lens = np.array([1, 1, 1, 1, 1], dtype=np.int32)
    rng = np.random.RandomState(23)
    Tg = rng.randn(5, 1, 1).astype(np.float32)
    n_elems = 5.0
    results = {}
    for B in (WAVE_B, WAVE_LIMIT_B):
        idx = five(B, 8, WAVE_LIMIT_B if B > WAVE_LIMIT_B else B - 8)
        M, mean, Ld = _solve_inputs(B, idx, lens, F32, 3, 24)
        target = put(nans((B, 1, 1), torch.float32), idx, Tg)
        y, grad = poison((B, 1, 1), torch.float32), poison((B, 1, 3), torch.float32)
        loss = poison((1,), torch.float64)
        status = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        c0 = counts()
        rc, ws = _mse_step(L, di, stream, win, B, mean, target, Ld, y, grad, loss, status, n_elems)
        if B == WAVE_B:
            msg = L.mlpg_hip_last_error().decode()
            assert rc == EINVAL and "16777215" in msg and "unit_mse_step" in msg, (rc, msg)
            assert moved(c0) == {}, moved(c0)
            for name, t in (("y_out", y), ("grad_mean", grad), ("loss", loss)):
                assert bool((t.view(-1).view(torch.uint8) == POISON).all()), name + " was written by a refused call"
            assert bool((status == 0x5A5A5A5A).all()) and not bool(ws.any())
            row("unit_mse_step (fused wave)", (B + 7) // 8 * 8, 256, "refused, nothing written; at the limit complete")
            continue
        assert rc == 0 and moved(c0) == {5: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
        assert not bool(status.any())
        results = (idx, M, y, grad, float(loss[0]))
    idx, M, y, grad, loss_big = results
    yc, gc, lc = poison((5, 1, 1), torch.float32), poison((5, 1, 3), torch.float32), poison((1,), torch.float64)
    sc = torch.full((5,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc, _ = _mse_step(L, di, stream, win, 5, dev(M), dev(Tg), dev(lens), yc, gc, lc, sc, n_elems)
    assert rc == 0, L.mlpg_hip_last_error()
    y_ref, loss_ref, grad_ref, st_ref = unit_mse_step64(M.astype(np.float64), Tg.astype(np.float64), WINDOWS, lens, n_elems)
    tol_y, tol_g, tol_l = TOL[(F32, 1)]
    _check_rows(gc.cpu().numpy(), grad_ref, lens, st_ref == 0, tol_g, "grad")
    _check_rows(yc.cpu().numpy(), y_ref, lens, st_ref == 0, tol_y, "y")
    print("unit_mse_step at the limit: loss %.17g (large) %.17g (compact) %.17g (float64)" % (loss_big, float(lc[0]), loss_ref))
    assert abs(float(lc[0]) - loss_ref) <= tol_l * loss_ref and abs(loss_big - loss_ref) <= tol_l * loss_ref
    assert same_bits(y[idx], yc) and same_bits(grad[idx], gc), "unit_mse_step: a live utterance differs from the compact batch"
    assert rest_is(y, idx, 0) and rest_is(grad, idx, 0), "unit_mse_step: a dead utterance's rows are not zero"


# ---------------------------------------------------------------------------------------------------- MLPG: the FIR form

FIR_T = 96
FIR_LIMIT_B = ((1 << 23) - 2) // 3                    # 2 B + B ceil(3 / 8) + 1 = 3 B + 1 workgroups of 512 threads: 2796202
FIR_B = FIR_LIMIT_B + 5


def _fir_solve(L, di, stream, algo, B, seed, backward=False):
    """One window (the identity), unit variances, no lengths: y = mean, and grad_mean = grad_out.  (rc, counters moved, output,
    input.)"""
    keep, win = win_args(WINDOW_SETS["static"])
    g = torch.Generator(device="cuda").manual_seed(seed)
    mean = torch.randn((B, FIR_T, 1), dtype=torch.float32, device="cuda", generator=g)
    out = poison((B, FIR_T, 1), torch.float32)
    c0 = counts()
    if backward:
        rc = L.mlpg_hip_backward(di, stream, F32, F32, algo, None, 2, mean.data_ptr(), None, B, FIR_T, 1, *win, out.data_ptr(), None)
    else:
        rc = L.mlpg_hip_forward(di, stream, F32, algo, mean.data_ptr(), None, 2, None, B, FIR_T, 1, *win, out.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, moved(c0), out, mean


@far_test
def test_fir_form_refuses_over_the_limit_and_is_right_at_it():
    """T = 96, one static dim, one window, float32: 3 B + 1 workgroups of 512 threads.  By name: B = 2796207 is refused with nothing
    written, B = 2796202 (2^23 - 1 workgroups with the training step's one more) runs; about 1 GiB per array.  Every utterance is
    live (the form takes no lengths): with the identity window y = mean, compared whole on the device at the float32 bound of
    tests/test_stream_routes_gpu.py."""
    import test_stream_routes_gpu as R
    L, di, stream = lib_call()
    rc, mv, out, mean = _fir_solve(L, di, stream, 7, 2, 30)             # (the window set's tap table is built on first use)
    assert rc == 0 and mv.get(7) == 1, (rc, L.mlpg_hip_last_error(), mv)
    rc, mv, out, mean = _fir_solve(L, di, stream, 7, FIR_B, 31)
    msg =L.mlpg_hip_last_error().decode()
    assert rc == EINVAL and "8388607" in msg and "MLPG_HIP_ALGO_FIR" in msg, (rc, msg)
    assert mv == {} and bool((out.view(-1).view(torch.uint8) == POISON).all())
    del out, mean
    rc, mv, out, mean = _fir_solve(L, di, stream, 7, FIR_LIMIT_B, 32)
    assert rc == 0 and mv == {7: 1}, (rc, L.mlpg_hip_last_error(), mv)
    assert float((out - mean).abs().max()) <= R.TOL[np.float32] * float(mean.abs().max())
    row("forward (fir)", 3 * FIR_B + 1, 512, "refused, nothing written; at the limit complete")


@far_test
def test_auto_takes_another_kernel_for_a_batch_over_the_fir_forms_limit():
    """The backward pass of float32 unit variances without lengths is AUTO's FIR case whatever the batch; over the form's limit
    AUTO takes another kernel and the whole gradient (= grad_out with the identity window) is there."""
    import test_stream_routes_gpu as R
    L, di, stream = lib_call()
    rc, mv, out, mean = _fir_solve(L, di, stream, 0, FIR_B, 33, backward=True)
    assert rc == 0 and sum(mv.values()) == 1 and 7 not in mv, (rc, L.mlpg_hip_last_error(), mv)
    assert float((out - mean).abs().max()) <= R.TOL[np.float32] * float(mean.abs().max())
    row("backward (auto, fir shape)", 3 * FIR_B + 1, 512, "complete (kind %s)" % sorted(mv))


def _fir_shape_step(L, di, stream, B, seed, tol):
    """mlpg_hip_unit_mse_step on the FIR shape (float32, no lengths, T = 96, one static dim, the identity window) with the
    workspace of mlpg_hip_unit_mse_workspace_bytes_t, which lets the entry choose the FIR form.  Every utterance is live; in
    float64 y = mean, loss = sum (y - target)^2 / n_elems and grad_mean = 2 (y - target) / n_elems, compared whole on the device:
    y and the gradient per utterance, of its largest value, as _check_rows of tests/test_mse_routes_gpu.py does.  Returns the
    counters the call moved."""
    tol_y, tol_g, tol_l = tol
    keep, win = win_args(WINDOW_SETS["static"])
    g = torch.Generator(device="cuda").manual_seed(seed)
    mean = torch.randn((B, FIR_T, 1), dtype=torch.float32, device="cuda", generator=g)
    target = torch.randn((B, FIR_T, 1), dtype=torch.float32, device="cuda", generator=g)
    y, grad = poison((B, FIR_T, 1), torch.float32), poison((B, FIR_T, 1), torch.float32)
    loss = poison((1,), torch.float64)
    status = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    n_elems = float(B * FIR_T)
    ws_bytes = int(L.mlpg_hip_unit_mse_workspace_bytes_t(B, FIR_T, 1, 1))
    ws = torch.zeros(ws_bytes + 128, dtype=torch.uint8, device="cuda")
    ws_ptr = -(-ws.data_ptr() // 128) * 128
    c0 = counts()
    rc = L.mlpg_hip_unit_mse_step(di, stream, F32, mean.data_ptr(), target.data_ptr(), None, B, FIR_T, 1, *win, n_elems, y.data_ptr(),
                                  grad.data_ptr(), loss.data_ptr(), status.data_ptr(), ws_ptr, ws_bytes)
    torch.cuda.synchronize()
    mv = moved(c0)
    assert rc == 0, L.mlpg_hip_last_error()
    del ws
    assert not bool(status.any()), "a status cell is not zero"
    per_utt = lambda t: t.view(B, -1).amax(dim=1)  # noqa: E731
    y.sub_(mean).abs_()
    assert bool((per_utt(y) <= tol_y * per_utt(mean.abs())).all()), "y differs from the mean"
    del y
    e = mean.double()
    del mean
    e.sub_(target)
    del target
    want = float(torch.dot(e.view(-1), e.view(-1))) / n_elems
    print("unit_mse_step at the FIR shape, B = %d, counters %s: loss %.17g, float64 %.17g" % (B, mv, float(loss[0]), want))
    assert abs(float(loss[0]) - want) <= tol_l * want, (float(loss[0]), want)
    e.mul_(2.0 / n_elems)                                    # the gradient in float64
    d = grad.double()
    del grad
    d.sub_(e).abs_()
    assert bool((per_utt(d) <= tol_g * per_utt(e.abs_())).all()), "the gradient differs"
    return mv


@far_test
def test_unit_mse_step_at_the_fir_shape_takes_the_fused_kernel_over_the_fir_forms_limit():
    """B = 2796207: 3 B + 1 workgroups of 512 threads are over the FIR form's limit, so the step hands the batch to the one-launch
    wave kernel (2796208 workgroups of 256 threads: under ITS limit).  Counter 5 moves once, counter 7 not at all; loss, y and
    gradient within the one-launch form's float32 bound of tests/test_mse_routes_gpu.py."""
    from test_mse_routes_gpu import TOL
    L, di, stream = lib_call()
    mv = _fir_shape_step(L, di, stream, FIR_B, 34, TOL[(F32, 1)])
    assert mv == {5: 1}, mv
    row("unit_mse_step (fir shape)", 3 * FIR_B + 1, 512, "complete (kind [5])")


@far_test
def test_unit_mse_step_takes_the_fir_form_at_its_limit():
    """B = 2796202: 3 B + 1 = 2^23 - 1 workgroups with the training step's one more -- the largest batch of this shape the FIR form
    takes.  Counter 7 moves twice (its two launches); loss, y and gradient within the FIR form's float32 bound."""
    from test_mse_routes_gpu import TOL
    L, di, stream = lib_call()
    rc, mv, out, mean = _fir_solve(L, di, stream, 7, 2, 35)              # (the window set's tap table is built on first use)
    assert rc == 0 and mv.get(7) == 1, (rc, L.mlpg_hip_last_error(), mv)
    assert 3 * FIR_LIMIT_B + 1 == LIMIT[512]
    mv = _fir_shape_step(L, di, stream, FIR_LIMIT_B, 36, TOL[(F32, 2)])
    assert mv == {7: 2}, mv


# ---------------------------------------------------------------------------------------------------- the aligner's entries

@far_test
def test_trim_lengths():
    """float32, N = 2^26 + 5, T = D = 1: one workgroup of 64 threads per utterance, every one live.  The length is 0 or 1 by
    |x| < eps."""
    L, di, stream = lib_call()
    N, eps = (1 << 26) + 5, 1e-7
    g = torch.Generator(device="cuda").manual_seed(41)
    x = torch.randn((N, 1, 1), dtype=torch.float32, device="cuda", generator=g)
    x[torch.rand((N,), device="cuda", generator=g) < 0.5] = 0.0
    x[N - 3], x[N - 2], x[N - 1] = 5e-8, -2e-7, 1.0
    out = torch.full((N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = L.mlpg_hip_trim_lengths(di, stream, F32, x.data_ptr(), N, 1, 1, eps, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    want = (~(x.view(-1).abs().double() < eps)).to(torch.int32)
    bad = out != want
    assert not bool(bad.any()), "%d lengths wrong, the first at utterance %d" % (int(bad.sum()), int(bad.int().argmax()))
    row("trim_lengths", N, 64, "complete")


@far_test
def test_gather_path():
    """float32, N = 2^24 + 5, Tsrc = 2, Tout = D = 1: one workgroup of 256 threads per utterance.  Dead utterances have path_len 0
    (their row of out is zero), the live ones copy row path[n, 0] of src."""
    L, di, stream = lib_call()
    N = (1 << 24) + 5
    idx = five(N, 5, LIMIT[256])
    rng = np.random.RandomState(42)
    S = rng.randn(5, 2, 1).astype(np.float32)
    P = np.array([[1], [0], [1], [1], [0]], dtype=np.int32)
    src = put(nans((N, 2, 1), torch.float32), idx, S)
    path = torch.full((N, 1), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    path[idx] = dev(P)
    plen = lengths_for(N, idx, [1] * 5)
    outs = []
    for s, p, l in ((src, path, plen), (dev(S), dev(P), dev(np.ones(5, dtype=np.int32)))):
        out = poison((s.shape[0], 1, 1), torch.float32)
        rc = L.mlpg_hip_gather_path(di, stream, F32, s.data_ptr(), p.data_ptr(), l.data_ptr(), s.shape[0], 2, 1, 1, 1, out.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, L.mlpg_hip_last_error()
        outs.append(out)
    big, compact = outs
    assert np.array_equal(compact.cpu().numpy()[:, 0, 0], S[np.arange(5), P[:, 0], 0])      # exact copies
    assert same_bits(big[idx], compact), "gather_path: a live utterance differs from the compact batch"
    assert rest_is(big, idx, 0), "gather_path: a dead utterance's row is not zero"
    row("gather_path", N, 256, "complete")


@far_test
def test_fastdtw():
    """N = 2^24 + 5 pairs, Tx = Ty = 2, D = 1, radius 1: more than 512 pairs, so the first launch has 256 threads per pair (limit
    2^24 - 1) and the second 512 (limit 2^23 - 1); both are over.  A dead pair (lengths 0) gets path_len 0 and the cost NaN, its
    path rows stay untouched; the live pairs' paths equal the oracle's.  No pair of a batch this long can be handed to the second
    launch: a pair costs 24 (Tx + Ty) bytes of arrays, so Tx + Ty <= 25 under 12 GiB, and the first launch's capacities (704 window
    cells, 2.5 Tx + 64 back-pointer halfwords) hold every pair of that size (at most 156 cells, Tx (Ty / 8 + 1.75) <= 42
    halfwords).  The second launch walks the same slices through the same launcher; here it finds every pair done."""
    from oracle import dtw as OD
    L, di, stream = lib_call()
    N, Tx, Ty = (1 << 24) + 5, 2, 2
    idx = five(N, 5, LIMIT[256])
    rng = np.random.RandomState(43)
    Xl, Yl = rng.randn(5, Tx, 1), rng.randn(5, Ty, 1)
    lx, ly = [2, 1, 2, 2, 1], [2, 2, 1, 2, 1]
    X, Y = put(nans((N, Tx, 1), torch.float64), idx, Xl), put(nans((N, Ty, 1), torch.float64), idx, Yl)
    outs = []
    for x, y, a, b in ((X, Y, lengths_for(N, idx, lx), lengths_for(N, idx, ly)),
                       (dev(Xl), dev(Yl), dev(np.asarray(lx, dtype=np.int32)), dev(np.asarray(ly, dtype=np.int32)))):
        n = x.shape[0]
        pi, pj = poison((n, Tx + Ty), torch.int32), poison((n, Tx + Ty), torch.int32)
        pl, cost = poison((n,), torch.int32), poison((n,), torch.float64)
        rc = L.mlpg_hip_fastdtw_l2(di, stream, x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), n, Tx, Ty, 1, 1, pi.data_ptr(),
                                   pj.data_ptr(), pl.data_ptr(), cost.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, L.mlpg_hip_last_error()
        outs.append((pi, pj, pl, cost))
    (pi, pj, pl, cost), (ci, cj, cl, cc) = outs
    hi, hj, hl, hc = ci.cpu().numpy(), cj.cpu().numpy(), cl.cpu().numpy(), cc.cpu().numpy()
    for k in range(5):
        d, path = OD.fastdtw(Xl[k, :lx[k]], Yl[k, :ly[k]], 1)
        assert hl[k] == len(path) and np.array_equal(hi[k, :hl[k]], path[:, 0]) and np.array_equal(hj[k, :hl[k]], path[:, 1]), k
        assert abs(hc[k] - d) <= 1e-12 * max(d, 1e-300), k
    assert same_bits(pl[idx], cl) and same_bits(cost[idx], cc), "fastdtw: a live pair's length or cost differs from the compact batch"
    assert same_bits(pi[idx], ci) and same_bits(pj[idx], cj), "fastdtw: a live pair's path differs from the compact batch"
    assert rest_is(pl, idx, 0), "fastdtw: a dead pair's path_len is not 0"
    dead_cost = cost.clone()
    dead_cost[idx] = float("nan")
    assert bool(torch.isnan(dead_cost).all()), "fastdtw: a dead pair's cost is not NaN"
    assert rest_is(pi, idx, POISON) and rest_is(pj, idx, POISON), "fastdtw: a dead pair's path rows were written"
    row("fastdtw", N, 256, "complete (both launches sliced)")


# ---------------------------------------------------------------------------------------------------- coverage

def test_every_row_was_run_over_its_limit():
    print("\nentry -> workgroups asked, limit, outcome")
    for name, (asked, limit, outcome) in TABLE.items():
        print("  %-32s %10d %10d  %s" % (name, asked, limit, outcome))
    missing = [r for r in ROWS if r not in TABLE]
    assert not missing, missing
    assert all(asked > limit for asked, limit, _ in TABLE.values())
