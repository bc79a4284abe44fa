"""CPU-side checks of the padded-minibatch modulation-spectrum entry points (-m "not gpu"): exports, refusals answered with
fake pointers before the runtime is touched, empty batches, mlpg_hip_modspec_loss_form and the workspace size."""
import ctypes
import math

import pytest

NEW = ("mlpg_hip_modspec_batch", "mlpg_hip_modspec_batch_backward", "mlpg_hip_modspec_loss_form",
       "mlpg_hip_modspec_loss_workspace_bytes", "mlpg_hip_modspec_loss_step")
fake = ctypes.c_void_p(64)
F32, F64 = 0, 1


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(20)]


def _batch(L, device=0, dtype=F64, x=fake, lengths=None, B=2, Tmax=10, D=3, n=16, ortho=0, ms=fake):
    return L.mlpg_hip_modspec_batch(device, None, dtype, x, lengths, B, Tmax, D, n, ortho, ms)


def _backward(L, device=0, dtype=F64, x=fake, g=fake, lengths=None, B=2, Tmax=10, D=3, n=16, ortho=0, gx=fake):
    return L.mlpg_hip_modspec_batch_backward(device, None, dtype, x, g, lengths, B, Tmax, D, n, ortho, gx)


def _step(L, device=0, dtype=F64, x=fake, tgt=fake, lengths=None, B=2, Tmax=10, D=3, n=16, ortho=0, log_domain=1, eps=1e-10,
          n_elems=54.0, gx=fake, loss=fake, ws=fake, ws_bytes=1 << 20):
    return L.mlpg_hip_modspec_loss_step(device, None, dtype, x, tgt, lengths, B, Tmax, D, n, ortho, log_domain, eps, n_elems, gx,
                                        loss, ws, ws_bytes)


def test_exports_abi_and_counter_kinds(L):
    from nnmnkwii_amd import _hip
    for name in NEW:
        assert name in _hip.EXPORTS and getattr(L, name) is not None
    assert L.mlpg_hip_abi_version() == 14
    for kind in (17, 18, 19):
        assert L.mlpg_hip_launch_count(kind) >= 0
    for kind in (12, 14, 16):
        assert L.mlpg_hip_launch_count(kind) == -1


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call below carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    inf, nan = math.inf, math.nan
    common = [dict(dtype=7), dict(dtype=-1), dict(n=1), dict(n=0), dict(n=-4), dict(B=-1), dict(Tmax=-1), dict(D=-1),
              dict(device=-1), dict(device=16), dict(device=99), dict(x=None)]
    cases = [(_batch, "modspec_batch:", common + [dict(ms=None)]),
             (_backward, "modspec_batch_backward:", common + [dict(g=None), dict(gx=None)]),
             (_step, "modspec_loss_step:", common + [dict(tgt=None), dict(gx=None), dict(loss=None), dict(eps=-1e-30), dict(eps=inf),
                                                      dict(eps=nan), dict(n_elems=0.0), dict(n_elems=-1.0), dict(n_elems=inf),
                                                      dict(n_elems=nan), dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=8),
                                                      dict(n=100), dict(n=8192), dict(n=24)])]
    for call, who, kws in cases:
        for kw in kws:
            rc = call(L, **kw)
            err = L.mlpg_hip_last_error().decode()
            assert rc == -1 and err.startswith(who), (who, kw, rc, err)
    need = L.mlpg_hip_modspec_loss_workspace_bytes(2, 3)
    assert _step(L, ws_bytes=need - 1) == -1 and b"workspace" in L.mlpg_hip_last_error()
    # more utterances than the direct transform's grid takes
    assert _batch(L, B=70000, n=100) == -1 and b"65535" in L.mlpg_hip_last_error()
    assert _backward(L, B=70000, n=100) == -1 and b"65535" in L.mlpg_hip_last_error()
    assert _counts(L) == c0


def test_empty_batches_are_no_ops(L):
    c0 = _counts(L)
    for kw in (dict(B=0), dict(D=0), dict(B=0, D=0)):
        assert _batch(L, x=None, ms=None, **kw) == 0
        assert _backward(L, x=None, g=None, gx=None, **kw) == 0
        assert _step(L, x=None, tgt=None, gx=None, loss=None, ws=None, ws_bytes=0, **kw) == 0
    assert _backward(L, Tmax=0, x=None) == 0                 # no row of grad_x to write
    assert _counts(L) == c0


def test_loss_form_names_the_lengths_the_fused_step_takes(L):
    for n in list(range(-2, 70)) + [100, 1000, 1024, 2047, 2048, 2049, 4096, 4097, 5000, 8192, 1 << 20]:
        want = 1 if 2 <= n <= 4096 and n & (n - 1) == 0 else 0
        assert L.mlpg_hip_modspec_loss_form(n) == want, n
    L.mlpg_hip_modspec_set_direct(1)
    try:
        for n in (2, 16, 2048, 4096, 100):
            assert L.mlpg_hip_modspec_loss_form(n) == 0
        assert _step(L, n=16) == -1 and b"modspec_loss_step:" in L.mlpg_hip_last_error()
    finally:
        L.mlpg_hip_modspec_set_direct(0)
    assert L.mlpg_hip_modspec_loss_form(2048) == 1


def test_loss_workspace_bytes(L):
    f = L.mlpg_hip_modspec_loss_workspace_bytes
    for B in (0, 1, 2, 7, 256, 4096):
        for D in (0, 1, 2, 3, 59, 60, 61, 512):
            assert f(B, D) >= 8 * B * ((D + 1) // 2)
            assert f(B + 1, D) >= f(B, D) and f(B, D + 1) >= f(B, D)
    assert f(-1, 4) == 0 and f(4, -1) == 0
