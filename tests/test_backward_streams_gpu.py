"""GPU tests (-m gpu): mlpg_hip_backward_streams, driven through raw stream tables, and autograd.multi_stream_mlpg that rests on
it, against tests/streamgrad64.py (float64, numpy only; pinned by tests/test_streamgrad64_cpu.py).

The layouts are those of tests/test_stream_routes_gpu.py: permuted output columns, unused columns between and beside the
streams in input and output rows (NaN in the unused input columns), ld_out > sum static_dim, odd in_col / out_col, per-stream
window lists, 1- and 60-dim streams.  Before each call grad_mean and grad_var hold a NaN sentinel of a fixed bit pattern and
the status array 0x5A5A5A5A; the padding rows of mean, var, y and grad_out hold NaN.  In every accepted cell
- the return code is 0; every dynamic stream moves its solve family's counter by one (the forced family's; under AUTO one of
  them), kind 15 moves by one per distinct window list when grad_var is asked for plus one for the pass-through streams, kind
  13 does not move;
- grad_mean matches the reference to 1e-10 (float64) / 3e-6 (float32) of the utterance's largest entry and grad_var to the same
  bars with the `terms` floor of tests/test_var_grad_gpu.py (its _check_var_grad, _masked and _terms, imported), padding rows
  and masked entries exactly 0;
- pass-through streams: grad_mean a bit copy of grad_out on live rows, 0 on padding, grad_var 0, status 0;
- every column outside the streams keeps the sentinel bit for bit, every status cell is written.
A refused cell returns EINVAL naming the stream and the algo, moves no counter and leaves every sentinel intact."""
import ctypes
import zlib

import numpy as np
import pytest

import stream_plan as SP
import streamgrad64 as SG
from test_backward_routes_gpu import ALGO_NAMES, FAMILIES, _check_grad, supported
from test_stream_routes_gpu import SENT, STATUS_SENT, _int_view, _poison, layout, make_inputs
from test_stream_routes_gpu import drive as drive_forward
from test_var_grad_gpu import _check_var_grad, _masked, _terms

pytestmark = pytest.mark.gpu

F, G, U = SP.VAR_FRAME, SP.VAR_GLOBAL, SP.VAR_UNIT
f64, f32 = np.float64, np.float32
TOL = {f64: 1e-10, f32: 3e-6}
SOLVE_KINDS = {kind: fam for fam, (_, kind) in FAMILIES.items()}
EPILOGUE_KIND = 15
WATCHED = tuple(range(10)) + (13, 15)
MODE_NAME = {F: "frame", G: "global", U: "unit"}
_ALGO = {0: "auto", 1: "generic", 2: "wave", 3: "strip", 5: "const", 6: "chunk", 7: "fir"}


def _counts():
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return {k: L.mlpg_hip_launch_count(k) for k in WATCHED}


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sg_streams(lay, streams=None):
    return [dict(in_col=s["in_col"], out_col=s["out_col"], static_dim=s["static_dim"],
                 windows=lay.windows_of(s) if s["num_windows"] else None) for s in (lay.streams if streams is None else streams)]


def drive(lay, M, V, mode, L, Y, GO, algo, want_var=True, want_status=True, streams=None, ld_out=None):
    """One raw mlpg_hip_backward_streams call on the current torch stream.  grad_mean / grad_var (B, T, ld_in) start as the NaN
    sentinel, status (B, sum static_dim) as 0x5A5A5A5A.  Returns (rc, grad_mean, grad_var, status, counter deltas, error text)."""
    import torch
    from nnmnkwii_amd import _hip
    streams = lay.streams if streams is None else streams
    ld_out = lay.ld_out if ld_out is None else ld_out
    B, T, ld_in = M.shape
    table = (_hip.StreamDesc * max(len(streams), 1))()
    for k, s in enumerate(streams):
        table[k] = _hip.StreamDesc(s["in_col"], s["out_col"], s["static_dim"], s["num_windows"], s["win_first"])
    dt = f64 if M.dtype == torch.float64 else f32
    it = torch.int64 if dt == f64 else torch.int32
    gm = torch.full((B, T, ld_in), SENT[dt], dtype=it, device=M.device).view(M.dtype)
    gv = torch.full((B, T, ld_in), SENT[dt], dtype=it, device=M.device).view(M.dtype)
    sd_total = sum(s["static_dim"] for s in streams)
    status = torch.full((B, max(sd_total, 1)), STATUS_SENT, dtype=torch.int32, device=M.device)
    torch.cuda.synchronize()
    c0 = _counts()
    rc = _hip.lib().mlpg_hip_backward_streams(
        M.device.index, _hip._stream(M.device), _hip._dt(M), algo, _hip._p(M), _hip._p(V), mode, ld_in, _hip._p(Y), _hip._p(GO),
        ld_out, _hip._p(L), B, T, len(streams), ctypes.addressof(table), lay.n_win, _hip._np(lay.wl), _hip._np(lay.wu),
        _hip._np(lay.wc), _hip._p(gm), _hip._p(gv) if want_var else None, _hip._p(status) if want_status else None)
    err = _hip.lib().mlpg_hip_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    moved = {k: n - c0[k] for k, n in _counts().items() if n != c0[k]}
    return rc, gm, gv, status, moved, err


def _warm_fir(lay):
    import torch
    from nnmnkwii_amd import _hip
    for s in lay.streams:
        if s["num_windows"]:
            try:
                _hip.forward(torch.zeros((1, 96, s["num_windows"]), dtype=torch.float32, device="cuda"), None, lay.windows_of(s),
                             algo=_hip.ALGO_FIR)
            except _hip.HipExtensionError:
                pass
    torch.cuda.synchronize()


def prepare(lay, dt, mode, B, T, ragged, seed, poisons=()):
    """Inputs of one cell as numpy: means, variances (NaN in unused columns), lengths, the trajectory of the GPU's own forward call
    and a random grad_out (NaN in the columns no stream owns); then NaN in every padding row of all four."""
    M, V, lens = make_inputs(lay, dt, mode, B, T, ragged, seed)
    Vp = _poison(lay, V, mode, lens, poisons) if poisons else V
    rc, out, _, _, err = drive_forward(lay, _dev(M), _dev(Vp), mode, _dev(lens), SP.AUTO)
    assert rc == 0, err
    Y = out.cpu().numpy()
    rng = np.random.RandomState(seed ^ 0x5BD1)
    GO = rng.randn(B, T, lay.ld_out).astype(dt)
    _, oo = SG.owned(sg_streams(lay), lay.ld_in, lay.ld_out)
    GO[:, :, ~oo] = np.nan
    if lens is not None:
        pad = np.arange(T)[None, :] >= lens[:, None]
        M, Y = M.copy(), Y.copy()
        M[pad] = np.nan
        Y[pad] = np.nan
        GO[pad] = np.nan
        if mode == F:
            V, Vp = V.copy(), Vp.copy()
            V[pad] = np.nan
            Vp[pad] = np.nan
    return M, V, Vp, lens, Y, GO


def expected_moves(lay, want_var, streams=None):
    """(number of solves, epilogue launches) of an accepted call."""
    streams = lay.streams if streams is None else streams
    dyn = [s for s in streams if s["num_windows"] and s["static_dim"]]
    lists = {(s["win_first"], s["num_windows"]) for s in dyn}
    has_pass = any(s["num_windows"] == 0 and s["static_dim"] for s in streams)
    return len(dyn), (len(lists) if want_var else 0) + int(has_pass)


def check_counters(lay, moved, algo, want_var):
    n_dyn, n_epi = expected_moves(lay, want_var)
    moved = dict(moved)
    assert moved.pop(EPILOGUE_KIND, 0) == n_epi, ("epilogue launches", moved, n_epi)
    assert 13 not in moved, moved
    assert set(moved) <= set(SOLVE_KINDS), moved
    assert sum(moved.values()) == n_dyn, ("solves", moved, n_dyn)
    if algo != SP.AUTO:
        fam = _ALGO[algo]
        assert moved == ({FAMILIES[fam][1]: n_dyn} if n_dyn else {}), (fam, moved)


def check_outputs(lay, M, V, Vp, mode, lens, Y, GO, gm, gv, status, dt, want_var, poisons=()):
    B, T, _ = M.shape
    lens_a = np.full(B, T, dtype=np.int32) if lens is None else lens
    live = np.arange(T)[None, :] < lens_a[:, None]
    streams = sg_streams(lay)
    oi, _ = SG.owned(streams, lay.ld_in, lay.ld_out)
    tol = TOL[dt]
    # the reference on the healthy variances; the poisoned systems are compared apart
    y_ref, gm_ref, gv_ref = SG.multi_stream_grad64(M, V, GO, streams, lens)
    exp_status = np.zeros((B, lay.sd_total), dtype=np.int32)
    bad = {}
    for k, d in poisons:
        s = lay.streams[k]
        cols = [s["in_col"] + j * s["static_dim"] + d for j in range(s["num_windows"])]
        from oracle import mlpg as O
        clean = lambda a: np.where(live[:, :, None], a, 1.0)  # noqa: E731
        v1 = Vp[cols] if mode == G else np.ascontiguousarray(clean(Vp[:, :, cols]))
        _, st1, _ = O.mlpg_batch(np.ascontiguousarray(clean(M[:, :, cols])), v1, lay.windows_of(s), lens)
        assert (st1[lens_a > 0, 0] > 0).any(), ("poison did not fail", k, d)
        exp_status[:, lay.stat_col[k] + d] = st1[:, 0]
        bad[(k, d)] = st1[:, 0] != 0
    for k, s in enumerate(streams):
        sd, ic, oc = s["static_dim"], s["in_col"], s["out_col"]
        if sd == 0:
            continue
        what = (k, sd, MODE_NAME[mode], dt.__name__)
        if not s["windows"]:
            got = gm[:, :, ic:ic + sd]
            assert not got[~live].any(), what + ("pass-through padding",)
            assert np.array_equal(_int_view(got[live]), _int_view(GO[:, :, oc:oc + sd][live])), what + ("pass-through copy",)
            if want_var:
                assert not gv[:, :, ic:ic + sd].any(), what + ("pass-through grad_var",)
            continue
        cols = SG.stream_cols(s)
        got_m, ref_m = gm[:, :, cols].copy(), gm_ref[:, :, cols].copy()
        got_v = gv[:, :, cols].copy() if want_var else None
        ref_v = gv_ref[:, :, cols].copy() if want_var else None
        nw = len(s["windows"])
        for (kk, d), failed in bad.items():
            if kk != k:
                continue
            dcols = [j * sd + d for j in range(nw)]
            # a failing system: every column exactly 0 (and left out of the comparison with the reference, which was computed on
            # the healthy variances); the utterances where this dim is healthy hold the same variances in both and are compared
            assert not got_m[failed][:, :, dcols].any(), what + ("failed system's grad_mean not zero", d)
            if want_var:
                assert not got_v[failed][:, :, dcols].any(), what + ("failed system's grad_var not zero", d)
            for a in (got_m, ref_m, got_v, ref_v):
                if a is not None:
                    a[np.ix_(failed, np.arange(T), dcols)] = 0.0
        _check_grad(got_m, ref_m, lens_a, tol, what + ("grad_mean",))
        if want_var:
            zero = lambda a: np.where(live[:, :, None], a, 0.0)  # noqa: E731
            Ms = zero(M[:, :, cols])
            Vs = np.broadcast_to(V[cols], Ms.shape).astype(dt) if mode == G else np.where(live[:, :, None], V[:, :, cols], 1.0).astype(dt)
            terms = _terms(Ms, Vs, y_ref[:, :, oc:oc + sd], ref_m, s["windows"])
            _check_var_grad(got_v, ref_v, lens_a, _masked(s["windows"], lens_a, T, sd), tol, what + ("grad_var",), terms)
    for name, arr in (("grad_mean", gm), ("grad_var", gv)):
        rest = _int_view(arr[:, :, ~oi]) if (want_var or name == "grad_mean") else _int_view(arr)
        assert (rest == SENT[dt]).all(), (name, "a column outside the streams was written")
    assert not (status == STATUS_SENT).any(), ("status cells left unwritten", np.argwhere(status == STATUS_SENT)[:4].tolist())
    assert np.array_equal(status, exp_status), ("status", np.argwhere(status != exp_status)[:4].tolist())


def stream_supported(lay, s, fam, mode, dt, T, has_lengths):
    return supported(fam, lay.windows_of(s), MODE_NAME[mode], dt, dt, T, has_lengths)


def cell_accepted(lay, algo, mode, dt, T, ragged):
    """None when every dynamic stream can take the forced family, else the index of the first one that cannot."""
    if algo == SP.AUTO:
        return None
    for k, s in enumerate(lay.streams):
        if s["num_windows"] and s["static_dim"] and not stream_supported(lay, s, _ALGO[algo], mode, dt, T, ragged):
            return k
    return None


def untouched(gm, gv, status, dt):
    return ((_int_view(gm.cpu().numpy()) == SENT[dt]).all() and (_int_view(gv.cpu().numpy()) == SENT[dt]).all()
            and (status.cpu().numpy() == STATUS_SENT).all())


def run_cell(lname, dt, mode, ragged, algo, T, B, poisons=()):
    lay = layout(lname)
    seed = zlib.crc32(repr(("bwd", lname, dt.__name__, mode, ragged, algo, T, B)).encode()) & 0x7FFFFFFF
    want_var = mode != U
    M, V, Vp, lens, Y, GO = prepare(lay, dt, mode, B, T, ragged, seed, poisons)
    if dt == f32 and mode == U and not ragged:
        _warm_fir(lay)
    refused = cell_accepted(lay, algo, mode, dt, T, ragged)
    rc, gm, gv, status, moved, err = drive(lay, _dev(M), _dev(Vp), mode, _dev(lens), _dev(Y), _dev(GO), algo, want_var)
    if refused is not None:
        assert rc == -1 and "stream %d: MLPG_HIP_ALGO_%s" % (refused, ALGO_NAMES[algo]) in err, (rc, err)
        assert moved == {} and untouched(gm, gv, status, dt), (moved, "a refused cell ran a kernel or wrote an output")
        return False
    assert rc == 0, err
    check_counters(lay, moved, algo, want_var)
    check_outputs(lay, M, V, Vp, mode, lens, Y, GO, gm.cpu().numpy(), gv.cpu().numpy(), status.cpu().numpy(), dt, want_var, poisons)
    return True


def _cell_id(c):
    return "%s-%s-%s-%s-%s-T%d-B%d%s" % (c[0], c[1].__name__, MODE_NAME[c[2]], "ragged" if c[3] else "full", _ALGO[c[4]], c[5], c[6],
                                         "-neg" if len(c) > 7 and c[7] else "")


def _matrix():
    """Layouts x dtypes x variance modes x forced families and AUTO x lengths x T from 1 to beyond 2048.  Every layout meets every
    family, mode and dtype; the utterance lengths rotate through the cells so that each family sees short, medium and long
    ones with and without lengths."""
    cells = []
    shapes = [(1, 1, False), (2, 6, True), (65, 6, True), (300, 6, True), (300, 2, False), (1100, 5, True), (2100, 4, True)]
    i = 0
    for lname in ("merlin", "mixed", "mixed_ext1", "zero_dim", "ones64", "two60_10", "slice_wide3"):
        for algo in (SP.AUTO, SP.GENERIC, SP.WAVE, SP.STRIP, SP.CONST, SP.CHUNK, SP.FIR):
            for mode in (F, G, U):
                for dt in (f64, f32):
                    T, B, ragged = shapes[i % len(shapes)]
                    i += 1
                    if algo == SP.FIR:
                        if not (mode == U and dt == f32):
                            continue                      # (its refusals are covered once per layout below)
                        T, B, ragged = (300, 3, False)
                    cells.append((lname, dt, mode, ragged, algo, T, B))
        cells.append((lname, f64, F, True, SP.FIR, 300, 6))     # refused: names the stream and the algo
        i += 1                                                  # the next layout meets every (family, mode, dtype) at another shape
    return cells


MATRIX = _matrix()


@pytest.mark.parametrize("cell", MATRIX, ids=[_cell_id(c) for c in MATRIX])
def test_backward_streams_cell(cell):
    run_cell(*cell)


def test_matrix_reaches_every_family_and_both_verdicts():
    """The matrix as a whole: every forced family is accepted somewhere and refused somewhere, in every layout family mix."""
    acc, ref = set(), set()
    for c in MATRIX:
        (acc if cell_accepted(layout(c[0]), c[4], c[2], c[1], c[5], c[3]) is None else ref).add(c[4])
    assert acc >= {SP.AUTO, SP.GENERIC, SP.WAVE, SP.STRIP, SP.CONST, SP.CHUNK, SP.FIR}, acc
    assert ref >= {SP.WAVE, SP.STRIP, SP.CONST, SP.CHUNK, SP.FIR}, ref


POISONED = [
    ("merlin", f64, F, True, SP.AUTO, 300, 6, [(0, 5), (3, 4)]),
    ("merlin", f32, F, False, SP.WAVE, 65, 2, [(3, 3)]),
    ("merlin", f64, G, True, SP.CONST, 300, 6, [(0, 7)]),
    ("mixed", f64, F, True, SP.GENERIC, 65, 6, [(1, 3)]),
    ("mixed_ext1", f32, F, True, SP.STRIP, 300, 6, [(1, 2)]),
    ("slice_wide3", f64, F, True, SP.CHUNK, 300, 6, [(0, 5)]),
]


@pytest.mark.parametrize("cell", POISONED, ids=[_cell_id(c) for c in POISONED])
def test_failing_system_in_one_stream(cell):
    """A negative variance in one system of one stream: its status cell holds the oracle's verdict, its grad_mean and grad_var
    columns are 0, every other system and stream is unaffected (compared with the reference as in a healthy cell)."""
    assert run_cell(*cell)


def test_means_only_call_needs_no_mean_y_status_and_launches_no_variance_work():
    """grad_var NULL: mean, y and status may be NULL too; kind 15 moves only for the pass-through streams."""
    import torch
    lay = layout("merlin")
    for mode, dt in ((F, f64), (G, f32), (U, f32)):
        M, V, Vp, lens, Y, GO = prepare(lay, dt, mode, 6, 300, True, 31)
        B, T, ld_in = M.shape
        rc, gm, gv, status, moved, err = drive(lay, _dev(M), _dev(V), mode, _dev(lens), _dev(Y), _dev(GO), SP.AUTO, want_var=False)
        assert rc == 0, err
        check_counters(lay, moved, SP.AUTO, False)
        check_outputs(lay, M, V, V, mode, lens, Y, GO, gm.cpu().numpy(), gv.cpu().numpy(), status.cpu().numpy(), dt, False)
        # the same call without mean, y and status
        from nnmnkwii_amd import _hip
        table = (_hip.StreamDesc * len(lay.streams))()
        for k, s in enumerate(lay.streams):
            table[k] = _hip.StreamDesc(s["in_col"], s["out_col"], s["static_dim"], s["num_windows"], s["win_first"])
        gm2 = torch.zeros_like(gm)
        Vd, Ld, God = _dev(V), _dev(lens), _dev(GO)
        rc = _hip.lib().mlpg_hip_backward_streams(0, _hip._stream(gm2.device), _hip._dt(gm2), 0, None, _hip._p(Vd), mode, ld_in, None,
                                                  _hip._p(God), lay.ld_out, _hip._p(Ld), B, T, len(lay.streams),
                                                  ctypes.addressof(table), lay.n_win, _hip._np(lay.wl), _hip._np(lay.wu),
                                                  _hip._np(lay.wc), _hip._p(gm2), None, None)
        assert rc == 0, _hip.lib().mlpg_hip_last_error().decode()
        torch.cuda.synchronize()
        oi, _ = SG.owned(sg_streams(lay), lay.ld_in, lay.ld_out)
        a, b = gm.cpu().numpy()[:, :, oi], gm2.cpu().numpy()[:, :, oi]
        assert np.array_equal(_int_view(a), _int_view(b))


def test_refused_tables_launch_nothing_and_touch_nothing():
    lay = layout("ones64")
    M, V, Vp, lens, Y, GO = prepare(lay, f64, F, 6, 65, True, 5)
    args = (_dev(M), _dev(V), F, _dev(lens), _dev(Y), _dev(GO))
    rc, gm, gv, status, moved, err = drive(lay, *args, SP.AUTO)                 # 64 streams are accepted
    assert rc == 0, err
    s65 = lay.streams + [dict(lay.streams[1])]
    rc, gm, gv, status, moved, err = drive(lay, *args, SP.AUTO, streams=s65)
    assert rc == -1 and "64 streams" in err and moved == {} and untouched(gm, gv, status, f64), (rc, err, moved)
    lay = layout("merlin")
    M, V, Vp, lens, Y, GO = prepare(lay, f32, F, 6, 300, True, 6)
    args = (_dev(M), _dev(V), F, _dev(lens), _dev(Y), _dev(GO))
    for field, value in (("out_col", lay.ld_out - 4), ("in_col", lay.ld_in - 14)):
        bad = [dict(s) for s in lay.streams]
        bad[3][field] = value                                                   # bap: 5 dims, 15 input columns
        rc, gm, gv, status, moved, err = drive(lay, *args, SP.AUTO, streams=bad)
        assert rc == -1 and "stream 3 does not fit" in err and moved == {} and untouched(gm, gv, status, f32), (field, rc, err)
    # grad_var with unit variances, grad_var without status
    rc, gm, gv, status, moved, err = drive(lay, args[0], None, U, *args[3:], SP.AUTO, want_var=True)
    assert rc == -1 and "MLPG_HIP_VAR_UNIT" in err and moved == {} and untouched(gm, gv, status, f32), (rc, err)
    rc, gm, gv, status, moved, err = drive(lay, *args, SP.AUTO, want_status=False)
    assert rc == -1 and "status" in err and moved == {} and untouched(gm, gv, status, f32), (rc, err)
    # a refusal leaves the stream usable
    rc, gm, gv, status, moved, err = drive(lay, *args, SP.AUTO)
    assert rc == 0, err
    check_outputs(lay, M, V, V, F, lens, Y, GO, gm.cpu().numpy(), gv.cpu().numpy(), status.cpu().numpy(), f32, True)


@pytest.mark.parametrize("lname", ["merlin", "mixed", "slice_wide3"])
@pytest.mark.parametrize("dt", [f64, f32])
def test_masked_variance_entries_are_never_read(lname, dt):
    """Masked entries of per-frame variances filled with 0, -1 and NaN: grad_var exactly 0 there, every other entry of both
    gradients bit-identical -- on every family but strip, which this check leaves out by name: its existing backward solve reads
    masked entries (tests/test_var_grad_gpu.py test_masked_variance_entries_are_never_read)."""
    lay = layout(lname)
    B, T = 6, 150
    M, V, Vp, lens, Y, GO = prepare(lay, dt, F, B, T, True, 77)
    masked = np.zeros(V.shape, dtype=bool)
    for s in sg_streams(lay):
        if s["windows"] and s["static_dim"]:
            masked[:, :, SG.stream_cols(s)] = _masked(s["windows"], lens, T, s["static_dim"])
    for fam in ("auto", "generic", "wave", "chunk"):
        algo = 0 if fam == "auto" else FAMILIES[fam][0]
        if cell_accepted(lay, algo, F, dt, T, True) is not None:
            continue
        base = drive(lay, _dev(M), _dev(V), F, _dev(lens), _dev(Y), _dev(GO), algo)
        assert base[0] == 0, base[5]
        if base[4].get(FAMILIES["strip"][1], 0):
            continue                                                             # AUTO took the strip family for some stream
        for fill in (0.0, -1.0, np.nan):
            Vx = V.copy()
            Vx[masked] = fill
            rc, gm, gv, status, moved, err = drive(lay, _dev(M), _dev(Vx), F, _dev(lens), _dev(Y), _dev(GO), algo)
            what = (lname, dt.__name__, fam, fill)
            assert rc == 0 and not status.cpu().numpy().any(), what + (err,)
            gvn = gv.cpu().numpy()
            assert not gvn[masked].any(), what + ("masked grad_var",)
            assert np.array_equal(_int_view(gvn), _int_view(base[2].cpu().numpy())), what + ("grad_var",)
            assert np.array_equal(_int_view(gm.cpu().numpy()), _int_view(base[1].cpu().numpy())), what + ("grad_mean",)


def test_dense_single_stream_is_bit_identical_to_backward_var():
    """One stream at column 0 with ld_in = D and ld_out = sd is the dense problem: grad_mean and the status are those of
    mlpg_hip_backward_var bit for bit on every family, grad_var to a few units in the last place."""
    import torch
    from cases import WINDOW_SETS
    from nnmnkwii_amd import _hip
    rng = np.random.RandomState(9)
    for wname, sd in (("std3", 60), ("std3", 5), ("wide3", 7), ("asym2", 3)):
        w = WINDOW_SETS[wname]
        B, T, D = 5, 200, len(w) * sd
        lens = _dev(np.array([200, 199, 77, 1, 0], dtype=np.int32))
        for dt in (torch.float64, torch.float32):
            m = torch.from_numpy(rng.randn(B, T, D)).to(dt).cuda()
            vf = torch.from_numpy(rng.rand(B, T, D) + 0.1).to(dt).cuda()
            go = torch.from_numpy(rng.randn(B, T, sd)).to(dt).cuda()
            for v in (vf, vf[0, 0].clone()):
                y, _ = _hip.forward(m, v, w, lens)
                for fam in ("auto", "generic", "wave", "strip", "const", "chunk"):
                    mode = "frame" if v.dim() == 3 else "global"
                    if fam != "auto" and not supported(fam, w, mode, np.float64, np.float64, T, True):
                        continue
                    algo = 0 if fam == "auto" else FAMILIES[fam][0]
                    a = _hip.backward_var(m, v, y, go, w, lens, algo=algo)
                    b = _hip.backward_streams(m, v, y, go, [(0, sd, w)], lens, algo=algo)
                    what = (wname, sd, dt, mode, fam)
                    assert torch.equal(a[0], b[0]) and torch.equal(a[2].view(B, sd), b[2]), what
                    # (grad_var: the same formula in another kernel -- the compiler may contract its multiply-adds differently)
                    eps = torch.finfo(dt).eps
                    assert float((a[1] - b[1]).abs().max()) <= 4 * eps * float(a[1].abs().max()), what


# ---------------------------------------------------------------------------------------------------- the autograd surface

SIZES, DYN = [180, 3, 1, 15], [True, True, False, True]


def _merlin_streams(windows):
    out, col, oc = [], 0, 0
    for size, d in zip(SIZES, DYN):
        sd = size // len(windows) if d else size
        out.append(dict(in_col=col, out_col=oc, static_dim=sd, windows=windows if d else None))
        col += size
        oc += sd
    return out


def _grads(fn, m, v, go):
    m = m.detach().clone().requires_grad_()
    v = None if v is None else v.detach().clone().requires_grad_()
    y = fn(m, v)
    y.backward(go.to(y.device))
    return y.detach(), m.grad, None if v is None else v.grad


def _composed(m, v, windows, lens):
    """What a user writes without the in-place call: slices, one mlpg_batch per dynamic stream, cat."""
    import torch
    from nnmnkwii_amd import autograd as AF
    live = (torch.arange(m.shape[1], device=m.device)[None, :] < torch.as_tensor(lens, device=m.device)[:, None])[:, :, None]
    ys, col = [], 0
    for size, d in zip(SIZES, DYN):
        ms = m[:, :, col:col + size].contiguous()
        if d:
            ys.append(AF.mlpg_batch(ms, v[..., col:col + size].contiguous(), windows, lens))
        else:
            ys.append(ms * live)
        col += size
    return torch.cat(ys, dim=2)


@pytest.mark.parametrize("dt", [f64, f32])
def test_autograd_matches_reference_composed_form_and_paramgen(dt):
    import torch
    from cases import WINDOW_SETS
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd import paramgen as PG
    w = WINDOW_SETS["std3"]
    B, T = 4, 120
    rng = np.random.RandomState(3)
    lens = np.array([120, 77, 1, 0], dtype=np.int32)
    M = rng.randn(B, T, 199).astype(dt)
    Vf = (rng.rand(B, T, 199) + 0.1).astype(dt)
    GO = rng.randn(B, T, 67).astype(dt)
    streams = _merlin_streams(w)
    tol = TOL[dt]
    for var in (Vf, Vf[0, 0].copy()):
        m, v, go = _dev(M), _dev(var), _dev(GO)
        y, gm, gv = _grads(lambda a, b: AF.multi_stream_mlpg(a, b, w, SIZES, DYN, lens), m, v, go)
        assert y.dtype == m.dtype and gm.dtype == m.dtype and gv.dtype == m.dtype and gv.shape == v.shape and gm.shape == m.shape
        assert torch.equal(y, PG.multi_stream_mlpg(m, v, w, SIZES, DYN, lengths=lens))
        y_ref, gm_ref, gv_ref = SG.multi_stream_grad64(M, var, GO, streams, lens)
        _check_grad(gm.cpu().numpy(), gm_ref, lens, tol, ("autograd grad_mean", dt.__name__, var.ndim))
        yc, gmc, gvc = _grads(lambda a, b: _composed(a, b, w, lens), m, v, go)
        gvn, gvcn = gv.double().cpu().numpy(), gvc.double().cpu().numpy()
        if var.ndim == 1:
            # the (D,) gradient is the float64 sum of N = sum(lens) per-frame contributions.  Each is within tol of its stream's
            # largest one (the bar of the per-frame checks of run_cell, which leaves two decades over the rounding errors it
            # covers); those errors are independent from frame to frame, so their sum grows like sqrt(N), not N: the sum is held
            # to tol * sqrt(N) * that largest contribution
            bar = np.zeros(199)
            for s in streams:
                cols = SG.stream_cols(s)
                bar[cols] = tol * np.sqrt(lens.sum()) * np.abs(gv_ref[:, :, cols]).max()
            for got in (gvn, gvcn):
                assert (np.abs(got - gv_ref.sum(axis=(0, 1))) <= bar).all() and got[183] == 0, ("autograd (D,) grad_var", dt.__name__)
        else:
            for k, s in enumerate(streams):
                cols = SG.stream_cols(s)
                if not s["windows"]:
                    assert not gvn[:, :, cols].any()
                    continue
                sd = s["static_dim"]
                live = (np.arange(T)[None, :] < lens[:, None])[:, :, None]
                terms = _terms(np.where(live, M[:, :, cols], 0), np.where(live, Vf[:, :, cols], 1).astype(dt),
                               y_ref[:, :, s["out_col"]:s["out_col"] + sd], gm_ref[:, :, cols], w)
                for got in (gvn, gvcn):
                    _check_var_grad(got[:, :, cols], gv_ref[:, :, cols], lens, _masked(w, lens, T, sd), tol, ("autograd grad_var", k), terms)
        _check_grad(gmc.cpu().numpy(), gm_ref, lens, tol, ("composed grad_mean", dt.__name__, var.ndim))
    # unit variances: the means' gradient alone
    y, gm, gv = _grads(lambda a, b: AF.multi_stream_mlpg(a, None, w, SIZES, DYN, lens), _dev(M), None, _dev(GO))
    _, gm_ref, _ = SG.multi_stream_grad64(M, None, GO, streams, lens)
    _check_grad(gm.cpu().numpy(), gm_ref, lens, tol, ("unit grad_mean", dt.__name__))
    assert torch.equal(y, PG.multi_stream_mlpg(_dev(M), None, w, SIZES, DYN, lengths=lens))


def test_gradcheck():
    """torch.autograd.gradcheck, float64, a small three-stream layout with a pass-through stream and per-stream window lists,
    ragged lengths, per-frame and global variances, both inputs requiring grad."""
    import torch
    from cases import WINDOW_SETS
    from nnmnkwii_amd import autograd as AF
    wl = [WINDOW_SETS["std3"], None, WINDOW_SETS["asym2"], WINDOW_SETS["wide3"]]
    sizes, dyn = [6, 1, 4, 3], [True, False, True, True]
    for T in (1, 3, 9, 33):
        rng = np.random.RandomState(T)
        lengths = [T, max(T // 2, 1) if T > 1 else 0]
        m = torch.from_numpy(rng.randn(2, T, 14)).cuda().requires_grad_()
        for v_np in (rng.rand(2, T, 14) + 0.5, rng.rand(14) + 0.5):
            v = torch.from_numpy(v_np).cuda().requires_grad_()
            assert torch.autograd.gradcheck(lambda a, b: AF.multi_stream_mlpg(a, b, wl, sizes, dyn, lengths), (m, v), eps=1e-6,
                                            atol=1e-6, rtol=1e-4), (T, v_np.ndim)


def test_2d_cpu_tensors_needs_input_grad_and_errors(monkeypatch):
    import torch
    from cases import WINDOW_SETS
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd.autograd import _mlpg
    w = WINDOW_SETS["std3"]
    rng = np.random.RandomState(5)
    m = torch.from_numpy(rng.randn(3, 40, 199))
    v = torch.from_numpy(rng.rand(3, 40, 199) + 0.1)
    go = torch.from_numpy(rng.randn(3, 40, 67))
    lens = [40, 12, 33]
    fn = lambda a, b: AF.multi_stream_mlpg(a, b, w, SIZES, DYN, lens)  # noqa: E731
    for var in (v, v[0, 0].clone()):
        yc, gmc, gvc = _grads(fn, m, var, go)
        yg, gmg, gvg = _grads(fn, m.cuda(), var.cuda(), go)
        assert yc.device.type == "cpu" and gmc.device.type == "cpu" and gvc.device.type == "cpu"
        assert torch.equal(yc, yg.cpu()) and torch.equal(gmc, gmg.cpu()) and torch.equal(gvc, gvg.cpu())
    # 2-D input: the (T, D) form equals a batch of one
    f1 = lambda a, b: AF.multi_stream_mlpg(a, b, w, SIZES, DYN)  # noqa: E731
    y2, gm2, gv2 = _grads(f1, m[0].cuda(), v[0].cuda(), go[0])
    y3, gm3, gv3 = _grads(f1, m[:1].cuda(), v[:1].cuda(), go[:1])
    assert y2.shape == (40, 67) and torch.equal(y2, y3[0]) and torch.equal(gm2, gm3[0]) and torch.equal(gv2, gv3[0])
    # needs_input_grad: means only -- no variance work (kind 15 moves once, for the pass-through stream); variances only
    L = _hip.lib()
    mc, vc, gc = m.cuda(), v.cuda(), go.cuda()
    _, gm_both, gv_both = _grads(fn, mc, vc, gc)
    mm = mc.clone().requires_grad_()
    y = fn(mm, vc)
    torch.cuda.synchronize()
    k0 = L.mlpg_hip_launch_count(15)
    y.backward(gc)
    torch.cuda.synchronize()
    assert L.mlpg_hip_launch_count(15) == k0 + 1 and torch.equal(mm.grad, gm_both)
    vv = vc.clone().requires_grad_()
    y = fn(mc, vv)
    y.backward(gc)
    torch.cuda.synchronize()
    assert L.mlpg_hip_launch_count(15) == k0 + 3 and torch.equal(vv.grad, gv_both)       # one window list + the pass-through launch
    # error types as MLPGBatch
    with pytest.raises(TypeError):
        AF.multi_stream_mlpg(mc, vc.float(), w, SIZES, DYN)
    with pytest.raises(TypeError):
        AF.multi_stream_mlpg(mc.half(), vc.half(), w, SIZES, DYN)
    with pytest.raises(ValueError):
        AF.multi_stream_mlpg(mc, vc[:, :, :5], w, SIZES, DYN)
    with pytest.raises(ValueError):
        AF.multi_stream_mlpg(mc, vc, w, [180, 3, 1, 14], DYN)
    with pytest.raises(ValueError):
        AF.multi_stream_mlpg(mc, vc, w, SIZES, DYN, lengths=[40, 41, 2])
    vb = vc.clone()
    vb[1, 5:9, 181] = -1e-3                                    # lf0's delta variance
    monkeypatch.setattr(_mlpg, "CHECK_STATUS", True)
    with pytest.raises(np.linalg.LinAlgError):
        AF.multi_stream_mlpg(mc, vb, w, SIZES, DYN)
    mm, vv = mc.clone().requires_grad_(), vc.clone().requires_grad_()
    gm, gv = torch.autograd.grad((fn(mm, vv) * gc).sum(), (mm, vv), create_graph=True)
    with pytest.raises(RuntimeError):
        (gm.sum() + gv.sum()).backward()


def test_no_slicing_copies(monkeypatch):
    """Parent arrays of 256 MB and more, per-frame variances: the peak of forward + backward above what was allocated before
    stays below bytes(y) + bytes(grad_mean) + bytes(grad_var) + half of bytes(means) -- there is room for the three results and
    for no copy of a stream.  The composed form cannot meet that bound (asserted: the test proves what it claims)."""
    import torch
    from cases import WINDOW_SETS
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd.autograd import _mlpg
    monkeypatch.setattr(_mlpg, "CHECK_STATUS", False)
    w = WINDOW_SETS["std3"]
    B, T, D = 96, 1800, 199
    gen = torch.Generator(device="cuda").manual_seed(7)
    m = torch.randn(B, T, D, dtype=torch.float64, device="cuda", generator=gen).requires_grad_()
    v = (torch.rand(B, T, D, dtype=torch.float64, device="cuda", generator=gen) + 0.1).requires_grad_()
    go = torch.randn(B, T, 67, dtype=torch.float64, device="cuda", generator=gen)
    nbytes = m.numel() * 8
    assert nbytes >= 256 * 2 ** 20
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    budget = go.numel() * 8 + 2 * nbytes + nbytes // 2

    def peak(fn):
        m.grad = None
        v.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y = fn()
        y.backward(go)
        torch.cuda.synchronize()
        assert m.grad is not None and v.grad is not None
        return torch.cuda.max_memory_allocated() - before

    for _ in range(2):      # (the first pass creates the scratch of the solve routes, which the caching allocator does not see)
        p_in = peak(lambda: AF.multi_stream_mlpg(m, v, w, SIZES, DYN, lens))
    p_co = peak(lambda: _composed(m, v, w, lens))
    print("peak above the inputs: in place %d MB, composed %d MB, budget %d MB" % (p_in >> 20, p_co >> 20, budget >> 20))
    assert p_in < budget, (p_in, budget)
    assert p_co >= budget, (p_co, budget)


def test_graph_capture_replays_equal_eager(monkeypatch):
    """CHECK_STATUS off: forward + backward capture after one eager step on the capturing stream; two replays equal eager."""
    import torch
    from cases import WINDOW_SETS
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd.autograd import _mlpg
    monkeypatch.setattr(_mlpg, "CHECK_STATUS", False)
    w = WINDOW_SETS["std3"]
    rng = np.random.RandomState(8)
    B, T = 16, 500
    m0 = torch.from_numpy(rng.randn(B, T, 199))
    v0 = torch.from_numpy(rng.rand(B, T, 199) + 0.1)
    go = torch.from_numpy(rng.randn(B, T, 67)).cuda()
    lens = torch.from_numpy(rng.randint(0, T + 1, size=B).astype(np.int32)).cuda()
    for var in (v0, v0[0, 0].clone()):
        mc = m0.cuda().requires_grad_()
        vc = var.cuda().requires_grad_()

        def step():
            mc.grad = None
            vc.grad = None
            y = AF.multi_stream_mlpg(mc, vc, w, SIZES, DYN, lens)
            y.backward(go)
            return y

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            y_e = step()
            eager = (y_e.detach().clone(), mc.grad.clone(), vc.grad.clone())
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            y_g = step()
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y_g, eager[0]) and torch.equal(mc.grad, eager[1]) and torch.equal(vc.grad, eager[2]), var.dim()
