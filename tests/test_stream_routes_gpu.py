"""GPU tests (-m gpu): every route of mlpg_hip_forward_streams, driven through a raw stream table, against the C oracle.

_hip.forward_streams always writes the streams side by side in table order, so out_col, the status column and ld_out
coincide in every other test.  Here each layout puts its streams at permuted output columns with unused columns between
and beside them, in input and output rows, and ld_out > sum static_dim.  Before each call the output holds a NaN sentinel
of a fixed bit pattern and the status array 0x5A5A5A5A.  In every accepted cell:
- the return code is 0 and the launch counters move as tests/stream_plan.py predicts (exactly under a forced family; under
  AUTO the merged launch and the number of launches);
- every dynamic stream matches oracle.mlpg.mlpg_batch on its own slice, per utterance, within the forward bars;
- pass-through streams are bit copies on live frames, every stream column is exactly 0 past each length;
- every other output column keeps the sentinel bit for bit;
- every status cell is written: the oracle's verdict in the stream's table-order column, 0 for pass-through streams.
Some cells put a negative variance into one system of a merged member, a piece or a stream that runs alone.  Refused calls
leave counters, output and status untouched, and name the family that refused; calls stay ordered on the caller's stream and
replay bit-identically from a captured graph."""
import collections
import ctypes
import zlib

import numpy as np
import pytest

import stream_plan as SP
from cases import WINDOW_SETS

pytestmark = pytest.mark.gpu

SENT = {np.float64: 0x7FF4DEAD0000BEEF, np.float32: 0x7FC0DEAD}
STATUS_SENT = 0x5A5A5A5A
TOL = {np.float64: 1e-9, np.float32: 5e-6}
_MOVED = collections.Counter()          # launches per counter kind over the whole file (test_every_forward_kind_was_reached)


class Layout(object):
    """A raw stream table.  spec: [(static_dim, window-set name or None)]; a name "std3#x" is a separate table entry with
    the values of std3, "std3#ulp" the same with its last coefficient one ulp larger.  Input columns start at 2 with a gap
    of 1-2 after each stream; output columns follow a permutation of the streams with gaps of 1, from column 1 on."""

    def __init__(self, spec, seed):
        rng = np.random.RandomState(seed)
        wl, wu, wc, first = [], [], [], {}
        self.streams = []
        col = 2
        for sd, name in spec:
            nw, f = 0, 0
            if name is not None:
                base = WINDOW_SETS[name.split("#")[0]]
                if name not in first:
                    first[name] = len(wl)
                    for l, u, c in base:
                        c = np.asarray(c, dtype=np.float64).ravel().copy()
                        wl.append(l)
                        wu.append(u)
                        wc.extend(c.tolist())
                    if name.endswith("#ulp"):
                        wc[-1] = float(np.nextafter(wc[-1], np.inf))
                nw, f = len(base), first[name]
            self.streams.append(dict(in_col=col, out_col=0, static_dim=sd, num_windows=nw, win_first=f))
            col += max(nw, 1) * sd + 1 + (len(self.streams) % 2)
        self.ld_in = col + 1
        oc = 1
        for k in rng.permutation(len(spec)):
            self.streams[k]["out_col"] = oc
            oc += self.streams[k]["static_dim"] + 1
        self.ld_out = oc + 2
        self.wl = np.array(wl or [0], dtype=np.int32)
        self.wu = np.array(wu or [0], dtype=np.int32)
        self.wc = np.array(wc or [0.0], dtype=np.float64)
        self.n_win = len(wl)
        self.stat_col = np.cumsum([0] + [s["static_dim"] for s in self.streams])[:-1].tolist()
        self.sd_total = sum(s["static_dim"] for s in self.streams)

    def windows_of(self, s):
        off = sum(int(self.wl[w]) + int(self.wu[w]) + 1 for w in range(s["win_first"]))
        res = []
        for w in range(s["win_first"], s["win_first"] + s["num_windows"]):
            n = int(self.wl[w]) + int(self.wu[w]) + 1
            res.append((int(self.wl[w]), int(self.wu[w]), self.wc[off:off + n].copy()))
            off += n
        return res

    def in_cols(self, s):
        return np.arange(s["in_col"], s["in_col"] + max(s["num_windows"], 1) * s["static_dim"])

    def predict(self, algo, mode, dtype, B, T, has_lengths):
        return SP.predict(self.streams, self.wl, self.wu, self.wc, algo, mode, SP.F32 if dtype == np.float32 else SP.F64,
                          B, T, self.ld_in, self.ld_out, has_lengths)


LAYOUTS = {
    "merlin": [(60, "std3"), (1, "std3"), (1, None), (5, "std3")],          # mgc | lf0 | vuv | bap
    "two60_10": [(60, "std3"), (60, "std3"), (10, "std3")],                 # cap 128, a piece of 2
    "sixty_4x1": [(60, "std3")] + [(1, "std3")] * 4,                        # 4 members, the fifth alone
    "sixty_forty": [(60, "std3"), (40, "std3")],                            # two groups, no trim
    "thirty_twenty": [(30, "std3"), (20, "std3")],
    "eq_copy": [(30, "std3"), (20, "std3#copy")],                           # equal values, distinct entries: merged
    "eq_ulp": [(30, "std3"), (20, "std3#ulp")],                             # one ulp apart: not merged
    "mixed": [(8, "std3"), (6, "wide3"), (4, "asym2"), (3, "static"), (5, "zero2"), (2, None)],
    "mixed_ext1": [(8, "std3"), (4, "asym2"), (3, "static"), (5, "zero2"), (2, None)],
    "zero_dim": [(40, "std3"), (0, "std3"), (3, None), (0, None), (20, "std3")],
    "ones64": [(1, "std3" if k % 4 else None) for k in range(64)],
    "slice_std3": [(40, "std3")],
    "slice_wide3": [(24, "wide3")],
}
_LAY = {}


def layout(name):
    if name not in _LAY:
        _LAY[name] = Layout(LAYOUTS[name], zlib.crc32(name.encode()) & 0xFFFF)
    return _LAY[name]


def _counts():
    from nnmnkwii_amd import _hip
    return {k: _hip.lib().mlpg_hip_launch_count(k) for k in SP.FORWARD_KINDS}


def _int_view(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def drive(lay, M, V, mode, L, algo, streams=None, ld_out=None):
    """One raw mlpg_hip_forward_streams call on the current torch stream.  Returns (rc, out, status, counter deltas, error
    text); out (B, T, ld_out) starts as the NaN sentinel, status (B, sum static_dim) as 0x5A5A5A5A.  Synchronises after."""
    import torch
    from nnmnkwii_amd import _hip
    streams = lay.streams if streams is None else streams
    ld_out = lay.ld_out if ld_out is None else ld_out
    B, T, ld_in = M.shape
    table = (_hip.StreamDesc * max(len(streams), 1))()
    for k, s in enumerate(streams):
        table[k] = _hip.StreamDesc(s["in_col"], s["out_col"], s["static_dim"], s["num_windows"], s["win_first"])
    dt = np.float64 if M.dtype == torch.float64 else np.float32
    it = torch.int64 if dt == np.float64 else torch.int32
    out = torch.full((B, T, ld_out), SENT[dt], dtype=it, device=M.device).view(M.dtype)
    sd_total = sum(s["static_dim"] for s in streams)
    status = torch.full((B, max(sd_total, 1)), STATUS_SENT, dtype=torch.int32, device=M.device)
    c0 = _counts()
    rc = _hip.lib().mlpg_hip_forward_streams(M.device.index, _hip._stream(M.device), _hip._dt(M), algo, _hip._p(M), _hip._p(V),
                                             mode, ld_in, _hip._p(L), B, T, len(streams), ctypes.addressof(table), lay.n_win,
                                             _hip._np(lay.wl), _hip._np(lay.wu), _hip._np(lay.wc), _hip._p(out), ld_out,
                                             _hip._p(status))
    err = _hip.lib().mlpg_hip_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    moved = {k: n - c0[k] for k, n in _counts().items() if n != c0[k]}
    _MOVED.update(moved)
    return rc, out, status, moved, err


def _warm_fir(lay):
    """The FIR form builds its tap table on first use per window set (one natural-order solve): build every table of the
    layout before a cell counts launches."""
    import torch
    from nnmnkwii_amd import _hip
    for s in lay.streams:
        if s["num_windows"]:
            try:
                _hip.forward(torch.zeros((1, 96, s["num_windows"]), dtype=torch.float32, device="cuda"), None, lay.windows_of(s),
                             algo=_hip.ALGO_FIR)
            except _hip.HipExtensionError:
                pass                            # a window set the FIR form does not serve: AUTO takes another kernel
    torch.cuda.synchronize()


def _ragged(B, T, rng):
    head = np.array([T, max(T - 1, 0), 1, 0], dtype=np.int32)
    return np.concatenate([head, rng.randint(0, T + 1, size=B - 4)]).astype(np.int32)[:B]


def make_inputs(lay, dt, mode, B, T, ragged, seed):
    """Means (B, T, ld_in) and variances per mode; unused input columns (and global-vector entries) are NaN."""
    rng = np.random.RandomState(seed)
    used = np.zeros(lay.ld_in, dtype=bool)
    for s in lay.streams:
        used[lay.in_cols(s)] = True
    M = rng.randn(B, T, lay.ld_in).astype(dt)
    M[:, :, ~used] = np.nan
    V = None
    if mode == SP.VAR_FRAME:
        V = (rng.rand(B, T, lay.ld_in) + 0.1).astype(dt)
        V[:, :, ~used] = np.nan
    elif mode == SP.VAR_GLOBAL:
        V = (rng.rand(lay.ld_in) + 0.1).astype(dt)
        V[~used] = np.nan
    lens = _ragged(B, T, rng) if ragged else None
    return M, V, lens


def _poison(lay, V, mode, lens, poisons):
    """A negative static-window variance in system (stream k, dim d): one live frame of utterance 1 (per-frame variances)
    or the global entry (every utterance)."""
    Vp = V.copy()
    for k, d in poisons:
        c = lay.streams[k]["in_col"] + d
        if mode == SP.VAR_GLOBAL:
            Vp[c] = -0.5
        else:
            b = 1 if Vp.shape[0] > 1 else 0
            n = Vp.shape[1] if lens is None else int(lens[b])
            assert n > 0
            Vp[b, n // 2, c] = -1e-3
    return Vp


def check_outputs(lay, M, V, Vp, mode, lens, out, status, dt, poisons=()):
    """Every assertion of an accepted cell on the whole batch; the oracle on a few utterances of a large one."""
    from oracle import mlpg as O
    B, T, _ = M.shape
    lens_a = np.full(B, T, dtype=np.int32) if lens is None else lens
    live = np.arange(T)[None, :] < lens_a[:, None]
    sel = np.arange(B) if B <= 8 else np.unique(np.r_[0:4, B // 2, B - 1])
    exp_status = np.zeros((B, lay.sd_total), dtype=np.int32)
    owned = np.zeros(out.shape[2], dtype=bool)
    bad = {}
    # the poisoned systems alone, on every utterance: the oracle's k and a zero column where it fails
    for k, d in poisons:
        s = lay.streams[k]
        w = lay.windows_of(s)
        cols = [s["in_col"] + j * s["static_dim"] + d for j in range(len(w))]
        v1 = Vp[cols] if mode == SP.VAR_GLOBAL else np.ascontiguousarray(Vp[:, :, cols])
        r1, st1, _ = O.mlpg_batch(np.ascontiguousarray(M[:, :, cols]), v1, w, lens)
        assert (st1[lens_a > 0, 0] > 0).any(), ("poison did not fail", k, d)
        exp_status[:, lay.stat_col[k] + d] = st1[:, 0]
        bad[(k, d)] = r1[:, :, 0]
        got = out[:, :, s["out_col"] + d]
        assert not got[st1[:, 0] != 0].any(), ("failed system's column not zero", k, d)
        ok = st1[:, 0] == 0
        scale = np.abs(r1[ok, :, 0]).max(axis=1) if ok.any() else np.zeros(0)
        err = np.abs(got[ok].astype(np.float64) - r1[ok, :, 0]).max(axis=1) if ok.any() else np.zeros(0)
        assert (err <= TOL[dt] * scale).all(), ("poisoned stream's other utterances", k, d)
    for k, s in enumerate(lay.streams):
        sd, oc = s["static_dim"], s["out_col"]
        if sd == 0:
            continue
        owned[oc:oc + sd] = True
        got = out[:, :, oc:oc + sd]
        assert not got[~live].any(), ("padding not zero", k)
        if s["num_windows"] == 0:
            src = M[:, :, s["in_col"]:s["in_col"] + sd]
            assert np.array_equal(_int_view(got[live]), _int_view(src[live])), ("pass-through not a bit copy", k)
            continue
        w = lay.windows_of(s)
        cols = lay.in_cols(s)
        ms = np.ascontiguousarray(M[sel][:, :, cols])
        vs = {SP.VAR_FRAME: lambda: np.ascontiguousarray(V[sel][:, :, cols]), SP.VAR_GLOBAL: lambda: V[cols],
              SP.VAR_UNIT: lambda: np.ones(len(cols), dtype=dt)}[mode]()
        ref, st, rc = O.mlpg_batch(ms, vs, w, None if lens is None else lens[sel])
        assert rc == 0, ("oracle failed on clean data", k)
        ref = ref.astype(np.float64)
        for (kk, d), r1 in bad.items():
            if kk == k:
                ref[:, :, d] = r1[sel]
        g = got[sel].astype(np.float64)
        err = np.abs(g - ref).max(axis=(1, 2))
        scale = np.abs(ref).max(axis=(1, 2))
        assert (err <= TOL[dt] * scale).all(), ("trajectory", k, (err / np.where(scale > 0, scale, 1)).tolist())
    rest = _int_view(out[:, :, ~owned])
    assert (rest == SENT[dt]).all(), ("a column outside the streams was written",
                                      sorted(set(np.nonzero(~owned)[0][np.nonzero((rest != SENT[dt]).any(axis=(0, 1)))[0]])))
    assert not (status == STATUS_SENT).any(), ("status cells left unwritten", np.argwhere(status == STATUS_SENT)[:4].tolist())
    assert np.array_equal(status, exp_status), ("status", np.argwhere(status != exp_status)[:4].tolist())


def check_counters(lay, moved, algo, mode, dt, B, T, has_lengths):
    plan, kinds, n = lay.predict(algo, mode, dt, B, T, has_lengths)
    assert set(moved) <= set(SP.FORWARD_KINDS), moved
    assert sum(moved.values()) == n, ("launches", moved, n, plan)
    merged_kind = SP.K_STRIP_MULTI if mode == SP.VAR_FRAME else SP.K_CONST_MULTI
    assert moved.get(merged_kind, 0) == int(plan.merged), ("merged launch", moved, plan)
    if kinds is not None:
        assert moved == dict(kinds), ("kinds", moved, dict(kinds), plan)
    return plan


def run_cell(lname, dt, mode, ragged, algo, T, B, poisons=()):
    import torch
    lay = layout(lname)
    seed = zlib.crc32(repr((lname, dt.__name__, mode, ragged, algo, T, B)).encode()) & 0x7FFFFFFF
    M, V, lens = make_inputs(lay, dt, mode, B, T, ragged, seed)
    Vp = _poison(lay, V, mode, lens, poisons) if poisons else V
    if dt == np.float32 and mode == SP.VAR_UNIT and not ragged:
        _warm_fir(lay)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rc, out, status, moved, err = drive(lay, dev(M), dev(Vp), mode, dev(lens), algo)
    assert rc == 0, err
    plan = check_counters(lay, moved, algo, mode, dt, B, T, ragged)
    check_outputs(lay, M, V, Vp, mode, lens, out.cpu().numpy(), status.cpu().numpy(), dt, poisons)
    return plan, moved


F, G, U = SP.VAR_FRAME, SP.VAR_GLOBAL, SP.VAR_UNIT
f64, f32 = np.float64, np.float32
# (layout, dtype, variances, ragged lengths, algo, T, B, poisoned systems (stream, dim))
CELLS = [
    # forced strip kernel, per-frame variances: the merged launch (kind 3) and every route of a piece or a lone stream
    ("merlin", f64, F, True, SP.STRIP, 300, 6, [(0, 5), (3, 4)]),      # bap's piece (dims 3-4): transposed form
    ("merlin", f32, F, False, SP.STRIP, 65, 1, [(3, 3)]),              # one utterance: the piece on the wave kernel
    ("merlin", f64, F, False, SP.STRIP, 2100, 1, []),                  # > 2048 frames: the piece on the natural-order kernel
    ("two60_10", f64, F, True, SP.STRIP, 300, 6, [(2, 9), (1, 0)]),
    ("two60_10", f32, F, True, SP.STRIP, 1100, 6, []),
    ("sixty_4x1", f32, F, True, SP.STRIP, 65, 6, [(4, 0), (1, 0)]),     # the fifth stream alone, a member
    ("sixty_forty", f64, F, False, SP.STRIP, 2, 6, []),
    ("thirty_twenty", f32, F, True, SP.STRIP, 1, 6, []),
    ("eq_copy", f64, F, True, SP.STRIP, 300, 6, []),
    ("eq_ulp", f64, F, True, SP.STRIP, 300, 6, []),
    ("zero_dim", f64, F, True, SP.STRIP, 65, 6, []),
    ("ones64", f32, F, True, SP.STRIP, 65, 6, []),
    ("mixed_ext1", f64, F, True, SP.STRIP, 300, 6, [(1, 2)]),
    # forced constant-coefficient kernel, global / unit variances: the merged launch (kind 8); pieces go to AUTO's choice
    ("merlin", f64, G, True, SP.CONST, 300, 6, [(0, 7), (3, 3)]),      # bap dim 3: in the piece
    ("merlin", f32, U, False, SP.CONST, 1100, 192, []),                # the piece on the transposed form
    ("two60_10", f64, U, True, SP.CONST, 65, 6, []),
    ("sixty_4x1", f64, G, False, SP.CONST, 2, 1, [(4, 0)]),
    ("sixty_forty", f32, G, True, SP.CONST, 300, 6, []),
    ("eq_copy", f64, G, True, SP.CONST, 65, 6, []),
    ("eq_ulp", f64, G, True, SP.CONST, 65, 6, []),
    ("zero_dim", f32, U, True, SP.CONST, 300, 6, []),
    ("ones64", f64, G, True, SP.CONST, 65, 6, []),
    ("slice_std3", f64, G, True, SP.CONST, 65, 6, [(0, 39)]),
    # the other forced families
    ("mixed_ext1", f64, F, True, SP.WAVE, 300, 6, [(0, 2)]),
    ("mixed_ext1", f32, G, True, SP.WAVE, 2, 6, []),
    ("mixed", f64, F, True, SP.GENERIC, 65, 6, [(1, 3)]),
    ("mixed", f32, U, False, SP.GENERIC, 2100, 1, []),
    ("slice_wide3", f64, F, True, SP.CHUNK, 300, 6, [(0, 5)]),
    ("slice_wide3", f32, U, False, SP.CHUNK, 65, 6, []),
    ("slice_std3", f32, U, False, SP.FIR, 300, 6, []),
    ("merlin", f32, U, False, SP.FIR, 300, 6, []),
    # AUTO
    ("merlin", f64, F, True, SP.AUTO, 1100, 6, [(0, 1), (3, 4)]),
    ("merlin", f32, G, False, SP.AUTO, 300, 192, []),
    ("merlin", f32, U, False, SP.AUTO, 300, 6, []),
    ("mixed", f64, F, True, SP.AUTO, 300, 6, [(2, 1)]),
    ("mixed", f32, U, False, SP.AUTO, 300, 6, []),
    ("ones64", f64, G, True, SP.AUTO, 65, 6, []),
    ("zero_dim", f32, F, True, SP.AUTO, 2100, 6, []),
    ("two60_10", f32, F, False, SP.AUTO, 2100, 6, []),
    ("slice_std3", f32, U, False, SP.AUTO, 300, 6, []),
    ("slice_wide3", f64, F, True, SP.AUTO, 300, 16, []),
    ("eq_copy", f64, G, True, SP.AUTO, 65, 192, []),
    ("sixty_4x1", f64, F, True, SP.AUTO, 65, 256, []),
]
_ALGO = {0: "auto", 1: "generic", 2: "wave", 3: "strip", 5: "const", 6: "chunk", 7: "fir"}
_MODE = {F: "frame", G: "global", U: "unit"}


def _cell_id(c):
    return "%s-%s-%s-%s-%s-T%d-B%d%s" % (c[0], c[1].__name__, _MODE[c[2]], "ragged" if c[3] else "full", _ALGO[c[4]], c[5], c[6],
                                         "-neg" if c[7] else "")


@pytest.mark.parametrize("cell", CELLS, ids=[_cell_id(c) for c in CELLS])
def test_stream_route_cell(cell):
    run_cell(*cell)


def _sweep():
    """Forced families over more layouts, both dtypes, every variance mode, short and long utterances, one and six
    utterances: every combination the plan accepts (a refusal is the refusal tests' business)."""
    cells = []
    for lname in ("merlin", "two60_10", "sixty_4x1", "zero_dim", "mixed_ext1", "eq_copy"):
        for algo in (SP.STRIP, SP.CONST, SP.WAVE, SP.GENERIC):
            for mode in (F, G, U):
                for dt in (f64, f32):
                    for T, B in ((2, 6), (65, 1), (300, 6), (1100, 6)):
                        ragged = B >= 4
                        try:
                            layout(lname).predict(algo, mode, dt, B, T, ragged)
                        except SP.Refused:
                            continue
                        cells.append((lname, dt, mode, ragged, algo, T, B, []))
    return cells


SWEEP = _sweep()


@pytest.mark.parametrize("cell", SWEEP, ids=[_cell_id(c) for c in SWEEP])
def test_stream_route_sweep(cell):
    run_cell(*cell)


def test_merged_launch_members_and_pieces_as_planned():
    """The cells' plans cover what the matrix is for: merges of 2, 3 and 4 members, a trimmed launch with a piece, a
    piece on each of its three kernels, and more lone streams than side streams."""
    plans = {}
    for c in CELLS:
        plan, _, _ = layout(c[0]).predict(c[4], c[2], c[1], c[6], c[5], c[3])
        plans[_cell_id(c)] = plan
    assert {len(p.members) for p in plans.values() if p.merged} >= {2, 3, 4}
    assert any(p.merged and p.cap == 128 and p.piece >= 0 for p in plans.values())
    assert any(len(p.alone) > 3 for p in plans.values())
    assert not plans[_cell_id(CELLS[9])].merged and plans[_cell_id(CELLS[8])].merged      # one ulp apart / equal values


# ---------------------------------------------------------------------------------------------------- refusals

def _untouched(out, status, dt):
    return (_int_view(out.cpu().numpy()) == SENT[dt]).all() and (status.cpu().numpy() == STATUS_SENT).all()


def test_refused_tables_launch_nothing_and_touch_nothing():
    import torch
    lay = layout("ones64")
    M, V, lens = make_inputs(lay, f64, F, 6, 65, True, 5)
    Md, Vd, Ld = (torch.from_numpy(a).cuda() for a in (M, V, lens))
    # 64 streams are accepted, 65 are not
    rc, out, status, moved, err = drive(lay, Md, Vd, F, Ld, SP.STRIP)
    assert rc == 0, err
    s65 = lay.streams + [dict(lay.streams[1])]
    rc, out, status, moved, err = drive(lay, Md, Vd, F, Ld, SP.STRIP, streams=s65)
    assert rc == -1 and "64 streams" in err and moved == {} and _untouched(out, status, f64), (rc, err, moved)
    # a stream that does not fit the output row, or the input row
    lay = layout("merlin")
    M, V, lens = make_inputs(lay, f32, F, 6, 300, True, 6)
    Md, Vd, Ld = (torch.from_numpy(a).cuda() for a in (M, V, lens))
    for field, value in (("out_col", lay.ld_out - 4), ("in_col", lay.ld_in - 14)):
        bad = [dict(s) for s in lay.streams]
        bad[3][field] = value                                # bap: 5 dims, 15 input columns
        rc, out, status, moved, err = drive(lay, Md, Vd, F, Ld, SP.AUTO, streams=bad)
        assert rc == -1 and "does not fit" in err and moved == {} and _untouched(out, status, f32), (field, rc, err, moved)


@pytest.mark.parametrize("lname,mode,ragged,algo", [
    ("mixed", F, True, SP.WAVE),            # wide3: extent 2
    ("mixed", F, True, SP.STRIP),
    ("mixed", G, True, SP.CONST),           # wide3, static, zero2
    ("merlin", F, True, SP.CONST),          # per-frame variances
    ("merlin", U, True, SP.FIR),            # a lengths vector
    ("mixed_ext1", F, True, SP.CHUNK),      # std3: extent 1 is fine, static / zero2 have none
])
def test_forced_family_refusal_names_the_family_and_leaves_the_stream_usable(lname, mode, ragged, algo):
    """A family one stream of the call cannot take: EINVAL naming the family, before anything is enqueued -- no counter moves,
    output and status keep their sentinels.  The next valid call on the same torch stream is correct (no fork or join event
    left dangling)."""
    import torch
    lay = layout(lname)
    dt = f64
    with pytest.raises(SP.Refused) as ei:
        lay.predict(algo, mode, dt, 6, 300, ragged)
    M, V, lens = make_inputs(lay, dt, mode, 6, 300, ragged, 7)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc, out, status, moved, err = drive(lay, dev(M), dev(V), mode, dev(lens), algo)
        assert rc == -1 and str(ei.value) in err, (rc, err)
        assert moved == {} and _untouched(out, status, dt), (err, moved)
        rc, out, status, moved, err = drive(lay, dev(M), dev(V), mode, dev(lens), SP.AUTO)
        assert rc == 0, err
    check_counters(lay, moved, SP.AUTO, mode, dt, 6, 300, ragged)
    check_outputs(lay, M, V, V, mode, lens, out.cpu().numpy(), status.cpu().numpy(), dt)


# ---------------------------------------------------------------------------------------------------- ordering and capture

def _call_async(lay, M, V, mode, L, algo, out, status):
    from nnmnkwii_amd import _hip
    table = (_hip.StreamDesc * len(lay.streams))()
    for k, s in enumerate(lay.streams):
        table[k] = _hip.StreamDesc(s["in_col"], s["out_col"], s["static_dim"], s["num_windows"], s["win_first"])
    B, T, ld_in = M.shape
    rc = _hip.lib().mlpg_hip_forward_streams(M.device.index, _hip._stream(M.device), _hip._dt(M), algo, _hip._p(M), _hip._p(V), mode,
                                             ld_in, _hip._p(L), B, T, len(lay.streams), ctypes.addressof(table), lay.n_win,
                                             _hip._np(lay.wl), _hip._np(lay.wu), _hip._np(lay.wc), _hip._p(out), lay.ld_out,
                                             _hip._p(status))
    assert rc == 0, _hip.lib().mlpg_hip_last_error().decode()


LAY_SIDE = [(60, "std3"), (1, "std3"), (1, None), (5, "std3"), (4, "wide3"), (3, "asym2")]


def test_side_stream_work_is_ordered_on_the_callers_stream():
    """Lone streams on the internal side streams, a merged launch on the caller's non-default stream; a clone queued on
    that stream right behind the call, with no host synchronisation, sees every column."""
    import torch
    lay = Layout(LAY_SIDE, 11)
    B, T = 32, 1100
    plan, _, _ = lay.predict(SP.AUTO, F, f64, B, T, True)
    assert plan.merged and len(plan.alone) > 3                       # more lone streams than side streams
    M, V, lens = make_inputs(lay, f64, F, B, T, True, 12)
    Md, Vd, Ld = (torch.from_numpy(a).cuda() for a in (M, V, lens))
    out = torch.zeros((B, T, lay.ld_out), dtype=torch.float64, device="cuda")
    status = torch.full((B, lay.sd_total), STATUS_SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            _call_async(lay, Md, Vd, F, Ld, SP.AUTO, out, status)
            snap, ssnap = out.clone(), status.clone()
            out.zero_()
            status.fill_(STATUS_SENT)
    torch.cuda.synchronize()
    _call_async(lay, Md, Vd, F, Ld, SP.AUTO, out, status)
    torch.cuda.synchronize()
    assert torch.equal(snap.view(torch.int64), out.view(torch.int64)) and torch.equal(ssnap, status)


def test_graph_capture_with_side_streams_and_a_merged_launch_replays_bit_identically():
    import torch
    lay = Layout(LAY_SIDE, 13)
    B, T = 4, 1100
    plan, _, _ = lay.predict(SP.AUTO, F, f64, B, T, True)
    assert plan.merged
    M, V, lens = make_inputs(lay, f64, F, B, T, True, 14)
    Md, Vd, Ld = (torch.from_numpy(a).cuda() for a in (M, V, lens))
    out = torch.full((B, T, lay.ld_out), SENT[f64], dtype=torch.int64, device="cuda").view(torch.float64)
    status = torch.full((B, lay.sd_total), STATUS_SENT, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call_async(lay, Md, Vd, F, Ld, SP.AUTO, out, status)           # warm the scratch of every stream the call uses
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _call_async(lay, Md, Vd, F, Ld, SP.AUTO, out, status)
    torch.cuda.synchronize()
    for seed in (15, 16):
        M2, V2, _ = make_inputs(lay, f64, F, B, T, True, seed)
        V2p = _poison(lay, V2, F, lens, [(0, 3)])                       # a failing system of a merged member
        Md.copy_(torch.from_numpy(M2))
        Vd.copy_(torch.from_numpy(V2p))
        status.fill_(STATUS_SENT)
        g.replay()
        torch.cuda.synchronize()
        rc, ref, sref, _, err = drive(lay, Md, Vd, F, Ld, SP.AUTO)
        assert rc == 0, err
        assert torch.equal(out.view(torch.int64), ref.view(torch.int64)) and torch.equal(status, sref), seed
        check_outputs(lay, M2, V2, V2p, F, lens, out.cpu().numpy(), status.cpu().numpy(), f64, [(0, 3)])


# ---------------------------------------------------------------------------------------------------- the user-facing call

@pytest.mark.parametrize("mode", ["frame", "global"])
def test_multi_stream_mlpg_merges_equal_window_lists_not_ulp_apart_ones(mode):
    """paramgen.multi_stream_mlpg with one window list per stream, equal in value but distinct objects: merged where AUTO
    merges (a long utterance with per-frame variances, 192 utterances with global ones).  One coefficient one ulp larger
    in one list: not merged.  Both match the oracle."""
    import copy
    from nnmnkwii_amd import paramgen as G
    from oracle import mlpg as O
    std3 = WINDOW_SETS["std3"]
    B, T = (2, 1100) if mode == "frame" else (192, 100)
    sizes, dyn = [180, 3, 1, 15], [True, True, False, True]
    rng = np.random.RandomState(21)
    X = rng.randn(B, T, 199)
    Vf = rng.rand(B, T, 199) + 0.1
    var = Vf if mode == "frame" else Vf[0, 0].copy()
    lens = np.array([T, T - 7] + [T] * (B - 2), dtype=np.int32)
    ulp_a, ulp_b = copy.deepcopy(std3), copy.deepcopy(std3)
    ulp_a[2] = (1, 1, np.array([1.0, -2.0, np.nextafter(1.0, 2.0)]))
    ulp_b[1] = (1, 1, np.array([np.nextafter(-0.5, 0.0), 0.0, 0.5]))
    kind = 3 if mode == "frame" else 8
    for lists, merged in (([copy.deepcopy(std3) for _ in range(4)], True), ([std3, ulp_a, None, ulp_b], False)):
        c0 = _counts()
        y = G.multi_stream_mlpg(X, var, lists, sizes, dyn, lengths=lens)
        c1 = _counts()
        assert c1[kind] - c0[kind] == int(merged), (mode, merged)
        col, oc = 0, 0
        for size, d, w in zip(sizes, dyn, lists):
            if d:
                sd = size // 3
                v = np.ascontiguousarray(Vf[:2, :, col:col + size]) if mode == "frame" else var[col:col + size]
                ref, _, rc = O.mlpg_batch(np.ascontiguousarray(X[:2, :, col:col + size]), v, w, lens[:2])
                assert rc == 0
                got = y[:2, :, oc:oc + sd]
                assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (mode, merged, size)
            else:
                sd = size
                assert np.array_equal(y[:2, :lens[1], oc], X[:2, :lens[1], col])
            col += size
            oc += sd


def test_every_forward_kind_was_reached():
    """The file as a whole: every forward launch counter kind moved (0 natural-order, 1 wave, 2 strip, 3 strip merged,
    4 constant-coefficient, 6 chunked, 7 FIR, 8 constant-coefficient merged, 9 transposed strip)."""
    print("launches per counter kind:", dict(sorted(_MOVED.items())))
    missing = [k for k in SP.FORWARD_KINDS if _MOVED[k] == 0]
    assert not missing, (missing, dict(_MOVED))
