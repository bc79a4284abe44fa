"""GPU tests (-m gpu): the entries that take a row stride, on a parent of few rows and a huge row stride (tests/far.py), so that
the rows the call reads and writes lie on both sides of 2^31 bytes and 2^32 bytes (float32: of 2^31 elements too) from the pointer
it is given.  Tmax = 130 (three 64-frame strips, the last of two frames) and ld = 2064888: 130 * 2064888 * 8 = 2^31 - 128, the
largest stride rows_fit_buffer (csrc/common.h) lets into the strip, constant-coefficient, chunked and FIR kernels' 2 GB buffer
window.  In float64 utterance b starts at b * (2^31 - 128) bytes, so row 0 of utterance 1 straddles 2^31 bytes inside its first 16
columns and row 0 of utterance 2 straddles 2^32 bytes inside its first 32; in float32 nine utterances of 2^30 - 64 bytes reach
2^33 bytes = 2^31 elements.  Streams are placed from column 0 (live data on both sides of the boundaries, mid-row) and at the end
of the row (t * ld + col large).

Only one array of a call is wide, the others are dense and small; where an entry takes two arrays of one layout the second
pointer is the parent's own, a few hundred columns in.  After each call FarParent.untouched() checks that every byte of the
parent outside the rows the call may write is what it was.  Each entry is compared with the reference and the bound of its
own GPU test, imported from there; where the header promises that a row's bits do not depend on the rest of the batch, also bit
for bit with the same call on a compact copy of the live rows.  The last test prints which boundaries each array argument
crossed and fails unless every one crossed all of them."""
import collections
import ctypes
import functools
import gc
import os
import sys
import zlib

import numpy as np
import pytest
import torch

import far
import stream_plan as SP
import test_stream_routes_gpu as R
from far import FarParent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
T, LD = 130, 2064888
LD_OVER = LD + 1                                    # 130 * 2064889 * 8 = 2^31 - 128 + 1040: the other side of the rule
BATCH = {F64: 3, F32: 9}
LENS = {3: [130, 67, 1], 9: [130, 67, 1, 130, 0, 65, 64, 129, 130]}
SHIFT = 512                                         # columns between two arrays of one layout that share a parent
BYTES = ("2^31 bytes", "2^32 bytes")
COVER = collections.defaultdict(set)                # (entry, array argument, dtype) -> boundaries crossed


def far_test(fn):
    """Peak device memory of the test stays under far.MEM_CAP; whatever it allocated is handed back at its end."""
    @functools.wraps(fn)
    def run(*a, **kw):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        try:
            fn(*a, **kw)
            peak = torch.cuda.max_memory_allocated()
        finally:
            gc.collect()
            torch.cuda.empty_cache()
        assert peak <= far.MEM_CAP, "peak device memory %.2f GiB" % (peak / 2.0 ** 30)
    return run


def wide_parent(dt, ld=LD, B=None, other_bytes=0):
    B = BATCH[dt] if B is None else B
    nbytes = B * T * ld * np.dtype(dt).itemsize
    return FarParent((B, T, ld), dt, low_guard_bytes=far.low_guard_for(nbytes, other_bytes))


def lengths_of(B, with_lengths):
    return np.array(LENS[B] if with_lengths else [T] * B, dtype=np.int32)


def put(parent, X, lens, col):
    """The live rows of the compact (B, T, w) array X into the parent from column col on."""
    for b, n in enumerate(lens):
        if n:
            parent.place(b, int(n), col, X[b, :n])


def expect(parent, col, width):
    for b in range(parent.B):
        parent.expect_written(b, T, col, width)


def get(parent, col, width):
    return np.stack([parent.read(b, T, col, width) for b in range(parent.B)])


def note(entry, arg, parent, dt, col0=0):
    got = parent.crossed(col0)
    COVER[(entry, arg, np.dtype(dt).name)] |= got
    return got


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def _counts(n=44):
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return [L.mlpg_hip_launch_count(k) for k in range(n)]


def _moved(c0):
    return {k: b - a for k, (a, b) in enumerate(zip(c0, _counts())) if a != b}


# ---------------------------------------------------------------------------------------------------- mlpg_hip_forward_streams

F, G, U = SP.VAR_FRAME, SP.VAR_GLOBAL, SP.VAR_UNIT
# family -> (stream table, algo, variances): a table the family accepts, whose plan is the launch the name says
FAMILIES = {
    "strip": ([(40, "std3"), (34, "std3#ulp")], SP.STRIP, F),                    # one ulp apart: two launches of their own
    "strip_merged": ([(40, "std3"), (24, "std3")], SP.STRIP, F),
    "const": ([(40, "std3"), (34, "std3#ulp")], SP.CONST, G),
    "const_merged": ([(40, "std3"), (24, "std3")], SP.CONST, U),
    "chunk": ([(24, "wide3"), (10, "wide3")], SP.CHUNK, F),
    "fir": ([(40, "std3"), (10, "std3")], SP.FIR, U),
    "wave": (R.LAYOUTS["mixed_ext1"], SP.WAVE, F),
    "generic": (R.LAYOUTS["mixed"], SP.GENERIC, G),
    "auto": (R.LAYOUTS["merlin"], SP.AUTO, F),
}
EXPECTED_KINDS = {"strip": {SP.K_STRIP: 2}, "strip_merged": {SP.K_STRIP_MULTI: 1}, "const": {SP.K_CONST: 2},
                  "const_merged": {SP.K_CONST_MULTI: 1}, "chunk": {SP.K_CHUNK: 2}, "fir": {SP.K_FIR: 2}, "wave": {SP.K_WAVE: 4},
                  "generic": {SP.K_GENERIC: 5}}


class WideLayout(object):
    """A stream table of tests/test_stream_routes_gpu.py with its dense columns (.dense) and the same streams moved into a row of
    `ld` elements on one side: the first streams from column 0 on, the last one at the row's end (`shift` columns short of it on
    the input side, where the variances follow the means in the same parent)."""

    def __init__(self, spec, side, ld, shift):
        self.dense = R.Layout(spec, zlib.crc32(repr(spec).encode()) & 0xFFFF)
        d = self.dense
        self.streams = [dict(s) for s in d.streams]
        self.ld_in, self.ld_out = d.ld_in, d.ld_out
        live = [k for k, s in enumerate(self.streams) if s["static_dim"] > 0]
        col = 0
        for k in live:
            s = self.streams[k]
            width = max(s["num_windows"], 1) * s["static_dim"] if side == "in" else s["static_dim"]
            at = col if k != live[-1] or len(live) == 1 else ld - width - shift
            s["in_col" if side == "in" else "out_col"] = at
            col += width + 1
        assert col + shift < ld - col - shift
        if side == "in":
            self.ld_in = ld
        else:
            self.ld_out = ld
        self.wl, self.wu, self.wc, self.n_win, self.stat_col, self.sd_total = d.wl, d.wu, d.wc, d.n_win, d.stat_col, d.sd_total

    def predict(self, algo, mode, dt, B, has_lengths):
        return SP.predict(self.streams, self.wl, self.wu, self.wc, algo, mode, SP.F32 if dt == F32 else SP.F64, B, T, self.ld_in,
                          self.ld_out, has_lengths)


def call_forward_streams(lay, dt, algo, mode, mean_ptr, var_ptr, lengths, B, out_ptr, status):
    from nnmnkwii_amd import _hip
    table = (_hip.StreamDesc * len(lay.streams))()
    for k, s in enumerate(lay.streams):
        table[k] = _hip.StreamDesc(s["in_col"], s["out_col"], s["static_dim"], s["num_windows"], s["win_first"])
    d = torch.device("cuda", torch.cuda.current_device())
    c0 = _counts(16)
    rc = _hip.lib().mlpg_hip_forward_streams(d.index, _hip._stream(d), int(dt == F64), algo, mean_ptr, var_ptr, mode, lay.ld_in,
                                             _hip._p(lengths), B, T, len(lay.streams), ctypes.addressof(table), lay.n_win,
                                             _hip._np(lay.wl), _hip._np(lay.wu), _hip._np(lay.wc), out_ptr, lay.ld_out,
                                             _hip._p(status))
    err = _hip.lib().mlpg_hip_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    moved = {k: n - c0[k] for k, n in enumerate(_counts(16)) if n != c0[k]}
    return rc, moved, err


def run_forward_streams(name, dt, with_lengths, side, ld=LD, B=None, spec=None, algo=None, mode=None):
    """One call with the means (and per-frame variances) or the output in a wide parent.  Returns (launch counter deltas, plan)
    after every check of the values, the status, the padding and the bytes around."""
    from oracle import mlpg as O
    if spec is None:
        spec, algo, mode = FAMILIES[name]
    B = BATCH[dt] if B is None else B
    lens = lengths_of(B, with_lengths) if B in LENS else np.array(([T, 67, 1, 0, 129] * B)[:B], dtype=np.int32)
    if not with_lengths:
        lens[:] = T
    shift = SHIFT if (side == "in" and mode == F) else 0
    lay = WideLayout(spec, side, ld, shift)
    dense = lay.dense
    M, V, _ = R.make_inputs(dense, dt, mode, B, T, False, zlib.crc32(repr((name, dt.__name__, with_lengths, side)).encode()) & 0xFFFF)
    if dt == F32 and mode == U and not with_lengths:
        R._warm_fir(dense)
    Ld = dev(lens) if with_lengths else None
    status = torch.full((B, lay.sd_total), R.STATUS_SENT, dtype=torch.int32, device="cuda")
    wide = wide_parent(dt, ld, B)
    if side == "in":
        for sw, sd_ in zip(lay.streams, dense.streams):
            cols = dense.in_cols(sd_)
            if len(cols):
                put(wide, M[:, :, cols], lens, sw["in_col"])
                if mode == F:
                    put(wide, V[:, :, cols], lens, sw["in_col"] + shift)
        mean_ptr, var_ptr = wide.ptr(), None
        if mode == F:
            var_ptr = wide.ptr(shift)
        elif mode == G:
            Vw = np.full(ld, np.nan, dtype=dt)
            for sw, sd_ in zip(lay.streams, dense.streams):
                Vw[sw["in_col"]:sw["in_col"] + len(dense.in_cols(sd_))] = V[dense.in_cols(sd_)]
            Vd = dev(Vw)
            var_ptr = Vd.data_ptr()
        it = torch.int64 if dt == F64 else torch.int32
        out = torch.full((B, T, lay.ld_out), R.SENT[dt], dtype=it, device="cuda")
        out_ptr = out.data_ptr()
        note("forward_streams", "mean", wide, dt)
        if mode == F:
            note("forward_streams", "var", wide, dt, shift)
    else:
        Md, Vd = dev(M), dev(V)
        mean_ptr, var_ptr = Md.data_ptr(), None if Vd is None else Vd.data_ptr()
        for s in lay.streams:
            if s["static_dim"]:
                expect(wide, s["out_col"], s["static_dim"])
        out_ptr = wide.ptr()
        note("forward_streams", "out", wide, dt)
    assert set(BYTES) <= wide.crossed(), wide.crossed()
    rc, moved, err = call_forward_streams(lay, dt, algo, mode, mean_ptr, var_ptr, Ld, B, out_ptr, status)
    assert rc == 0, err
    plan, kinds, n = lay.predict(algo, mode, dt, B, with_lengths)
    assert set(moved) <= set(SP.FORWARD_KINDS) and sum(moved.values()) == n, (moved, n, plan)
    if kinds is not None:
        assert moved == dict(kinds), (moved, dict(kinds), plan)
    # values, per stream, against the oracle on the compact slice
    st = status.cpu().numpy()
    assert not (st == R.STATUS_SENT).any()
    live = np.arange(T)[None, :] < lens[:, None]
    owned = np.zeros(lay.ld_out, dtype=bool) if side == "in" else None
    outh = out.view(torch.float64 if dt == F64 else torch.float32).cpu().numpy() if side == "in" else None
    for k, (sw, sd_) in enumerate(zip(lay.streams, dense.streams)):
        sd, oc = sw["static_dim"], sw["out_col"]
        if sd == 0:
            continue
        if side == "in":
            owned[oc:oc + sd] = True
            got = outh[:, :, oc:oc + sd]
        else:
            got = get(wide, oc, sd)
        assert not got[~live].any(), ("padding not zero", k)
        cols = dense.in_cols(sd_)
        if sd_["num_windows"] == 0:
            assert bits(got[live]) == bits(M[:, :, cols][live]), ("pass-through not a bit copy", k)
            assert not st[:, lay.stat_col[k]:lay.stat_col[k] + sd].any()
            continue
        w = dense.windows_of(sd_)
        vs = {F: lambda: np.ascontiguousarray(V[:, :, cols]), G: lambda: V[cols], U: lambda: np.ones(len(cols), dtype=dt)}[mode]()
        ref, rst, orc = O.mlpg_batch(np.ascontiguousarray(M[:, :, cols]), vs, w, lens if with_lengths else None)
        assert orc == 0 and np.array_equal(st[:, lay.stat_col[k]:lay.stat_col[k] + sd], rst), ("status", k)
        e = np.abs(got.astype(np.float64) - ref).max(axis=(1, 2))
        scale = np.abs(ref).max(axis=(1, 2))
        assert (e <= R.TOL[dt] * scale).all(), ("trajectory", name, k, (e / np.where(scale > 0, scale, 1)).tolist())
    if side == "in":
        assert (R._int_view(outh[:, :, ~owned]) == R.SENT[dt]).all(), "a column outside the streams was written"
    fails = wide.untouched()
    assert fails == [], fails
    wide.free()
    return moved, plan


FS_CASES = [(name, dt, wl, side) for name in FAMILIES for dt in (F64, F32) for wl in (True, False) for side in ("in", "out")
            if name != "fir" or (dt == F32 and not wl)]


@pytest.mark.parametrize("name,dt,with_lengths,side", FS_CASES,
                         ids=["%s-%s-%s-wide_%s" % (n, d.__name__, "lengths" if w else "full", s) for n, d, w, s in FS_CASES])
@far_test
def test_forward_streams_each_family_on_far_rows(name, dt, with_lengths, side):
    moved, plan = run_forward_streams(name, dt, with_lengths, side)
    if name in EXPECTED_KINDS:
        assert moved == EXPECTED_KINDS[name], (moved, plan)          # the family the case is named for, not only the model's word
    else:
        assert plan.attempted and not plan.merged                    # AUTO: 3 x 3 strips and 3 utterances merit no merged launch


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("side", ["in", "out"])
@far_test
def test_beyond_the_window_auto_takes_the_wave_or_natural_order_kernel(side, dt):
    """One element more per row: 130 * 2064889 * 8 >= 2^31 - 1.  AUTO still gives the right trajectory and moves none of the
    counters of the kernels that address an utterance through a buffer descriptor (kinds 2 - 9)."""
    assert not SP.rows_fit_buffer(T, LD_OVER) and SP.rows_fit_buffer(T, LD)
    for name in ("auto", "strip_merged"):
        spec, _, mode = FAMILIES[name]
        moved, plan = run_forward_streams(name, dt, True, side, ld=LD_OVER, spec=spec, algo=SP.AUTO, mode=mode)
        assert set(moved) <= {SP.K_GENERIC, SP.K_WAVE} and not plan.merged, (moved, plan)


TR_SPEC = [(5, "std3")]                             # u = 64 // 5 = 12 utterances share a group of the transposed strip form
TR_LD_IN, TR_LD_OVER = 172074, 172075               # 12 * 130 * 172074 * 8 < 2^31 - 1 <= 12 * 130 * 172075 * 8
TR_B = 25                                           # 25 * 130 * 172074 * 8 = 4.47e9 bytes: past 2^32


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("with_lengths", [True, False])
@pytest.mark.parametrize("side", ["in", "out"])
@pytest.mark.parametrize("ld", [TR_LD_IN, TR_LD_OVER])
@far_test
def test_transposed_strip_form_on_both_sides_of_its_rule(ld, side, with_lengths, dt):
    """The transposed form addresses the u utterances of a group from the first one's base: u * Tmax * ld * 8 < 2^31 - 1
    (strip_tr_supported).  Just inside, a forced STRIP moves counter 9; just outside it moves counter 2 and not 9; the values
    are right on both sides."""
    assert 12 * T * TR_LD_IN * 8 < 2 ** 31 - 1 <= 12 * T * TR_LD_OVER * 8
    B = TR_B * (2 if dt == F32 else 1)
    for mode in (F, G):
        moved, plan = run_forward_streams("tr", dt, with_lengths, side, ld=ld, B=B, spec=TR_SPEC, algo=SP.STRIP, mode=mode)
        assert moved == ({SP.K_STRIP_TR: 1} if ld == TR_LD_IN else {SP.K_STRIP: 1}), (mode, moved)


# ---------------------------------------------------------------------------------------------------- entries with one row stride per array

D_MAP = 40                                          # columns of the single-array entries: row 0 of utterance 2 straddles 2^32 bytes at column 32
COLS = (0, LD - D_MAP)


def run_map(entry, dt, variant, with_lengths, X, fn, check, args=("x", "out")):
    """An entry out = f(x) on (B, T, D) arrays with one row stride each.  variant: "wide_in" (x in the wide parent, out dense),
    "wide_out" (x dense, out in the wide parent) or "in_place" (both: the same columns of the wide parent).  fn(x, out, lengths)
    runs it on tensors (out None: a new dense one) and returns out.  check(got, lens) compares the (B, T, D) result with the
    entry's reference; the result on a compact copy of the rows must have the same bits."""
    B, _, D = X.shape
    lens = lengths_of(B, with_lengths)
    Ld = dev(lens) if with_lengths else None
    compact = fn(dev(X), None, Ld).cpu().numpy()
    check(compact, lens)
    wide = wide_parent(dt)
    for col in (0, LD - D):
        if variant != "wide_out":
            put(wide, X, lens, col)
        if variant != "wide_in":
            expect(wide, col, D)
        view = wide.cols(col, D)
        if variant == "wide_in":
            got = fn(view, None, Ld).cpu().numpy()
        else:
            r = fn(view if variant == "in_place" else dev(X), view, Ld)
            assert r.data_ptr() == view.data_ptr()
            torch.cuda.synchronize()
            got = get(wide, col, D)
        check(got, lens)
        assert bits(got) == bits(compact), (entry, variant, col, "differs from the call on a compact copy")
        fails = wide.untouched()
        assert fails == [], (entry, variant, col, fails)
    assert set(BYTES) <= wide.crossed()
    if variant != "wide_out":
        note(entry, args[0], wide, dt)
    if variant != "wide_in":
        note(entry, args[1], wide, dt)
    wide.free()


VARIANTS = ["wide_in", "wide_out", "in_place"]
MAP_CASES = [(dt, v, wl) for dt in (F64, F32) for v in VARIANTS for wl in (True, False)]
MAP_IDS = ["%s-%s-%s" % (d.__name__, v, "lengths" if w else "full") for d, v, w in MAP_CASES]


def _zero_pads(got, lens):
    for b, n in enumerate(lens):
        assert not got[b, n:].any(), ("padding", b)


@pytest.mark.parametrize("dt,variant,with_lengths", MAP_CASES, ids=MAP_IDS)
@far_test
def test_merlin_post_filter_on_far_rows(dt, variant, with_lengths):
    import postfilter_model as PM
    import test_postfilter_gpu as TP
    from nnmnkwii_amd import _hip
    d = torch.device("cuda", torch.cuda.current_device())
    B, alpha, order, fftlen = BATCH[dt], 0.42, 63, 128
    rng = np.random.RandomState(40)
    X = np.stack([TP.mgc_like(rng, T, D_MAP) for _ in range(B)]).astype(dt)
    w, G = dev(PM.default_weight(D_MAP)), _hip.postfilter_table(d, D_MAP, alpha, order, fftlen)

    def check(got, lens):
        ref = PM.post_filter_batch(X.astype(F64), alpha, order, fftlen, lengths=lens)
        assert TP._err(got, ref) <= TP.BOUND[dt], TP._err(got, ref)
        _zero_pads(got, lens)
    c0 = _counts()
    run_map("merlin_post_filter", dt, variant, with_lengths, X,
            lambda x, out, L: _hip.merlin_post_filter(x, alpha, w, G, fftlen, lengths=L, out=out), check, ("mgc", "out"))
    assert _moved(c0) == {29: 3}


@pytest.mark.parametrize("dt,variant,with_lengths", MAP_CASES, ids=MAP_IDS)
@far_test
def test_modspec_filter_on_far_rows(dt, variant, with_lengths):
    import modspec_batch64 as R64
    import msfilter_model as MM
    import test_msfilter_gpu as TM
    from nnmnkwii_amd import _hip
    B, n, limit_bin = BATCH[dt], 256, 40
    nb = n // 2 + 1
    rng = np.random.RandomState(41)
    A, C = TM._tables(rng, nb, D_MAP)
    At, Ct = dev(A), dev(C)
    X = R64.make_batch(rng, B, T, D_MAP, lengths_of(B, with_lengths)).astype(dt)        # NaN from each length on
    assert TM._phase_condition(X, MM.live_frames(lengths_of(B, with_lengths), B, T), n) >= 1e-6

    def check(got, lens):
        ref = MM.filter_batch(X, n, "ortho", lens, A, C, limit_bin, True)
        assert TM._err(got, ref) <= TM.BOUND[dt], TM._err(got, ref)
        TM._check_rows(got, lens)
    c0 = _counts()
    run_map("modspec_filter", dt, variant, with_lengths, X,
            lambda x, out, L: _hip.modspec_filter(x, n, At, Ct, limit_bin, True, True, lengths=L, out=out), check)
    assert _moved(c0) == {TM.KIND: 3}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt,variant,with_lengths", MAP_CASES, ids=MAP_IDS)
@far_test
def test_column_affine_on_far_rows(dt, variant, with_lengths, mode):
    import norm_cases as C
    import test_norm_gpu as TN
    from nnmnkwii_amd import _hip
    B = BATCH[dt]
    X, _ = C.padded(42 + mode, LENS[B] if with_lengths else [T] * B, D_MAP, dt, Tmax=T)
    rng = np.random.RandomState(42)
    a, c = rng.rand(D_MAP) + 0.5, rng.randn(D_MAP)
    at, ct = dev(a), dev(c)

    def check(got, lens):
        assert got.dtype == dt and TN.same_bits(got, C.NM.affine(X, a, c, mode, lens if with_lengths else None, dt))
        _zero_pads(got, lens)
    c0 = _counts()
    run_map("column_affine", dt, variant, with_lengths, X, lambda x, out, L: _hip.column_affine(x, at, ct, mode, L, out), check,
            ("x", "y"))
    assert _moved(c0) == {41: 3}


REDUCE_CASES = [(dt, wl) for dt in (F64, F32) for wl in (True, False)]
REDUCE_IDS = ["%s-%s" % (d.__name__, "lengths" if w else "full") for d, w in REDUCE_CASES]


def run_reduce(entry, dt, with_lengths, X, fn, check, arg="x"):
    """An entry that reads x (B, T, D) with a row stride and writes a small dense result: fn(x, lengths) -> tensor."""
    B, _, D = X.shape
    lens = lengths_of(B, with_lengths)
    Ld = dev(lens) if with_lengths else None
    compact = fn(dev(X), Ld).cpu().numpy()
    check(compact, lens)
    wide = wide_parent(dt)
    for col in (0, LD - D):
        put(wide, X, lens, col)
        got = fn(wide.cols(col, D), Ld).cpu().numpy()
        check(got, lens)
        assert bits(got) == bits(compact), (entry, col, "differs from the call on a compact copy")
        fails = wide.untouched()
        assert fails == [], (entry, col, fails)
    note(entry, arg, wide, dt)
    wide.free()


@pytest.mark.parametrize("dt,with_lengths", REDUCE_CASES, ids=REDUCE_IDS)
@far_test
def test_column_stats_on_far_rows(dt, with_lengths):
    import norm_cases as C
    import test_norm_gpu as TN
    from nnmnkwii_amd import _hip
    B = BATCH[dt]
    X, _ = C.padded(43, LENS[B] if with_lengths else [T] * B, D_MAP, dt, Tmax=T)
    model = C.NM.kernel_state(X, lengths_of(B, True) if with_lengths else None)
    truth = C.NM.exact(X, lengths_of(B, True) if with_lengths else None)

    def check(state, lens):
        assert TN.same_bits(state, model), np.abs(state - model).max()
        TN.check_stats(state, X, lens if with_lengths else None, truth)
    c0 = _counts()
    run_reduce("column_stats", dt, with_lengths, X, lambda x, L: _hip.column_stats(x, L), check)
    assert _moved(c0) == {39: 3}


@pytest.mark.parametrize("dt,with_lengths", REDUCE_CASES, ids=REDUCE_IDS)
@far_test
def test_gv_on_far_rows(dt, with_lengths):
    import gvmlpg_cases as GC
    from nnmnkwii_amd import _hip
    B = BATCH[dt]
    rng = np.random.RandomState(44)
    X = (rng.randn(B, T, D_MAP) * np.linspace(0.5, 4, D_MAP) + 2.0).astype(dt)

    def check(g, lens):
        ref = GC.GV.gv_padded(X, lens)
        assert g.dtype == np.float64 and (g[lens <= 1] == 0).all()
        assert np.abs(g - ref).max() <= 4 * T * GC.EPS * float(np.abs(X).max()) ** 2        # tests/test_gvmlpg_gpu.py
    c0 = _counts()
    run_reduce("gv", dt, with_lengths, X, lambda x, L: _hip.gv(x, L), check)
    assert _moved(c0) == {37: 3}


@pytest.mark.parametrize("dt,with_lengths", REDUCE_CASES, ids=REDUCE_IDS)
@pytest.mark.parametrize("which", ["x", "y"])
@far_test
def test_metrics_batch_on_far_rows(which, dt, with_lengths):
    """x wide and y dense, then y wide and x dense: eight terms inside 187 columns at the row's start and at its end; the totals
    and the per-utterance pairs against tools/metrics_model.py as tests/test_metrics_gpu.py has them, per_utt bit for bit
    against the call on compact copies."""
    import metrics_cases as MC
    from nnmnkwii_amd import _metrics_hip as M
    B, D = BATCH[dt], 187
    terms = MC.eight_terms()
    lens = lengths_of(B, with_lengths)
    X, Y, _ = MC.kernel_case(45, lens, T, D, dt, dt, terms)
    tt = [M.term(**{k: (None if k == "threshold" and v != v else v) for k, v in t.items()}) for t in terms]
    Ld = dev(lens) if with_lengths else None
    L_model = lens if with_lengths else None
    tot_c, per_c = M.metrics_batch(dev(X), dev(Y), tt, Ld, per_utt=True)
    model = MC.MM.kernel_order(X, Y, L_model, terms)
    wide = wide_parent(dt)
    c0 = M.lib().nnmk_metrics_launch_count()
    for col in (0, LD - D):
        put(wide, X if which == "x" else Y, lens, col)
        v = wide.cols(col, D)
        tot, per = M.metrics_batch(v if which == "x" else dev(X), v if which == "y" else dev(Y), tt, Ld, per_utt=True)
        tot, per = tot.cpu().numpy(), per.cpu().numpy()
        MC.check_against_model(tot, per, X, Y, L_model, terms, model)
        assert bits(per) == bits(per_c.cpu().numpy()) and bits(tot) == bits(tot_c.cpu().numpy())
        assert not per[lens == 0].any()
        fails = wide.untouched()
        assert fails == [], (which, col, fails)
    assert M.lib().nnmk_metrics_launch_count() - c0 == 2
    note("metrics_batch", which, wide, dt)
    wide.free()


@pytest.mark.parametrize("with_lengths", [True, False])
@pytest.mark.parametrize("which", ["x", "mean", "var"])
@far_test
def test_gmm_trajectory_stats_on_far_rows(which, with_lengths):
    """Each of the three arrays with a row stride in the wide parent in turn (float64 is the entry's only type)."""
    import gmmtraj_model as GM
    import test_gmmtraj_gpu as TG
    from nnmnkwii_amd import _hip
    B, D, M = BATCH[F64], D_MAP, 7
    lens = lengths_of(B, with_lengths)
    L_model = lens if with_lengths else None
    mu_x, mu_y, A, cvar = TG.tables(M, D, 46)
    tabs = [dev(a) for a in (mu_x, mu_y, A, cvar)]
    rng = np.random.RandomState(46)
    live = np.arange(T)[None] < lens[:, None]
    X = rng.randn(B, T, D) * 2.0
    X[~live] = np.nan                                                                     # a pad row's x is not read
    lab = ((np.arange(B * T) // 5) % M).astype(np.int32).reshape(B, T)
    lab[~live] = -7                                                                       # nor is its label
    Ld, labd = (dev(lens) if with_lengths else None), dev(lab)
    rm, rv = GM.stats_padded(X, L_model, lab.ravel(), mu_x, mu_y, A, cvar)
    S = GM.error_scale(X[live], lab[live], mu_x, mu_y, A)
    mc, vc = _hip.gmm_trajectory_stats(dev(X), Ld, labd, *tabs)
    mc, vc = mc.cpu().numpy(), vc.cpu().numpy()
    wide = wide_parent(F64)
    c0 = _counts()
    for col in (0, LD - D):
        view = wide.cols(col, D)
        if which == "x":
            put(wide, X, lens, col)
            gm, gv = _hip.gmm_trajectory_stats(view, Ld, labd, *tabs)
            gm, gv = gm.cpu().numpy(), gv.cpu().numpy()
        else:
            expect(wide, col, D)
            kw = {which: view}
            gm, gv = _hip.gmm_trajectory_stats(dev(X), Ld, labd, *tabs, **kw)
            torch.cuda.synchronize()
            gm, gv = (get(wide, col, D), gv.cpu().numpy()) if which == "mean" else (gm.cpu().numpy(), get(wide, col, D))
        assert (gm[~live] == 0).all() and (gv[~live] == 1).all()
        assert bits(gv[live]) == bits(cvar[lab[live]]) == bits(rv.reshape(B, T, D)[live])
        ratio = float((np.abs(gm[live] - rm.reshape(B, T, D)[live]) / (2 * (D + 4) * TG.EPS * S)).max())
        assert ratio <= 1.0, ratio                                                        # tests/test_gmmtraj_gpu.py
        assert bits(gm) == bits(mc) and bits(gv) == bits(vc), (which, col, "differs from the call on compact arrays")
        fails = wide.untouched()
        assert fails == [], (which, col, fails)
    assert _moved(c0) == {33: 2}
    note("gmm_trajectory_stats", which, wide, F64)
    wide.free()


# ---------------------------------------------------------------------------------------------------- mlpg_hip_backward_streams

BWD_CASES = [(dt, mode, algo, side, wl) for dt in (F64, F32) for mode, algo in ((F, SP.AUTO), (F, SP.STRIP), (U, SP.AUTO), (G, SP.CONST))
             for side in ("in", "out") for wl in (True, False)]


@pytest.mark.parametrize("dt,mode,algo,side,with_lengths", BWD_CASES,
                         ids=["%s-%s-%s-wide_%s-%s" % (d.__name__, R._MODE[m], R._ALGO[a], s, "lengths" if w else "full")
                              for d, m, a, s, w in BWD_CASES])
@far_test
def test_backward_streams_on_far_rows(dt, mode, algo, side, with_lengths):
    """With grad_var (per-frame and global variances) and without (unit variances).  side "in": mean, var, grad_mean and grad_var
    -- the four arrays of the input's layout -- share the wide parent, SHIFT columns apart; side "out": y and grad_out do.  The
    results are gathered back into the dense layout of tests/test_backward_streams_gpu.py and go through its checks against
    tests/streamgrad64.py unchanged."""
    import test_backward_streams_gpu as TB
    from nnmnkwii_amd import _hip
    spec = [(40, "std3"), (2, None), (24, "std3")]
    B = BATCH[dt]
    want_var = mode != U
    n_in = 4 if side == "in" else 2
    lay = WideLayout(spec, side, LD, (n_in - 1) * SHIFT)
    dense = lay.dense
    lens = lengths_of(B, with_lengths)
    seed = zlib.crc32(repr(("far bwd", dt.__name__, mode, algo, side, with_lengths)).encode()) & 0x7FFFFFFF
    M, V, Vp, _, Y, GO = TB.prepare(dense, dt, mode, B, T, False, seed)
    if with_lengths:                                  # (prepare's own ragged lengths are random: ours, and NaN behind them)
        pad = np.arange(T)[None, :] >= lens[:, None]
        M, Y, GO = M.copy(), Y.copy(), GO.copy()
        M[pad], Y[pad], GO[pad] = np.nan, np.nan, np.nan
        if mode == F:
            V = V.copy()
            V[pad] = np.nan
        rc, out, _, _, err = TB.drive_forward(dense, dev(np.nan_to_num(M)), dev(V if mode != F else np.nan_to_num(V, nan=1.0)), mode,
                                              dev(lens), SP.AUTO)
        assert rc == 0, err
        Y = out.cpu().numpy()
        Y[pad] = np.nan
    Ld = dev(lens) if with_lengths else None
    wide = wide_parent(dt)
    status = torch.full((B, lay.sd_total), R.STATUS_SENT, dtype=torch.int32, device="cuda")
    it = torch.int64 if dt == F64 else torch.int32
    pairs = list(zip(lay.streams, dense.streams))
    if side == "in":
        for sw, sd_ in pairs:
            cols = dense.in_cols(sd_)
            if not len(cols):
                continue
            put(wide, M[:, :, cols], lens, sw["in_col"])
            if mode == F:
                put(wide, V[:, :, cols], lens, sw["in_col"] + SHIFT)
            expect(wide, sw["in_col"] + 2 * SHIFT, len(cols))
            if want_var:
                expect(wide, sw["in_col"] + 3 * SHIFT, len(cols))
        var_ptr = wide.ptr(SHIFT) if mode == F else None
        if mode == G:
            Vw = np.full(LD, np.nan, dtype=dt)
            for sw, sd_ in pairs:
                Vw[sw["in_col"]:sw["in_col"] + len(dense.in_cols(sd_))] = V[dense.in_cols(sd_)]
            Vd = dev(Vw)
            var_ptr = Vd.data_ptr()
        Yd, GOd = dev(Y), dev(GO)
        ptrs = dict(mean=wide.ptr(), var=var_ptr, y=Yd.data_ptr(), grad_out=GOd.data_ptr(), grad_mean=wide.ptr(2 * SHIFT),
                    grad_var=wide.ptr(3 * SHIFT) if want_var else None)
        for k, arg in enumerate(("mean", "var", "grad_mean", "grad_var")):
            if (arg != "var" or mode == F) and (arg != "grad_var" or want_var):
                note("backward_streams", arg, wide, dt, k * SHIFT)
    else:
        for sw, sd_ in pairs:
            sd = sw["static_dim"]
            if sd:
                oc = sd_["out_col"]
                put(wide, Y[:, :, oc:oc + sd], lens, sw["out_col"])
                put(wide, GO[:, :, oc:oc + sd], lens, sw["out_col"] + SHIFT)
        Md, Vd = dev(M), dev(V)
        gmd = torch.full((B, T, dense.ld_in), R.SENT[dt], dtype=it, device="cuda")
        gvd = torch.full((B, T, dense.ld_in), R.SENT[dt], dtype=it, device="cuda")
        ptrs = dict(mean=Md.data_ptr(), var=None if Vd is None else Vd.data_ptr(), y=wide.ptr(), grad_out=wide.ptr(SHIFT),
                    grad_mean=gmd.data_ptr(), grad_var=gvd.data_ptr() if want_var else None)
        note("backward_streams", "y", wide, dt)
        note("backward_streams", "grad_out", wide, dt, SHIFT)
    assert set(BYTES) <= wide.crossed()
    table = (_hip.StreamDesc * len(lay.streams))()
    for k, s in enumerate(lay.streams):
        table[k] = _hip.StreamDesc(s["in_col"], s["out_col"], s["static_dim"], s["num_windows"], s["win_first"])
    d = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.synchronize()
    c0 = TB._counts()
    rc = _hip.lib().mlpg_hip_backward_streams(
        d.index, _hip._stream(d), int(dt == F64), algo, ptrs["mean"], ptrs["var"], mode, lay.ld_in, ptrs["y"], ptrs["grad_out"],
        lay.ld_out, _hip._p(Ld), B, T, len(lay.streams), ctypes.addressof(table), lay.n_win, _hip._np(lay.wl), _hip._np(lay.wu),
        _hip._np(lay.wc), ptrs["grad_mean"], ptrs["grad_var"], _hip._p(status))
    err = _hip.lib().mlpg_hip_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, err
    moved = {k: n - c0[k] for k, n in TB._counts().items() if n != c0[k]}
    TB.check_counters(dense, moved, algo, want_var)
    # the gradients back in the dense layout
    if side == "in":
        gm = np.frombuffer(np.full(B * T * dense.ld_in, R.SENT[dt], dtype=R._int_view(M).dtype).tobytes(), dtype=dt).reshape(M.shape).copy()
        gv = gm.copy()
        for sw, sd_ in pairs:
            cols = dense.in_cols(sd_)
            if len(cols):
                gm[:, :, cols] = get(wide, sw["in_col"] + 2 * SHIFT, len(cols))
                if want_var:
                    gv[:, :, cols] = get(wide, sw["in_col"] + 3 * SHIFT, len(cols))
    else:
        fl = torch.float64 if dt == F64 else torch.float32
        gm, gv = gmd.view(fl).cpu().numpy(), gvd.view(fl).cpu().numpy()
    TB.check_outputs(dense, M, V, V, mode, lens if with_lengths else None, Y, GO, gm, gv, status.cpu().numpy(), dt, want_var)
    fails = wide.untouched()
    assert fails == [], fails
    wide.free()


# ---------------------------------------------------------------------------------------------------- the Python surface

def _surface(fn):
    """fn() runs a public function on a column-slice view of the wide parent: the host-memory routes (kinds 10, 11) may not run
    and the peak of allocated device memory may grow by less than 64 MiB.  (Slices this small would pass both after a copy: that
    the slice itself reached the C entry is shown by the in-place forms, whose result comes back at the slice's pointer, and by
    the bits left in the parent.)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    c0 = _counts()
    res = fn()
    torch.cuda.synchronize()
    moved = _moved(c0)
    grown = torch.cuda.max_memory_allocated() - before
    assert grown < (64 << 20), "the call allocated %.1f MiB" % (grown / 2.0 ** 20)
    assert 10 not in moved and 11 not in moved, moved
    return res, moved


@far_test
def test_python_surface_on_column_slices_of_the_wide_parent():
    """paramgen.mlpg_batch, postfilters.merlin_post_filter_batch, preprocessing.scale and meanvar, metrics.batch_metrics on
    column-slice views of the wide float64 parent: the bits of the C entry on the same rows."""
    import metrics_cases as MC
    import norm_cases as C
    import postfilter_model as PM
    import test_postfilter_gpu as TP
    from cases import WINDOW_SETS
    from nnmnkwii_amd import _hip, _metrics_hip as M, metrics, paramgen, postfilters, preprocessing as P
    dt, B, D = F64, BATCH[F64], D_MAP
    lens = lengths_of(B, True)
    Ld = dev(lens)
    d = torch.device("cuda", torch.cuda.current_device())
    wide = wide_parent(dt)
    rng = np.random.RandomState(47)
    for col in (0, LD - 3 * D - SHIFT):
        # paramgen.mlpg_batch: means and per-frame variances, SHIFT columns apart, against mlpg_hip_forward_streams on the same rows
        lay = WideLayout([(D, "std3")], "in", LD, 0)
        lay.streams[0]["in_col"] = col
        Mx, Vx = rng.randn(B, T, 3 * D), rng.rand(B, T, 3 * D) + 0.1
        put(wide, Mx, lens, col)
        put(wide, Vx, lens, col + SHIFT)
        out = torch.zeros((B, T, lay.ld_out), dtype=torch.float64, device="cuda")
        status = torch.zeros((B, D), dtype=torch.int32, device="cuda")
        rc, moved_c, err = call_forward_streams(lay, dt, SP.AUTO, F, wide.ptr(), wide.ptr(SHIFT), Ld, B, out.data_ptr(), status)
        assert rc == 0, err
        oc = lay.streams[0]["out_col"]
        y, moved = _surface(lambda: paramgen.mlpg_batch(wide.cols(col, 3 * D), wide.cols(col + SHIFT, 3 * D), WINDOW_SETS["std3"], Ld))
        assert set(moved) == set(moved_c), (moved, moved_c)
        assert bits(y.cpu().numpy()) == bits(out[:, :, oc:oc + D].cpu().numpy())
        assert wide.untouched() == []
    for col in COLS:
        view = wide.cols(col, D)
        # postfilters.merlin_post_filter_batch
        X = np.stack([TP.mgc_like(rng, T, D) for _ in range(B)])
        put(wide, X, lens, col)
        assert bits(postfilters._weight(D, 1.4, None)) == bits(PM.default_weight(D))
        ref = _hip.merlin_post_filter(view, 0.42, dev(PM.default_weight(D)), _hip.postfilter_table(d, D, 0.42, 63, 128), 128, lengths=Ld)
        y, moved = _surface(lambda: postfilters.merlin_post_filter_batch(view, 0.42, 63, 128, lengths=Ld))
        assert moved == {29: 1} and torch.equal(y, ref)
        # in place: the tensor that comes back is the slice itself -- the pointer the C entry was given -- and holds those bits
        expect(wide, col, D)
        z, moved = _surface(lambda: postfilters.merlin_post_filter_batch(view, 0.42, 63, 128, lengths=Ld, out=view))
        assert moved == {29: 1} and z.data_ptr() == view.data_ptr() == wide.ptr(col) and bits(get(wide, col, D)) == bits(ref.cpu().numpy())
        assert wide.untouched() == []
        wide.forget()
        # preprocessing.meanvar and scale
        X, _ = C.padded(48, LENS[B], D, dt, Tmax=T)
        put(wide, X, lens, col)
        state = _hip.column_stats(view, Ld)
        (mean, var), moved = _surface(lambda: P.meanvar(view, Ld))
        assert moved == {39: 1}
        _, m_ref, v_ref, _, _ = C.NM.stats_of(state.cpu().numpy())
        assert bits(mean.cpu().numpy()) == bits(m_ref) and bits(var.cpu().numpy()) == bits(v_ref)
        std = var.sqrt()
        one = torch.where(std == 0, torch.ones_like(std), std)       # the reference's rule for a constant column's scale
        ref = _hip.column_affine(view, one, mean, 0, Ld)
        y, moved = _surface(lambda: P.scale(view, mean, std, lengths=Ld))
        assert moved == {41: 1} and bits(y.cpu().numpy()) == bits(ref.cpu().numpy())
        expect(wide, col, D)
        z, moved = _surface(lambda: P.scale(view, mean, std, lengths=Ld, out=view))
        assert moved == {41: 1} and z.data_ptr() == view.data_ptr() == wide.ptr(col) and bits(get(wide, col, D)) == bits(ref.cpu().numpy())
        assert wide.untouched() == []
        wide.forget()
    # metrics.batch_metrics: x a slice of the wide parent, y dense
    Dm = MC.G_D
    X, Y = MC.pair(49, B, T, Dm, dt, lf0_cols=(MC.G_LF0,), vuv_cols=(MC.G_VUV,))
    terms = {"mcd": ("melcd", MC.G_MGC), "bap": ("mse", MC.G_BAP), "lf0": ("lf0_mse", MC.G_LF0, MC.G_VUV), "vuv": ("vuv_error", MC.G_VUV)}
    gt = MC.golden_terms()
    tt = [M.term(**{k: (None if k == "threshold" and v != v else v) for k, v in gt[name].items()})
          for name in ("melcd/lengths", "mse/lengths", "lf0/lengths", "vuv/lengths")]
    for col in (0, LD - Dm):
        put(wide, X, lens, col)
        view, Yd = wide.cols(col, Dm), dev(Y)
        tot, _ = M.metrics_batch(view, Yd, tt, Ld)
        n0 = M.lib().nnmk_metrics_launch_count()
        got, moved = _surface(lambda: metrics.batch_metrics(view, Yd, Ld, terms))
        assert moved == {} and M.lib().nnmk_metrics_launch_count() - n0 == 1
        pairs = tot.cpu().numpy()
        # the same pairs (sum, count) as the C entry's: the root-mean figures and the ratio are then the model's bits
        want = {k: MC.figure(n, pairs[i]) for i, (k, n) in enumerate((("mcd", "melcd"), ("bap", "mse"), ("lf0", "lf0"), ("vuv", "vuv")))}
        assert all(got[k] == float(want[k]) for k in ("bap", "lf0", "vuv")), (got, want)
        # and every figure, the cepstral distortion included, is the one the same call gives on a dense copy of the slice
        dense = metrics.batch_metrics(dev(X), Yd, Ld, terms)
        assert got == dense, (got, dense)
        assert wide.untouched() == []
    assert set(BYTES) <= wide.crossed()
    wide.free()


# ---------------------------------------------------------------------------------------------------- coverage

def test_every_array_argument_crossed_every_boundary():
    """The table (entry, array argument, dtype) -> boundaries crossed, built from FarParent.crossed() as the tests above ran."""
    want = {}
    args = {"forward_streams": ("mean", "var", "out"), "backward_streams": ("mean", "var", "y", "grad_out", "grad_mean", "grad_var"),
            "merlin_post_filter": ("mgc", "out"), "modspec_filter": ("x", "out"), "column_affine": ("x", "y"), "column_stats": ("x",),
            "gv": ("x",), "metrics_batch": ("x", "y")}
    for entry, names in args.items():
        for arg in names:
            want[(entry, arg, "float64")] = set(BYTES)
            want[(entry, arg, "float32")] = set(BYTES) | {"2^31 elements"}
    for arg in ("x", "mean", "var"):
        want[("gmm_trajectory_stats", arg, "float64")] = set(BYTES)
    print()
    for key in sorted(set(want) | set(COVER)):
        print("%-24s %-10s %-8s %s" % (key + (", ".join(sorted(COVER.get(key, ()))) or "-",)))
    missing = {k: sorted(v - COVER.get(k, set())) for k, v in want.items() if v - COVER.get(k, set())}
    assert not missing, missing
