"""The launch contract of the device entry points (-m gpu): "enqueued on the current stream", "no synchronisation", "allocates
nothing".  One cell per entry (tests/stream_contract.py: make, load, call, verdict), each at the smallest shape at which the entry's
tiling still has more than one tile and a ragged tail, run through three checks:

``replayed_on_new_data``     the call captured into a graph on a side stream, replayed on other values and other lengths;
``two_streams_interleaved``  two cases on two streams, eight rounds, against the default stream's bytes;
``behind_a_late_producer``   the call behind a sleep and the copies that bring its inputs in.

Every verdict is the family's own (bits of its model, or its recorded bound); a run against another run is compared by bytes.
An entry whose header documents a synchronisation is kept out of the capture check, with the sentence quoted in its cell."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import stream_contract as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int16): torch.int16,
            np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}
CELLS = []


def cell(name, entries, **kw):
    """Decorator-free registration: ``cell(name, entries, make=..., load=..., call=..., verdict=..., expected=...)``; make is
    remembered per seed (a case is built once and left unchanged)."""
    kw["make"] = functools.lru_cache(maxsize=None)(kw["make"])
    c = SC.Cell(name, entries, **kw)
    CELLS.append(c)
    return c


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bit_fails(*pairs):
    """The names of the (name, device tensor, model array) triples whose bytes differ."""
    return [name for name, got, want in pairs if not same_bits(host(got), want)]


def want(case, compute):
    """The model's answer for a case, computed once."""
    if "_want" not in case:
        case["_want"] = compute(case)
    return case["_want"]


# ---- frame expansion (csrc/frame_expand.hip) ---------------------------------------------------------------------------------------

def _frontend():
    import frontend_model as FM
    import test_frontend_host_cpu as FHC
    BLOCK = FM.BLOCK_ROWS
    B, Nmax, S, Dl, kind = 4, 12, 5, 56, FM.FULL             # Dl + F = 65: a second pass over the columns
    W, Tmax = Dl + FM.SIZES[kind], 2 * BLOCK + 3
    # frames per utterance and phones per utterance: A and B differ in both; B holds an empty utterance (no phones) and a full one;
    # one utterance of each asks for more frames than Tmax (its length is capped, its count is not)
    PLAN = {1: ([Tmax, 0, BLOCK, Tmax + 9], [12, 0, 7, 12]), 2: ([5, Tmax, 0, Tmax + 20], [3, 12, 0, 11])}

    def make(seed):
        targets, n = PLAN[seed]
        P, d, n = FHC.make_case(seed, Nmax, S, Dl, targets, np.float32, n)
        rng = np.random.RandomState(seed + 7)
        return dict(P=P.astype(F32), d=d, n=n, scale=rng.rand(W) + 0.5, min=np.round(rng.randn(W) * 8) / 8)

    def model(c):
        return FM.frame_features_batch(c["P"], c["d"], c["n"], FM.KINDS[kind], 0, c["scale"], c["min"], Tmax, F32)

    def load(b, c):
        SC.put(b, "in_phone", c["P"])
        SC.put(b, "in_dur", c["d"])
        SC.put(b, "in_n", c["n"])
        SC.put(b, "in_scale", c["scale"])
        SC.put(b, "in_min", c["min"])

    def load_expand(b, c):
        load(b, c)
        SC.out(b, "out_rows", (B, Tmax, W), torch.float32)
        SC.out(b, "out_len", (B,), torch.int32)

    def call_counts(b):
        from nnmnkwii_amd import _frontend_hip as FH
        b["out_counts"] = FH.frame_counts(b["in_dur"], b["in_n"], 0)

    def call_expand(b):
        from nnmnkwii_amd import _frontend_hip as FH
        FH.expand(b["in_phone"], b["in_dur"], b["in_n"], kind, 0, None, b["in_scale"], b["in_min"], b["out_rows"], b["out_len"])

    cell("frontend.frame_counts", ["_frontend_hip.frame_counts"], make=make, load=load, call=call_counts,
         verdict=lambda c, b: bit_fails(("counts", b["out_counts"], want(c, model)[2])), expected=lambda c: [want(c, model)[2]])
    cell("frontend.expand", ["_frontend_hip.expand"], make=make, load=load_expand, call=call_expand,
         verdict=lambda c, b: bit_fails(("rows", b["out_rows"], want(c, model)[0]), ("lengths", b["out_len"], want(c, model)[1])),
         expected=lambda c: list(want(c, model)[:2]))


# ---- silence removal (csrc/frame_keep.hip) -----------------------------------------------------------------------------------------

def _silence():
    import silence_cases as C
    FM, SM = C.FM, C.SM
    BLOCK = C.BLOCK
    PLANS = {1: C.PLANS_A, 2: C.PLANS_B}                     # K_b = 0, 1, 63, 64, 65, 131 against 0, 26, 5, 140, 20, 0
    B, Nmax, S, Dl, kind = 6, 13, 5, 56, FM.FULL
    W, Tcap = Dl + FM.SIZES[kind], 2 * BLOCK + 3                # 131: A's longest fits exactly, B's 140 kept frames are cut
    Tsrc, D = 280, 63
    assert all(len(p) == B and max(len(u) for u in p) <= Nmax for p in PLANS.values())

    def make(seed):
        P, d, sil, n, _ = C.make_batch(seed, PLANS[seed], S, Dl, np.float64, Nmax=Nmax)
        scale, mn = C.affine(seed, W)
        T = C.all_counts(PLANS[seed])
        lens = np.clip(T + np.array([0, -1, 70, 0, -3, 5]) * (1 if seed == 1 else -1), 0, Tsrc).astype(np.int32)
        return dict(P=P.astype(F32), d=d, sil=sil, n=n, scale=scale, min=mn, Y=C.source(seed, B, Tsrc, D, lens), lens=lens)

    def counts(c):
        return SM.frame_counts(c["d"], c["sil"], c["n"], 0)

    def rows(c):
        return SM.kept_frame_features_batch(c["P"], c["d"], c["sil"], c["n"], FM.KINDS[kind], 0, c["scale"], c["min"], Tcap, F32)

    def gathered(c):
        return SM.remove_silence_frames_batch(c["Y"], c["d"], c["sil"], c["lens"], c["n"], 0, Tcap, F32)

    def load(b, c):
        SC.put(b, "in_dur", c["d"])
        SC.put(b, "in_sil", c["sil"])
        SC.put(b, "in_n", c["n"])

    def load_expand(b, c):
        load(b, c)
        SC.put(b, "in_phone", c["P"])
        SC.put(b, "in_scale", c["scale"])
        SC.put(b, "in_min", c["min"])
        SC.out(b, "out_rows", (B, Tcap, W), torch.float32)
        SC.out(b, "out_len", (B,), torch.int32)

    def load_gather(b, c):
        load(b, c)
        SC.put(b, "in_src", c["Y"])
        SC.put(b, "in_lens", c["lens"])
        SC.out(b, "out_rows", (B, Tcap, D), torch.float32)
        SC.out(b, "out_len", (B,), torch.int32)

    def call_counts(b):
        from nnmnkwii_amd import _silence_hip as SH
        b["out_counts"] = SH.frame_counts(b["in_dur"], b["in_n"], b["in_sil"], 0)

    def call_expand(b):
        from nnmnkwii_amd import _silence_hip as SH
        SH.expand(b["in_phone"], b["in_dur"], b["in_n"], b["in_sil"], kind, 0, None, b["in_scale"], b["in_min"], b["out_rows"], b["out_len"])

    def call_gather(b):
        from nnmnkwii_amd import _silence_hip as SH
        SH.gather(b["in_src"], b["in_lens"], b["in_dur"], b["in_n"], b["in_sil"], 0, b["out_rows"], b["out_len"])

    # (one case dict serves three cells: each keeps its own answer)
    def own(model, key):
        def f(c):
            if key not in c:
                c[key] = model(c)
            return c[key]
        return f
    cnt, exp, gat = own(counts, "_counts"), own(rows, "_rows"), own(gathered, "_gathered")
    cell("silence.frame_counts", ["_silence_hip.frame_counts"], make=make, load=load, call=call_counts,
         verdict=lambda c, b: bit_fails(("counts", b["out_counts"], cnt(c))), expected=lambda c: [cnt(c)])
    cell("silence.expand", ["_silence_hip.expand"], make=make, load=load_expand, call=call_expand,
         verdict=lambda c, b: bit_fails(("rows", b["out_rows"], exp(c)[0]), ("lengths", b["out_len"], exp(c)[1])),
         expected=lambda c: list(exp(c)[:2]))
    cell("silence.gather", ["_silence_hip.gather"], make=make, load=load_gather, call=call_gather,
         verdict=lambda c, b: bit_fails(("rows", b["out_rows"], gat(c)[0]), ("lengths", b["out_len"], gat(c)[1])),
         expected=lambda c: list(gat(c)[:2]))


# ---- joint rows (csrc/joint_rows.hip): count then write in one capture, a fixed capacity ------------------------------------------------

JOINT_POISON = np.frombuffer(bytes([SC.POISON]) * 8, dtype=np.float64)[0]


def joint_case(seed, name="stream"):
    """A (3, 2 * TILE + 3) batch of 63 + 65 columns under two windows.  Seed 1 keeps fewer rows than the capacity, seed 2 more
    (an empty utterance and two full ones); seeds 3 and 4 are a larger and a smaller batch (tests/test_workspace_content_gpu.py)."""
    import joint_cases as JC
    T = JC.TILE
    Tmax = 2 * T + 3
    rng = np.random.RandomState(4000 + seed)
    if seed == 3:
        return JC.case("%s-%d" % (name, seed), rng, 5, 3 * T + 1, 63, 65, JC.W2, [3 * T + 1, 7, 0, 3 * T, T + 1], [3 * T + 1, 9, 0, 3 * T, T],
                       zeros=[(0, 0), (0, T), (3, 2 * T - 1), (4, 5)], dtypes=(F32, F64, F64), cap=JOINT_CAP)
    if seed == 4:
        return JC.case("%s-%d" % (name, seed), rng, 2, T + 6, 63, 65, JC.W2, [T + 6, 9], [T + 5, 9], zeros=[(0, 3), (1, 0)], dtypes=(F32, F64, F64),
                       cap=JOINT_CAP)
    lens = {1: ([T + 30, Tmax, 0], [T + 36, Tmax - 1, 0]), 2: ([Tmax, 0, Tmax], [Tmax, 0, Tmax])}[seed]
    zeros = {1: [(0, 0), (0, T - 1), (0, T), (1, 2 * T), (1, 2 * T + 2)], 2: [(0, 5), (2, T), (2, 2 * T - 1)]}[seed]
    return JC.case("%s-%d" % (name, seed), rng, 3, Tmax, 63, 65, JC.W2, lens[0], lens[1], zeros=zeros, dtypes=(F32, F64, F64), cap=JOINT_CAP)


JOINT_CAP = 240        # rows of the output: case 1 keeps 231 rows, case 2 keeps 262 (tests/test_stream_contract_cpu.py asserts both)


def joint_load(b, c):
    import joint_cases as JC
    from nnmnkwii_amd import _joint_hip as JH
    X, Y = JC.typed(c)
    SC.put(b, "in_x", X)
    SC.put(b, "in_y", Y)
    SC.put(b, "in_len_x", c["len_x"])
    SC.put(b, "in_len_y", c["len_y"])
    SC.out(b, "out_rows", (JOINT_CAP, JC.width(c)), TORCH_DT[np.dtype(c["dtypes"][2])])
    SC.out(b, "out_offsets", (X.shape[0] + 1,), torch.int64)
    if b.get("ws") is None:
        b["ws"] = JH.workspace(X.shape[0], X.shape[1], "cuda")


def joint_call(b):
    import joint_cases as JC
    from nnmnkwii_amd import _joint_hip as JH
    plan, _ = JH.count(b["in_x"], b["in_y"], b["in_len_x"], b["in_len_y"], JC.W2, JH.NONZERO, 1e-7, b["out_rows"].dtype, ws=b["ws"],
                       offsets=b["out_offsets"])
    JH.write(plan, b["out_rows"])


def joint_verdict(c, b):
    import joint_cases as JC
    return JC.verdict(c, host(b["out_rows"]), host(b["out_offsets"]), sentinel=JOINT_POISON)


def joint_expected(c):
    import joint_cases as JC
    rows, offs = JC.expected(c)
    shown = np.full((JOINT_CAP, JC.width(c)), 1.0, dtype=rows.dtype)        # (the rows the capacity lets through)
    shown[:min(len(rows), JOINT_CAP)] = rows[:JOINT_CAP]
    return [shown, offs]


def _joint():
    cell("joint.count+write", ["_joint_hip.Plan.count", "_joint_hip.Plan.write"], make=joint_case, load=joint_load, call=joint_call,
         verdict=joint_verdict, expected=joint_expected)


# ---- continuous F0 (csrc/f0_interp.hip): the five modes ----------------------------------------------------------------------------------

def _f0():
    import f0_cases as FC
    F0 = FC.F0
    T = FC.TILE
    Tmax, C = 2 * T + 5, 3
    LENS = {1: [Tmax, T + 1, 0, 2, T], 2: [T - 1, 0, Tmax, Tmax - 3, 1]}
    LAYOUT = ((C + 2, 1), (C + 3, 2), (C + 1, 0))              # (ld, first column) of x, y, vuv: tests/test_f0_gpu.py's

    def maker(mode, kind, dtypes):
        def make(seed):
            rng = np.random.RandomState(150 + seed)
            X, lengths = FC.pack([FC.runs(rng, n) for n in LENS[seed]] , C, rng)
            if X.shape[1] < Tmax:
                X = np.concatenate([X, np.full((X.shape[0], Tmax - X.shape[1], C), np.nan)], axis=1)
            return FC._case("stream-%s-%d" % (mode, seed), X, lengths, kind, dtypes, mode)
        return make

    def load(b, c):
        dx, dy, dv = (np.dtype(t) for t in c["dtypes"])
        B = c["X"].shape[0]
        (ld_x, off_x), (ld_y, off_y), (ld_v, off_v) = LAYOUT
        wide = np.full((B, Tmax, ld_x), np.nan, dtype=dx)
        wide[:, :, off_x:off_x + C] = c["X"].astype(dx)
        c["_wide"] = wide
        SC.put(b, "in_x", wide)
        SC.put(b, "in_lengths", c["lengths"])
        SC.out(b, "out_y", (B, Tmax, ld_y), TORCH_DT[dy])
        SC.out(b, "out_v", (B, Tmax, ld_v), TORCH_DT[dv])
        if c["mode"] in ("inplace", "inplace_y"):
            SC.out(b, "out_x", wide.shape, TORCH_DT[dx])       # the tensor written in place: the call restores it from in_x first

    def call(b, mode, kind):
        from nnmnkwii_amd import _f0_hip as FH
        (_, off_x), (_, off_y), (_, off_v) = LAYOUT
        inplace = mode in ("inplace", "inplace_y")
        if inplace:
            b["out_x"].copy_(b["in_x"])
        xs = (b["out_x"] if inplace else b["in_x"])[:, :, off_x:off_x + C]
        y = None if mode == "vuv" else (xs if inplace else b["out_y"][:, :, off_y:off_y + C])
        v = None if mode in ("y", "inplace_y") else b["out_v"][:, :, off_v:off_v + C]
        FH.interp(xs, b["in_lengths"], F0.kind_of(kind), y, v)

    def verdict(c, b):
        inplace = c["mode"] in ("inplace", "inplace_y")
        fails = [] if same_bits(host(b["in_x"]), c["_wide"]) else ["the source changed"]
        xa = host(b["out_x"]) if inplace else host(b["in_x"])
        return fails + FC.verdict(c, (xa, host(b["out_y"]), host(b["out_v"]), c["_wide"], tuple(o for _, o in LAYOUT)))

    def expected(c):
        y, v = want(c, FC.expected)
        return [a for a, skip in ((y, c["mode"] == "vuv"), (v, c["mode"] in ("y", "inplace_y"))) if not skip]

    settings = {"both": ("slinear", (F64, F64, F64)), "y": ("nearest", (F64, F64, F32)), "vuv": ("zero", (F64, F64, F32)),
                "inplace": ("linear", (F32, F32, F32)), "inplace_y": ("next", (F32, F32, F64))}
    assert tuple(settings) == FC.MODES
    for mode in FC.MODES:
        kind, dtypes = settings[mode]
        cell("f0.interp[%s]" % mode, ["_f0_hip.interp"], make=maker(mode, kind, dtypes), load=load,
             call=functools.partial(call, mode=mode, kind=kind), verdict=verdict, expected=expected, sentinel=FC.SENTINEL)


# ---- waveform codec (csrc/wave_codec.hip): one float stage and one class stage each way --------------------------------------------------

def _wave():
    import wave_cases as WC
    WM = WC.WM
    T = WC.TILE
    Lmax = 2 * T + 5
    LENS = {1: [Lmax, 0, T + 1, T], 2: [1, Lmax, 0, 2 * T + 1]}
    NONE = 1 << 40

    def maker(tag, op, coef, stage, mu, segment, dtypes):
        def make(seed):
            rng = np.random.RandomState(160 + seed)
            tracks = [WC.wave(rng, n) for n in LENS[seed]]
            if op == "decode" and stage == WM.QUANTIZE:
                tracks = [rng.randint(0, mu + 1, size=len(t)).astype(dtypes[0]) for t in tracks]
                X, lengths = WC.pack(tracks, 9999)
                X[3 - 2 * (seed - 1), 5:7] = (-3, mu + 7)     # classes outside [0, mu] in live places: clamped
            else:
                X, lengths = WC.pack(tracks, np.nan)
            assert X.shape == (4, Lmax)
            return WC._case("stream-%s-%d" % (tag, seed), op, X, lengths, coef, stage, mu, segment, dtypes, "wide")
        return make

    def load(b, c):
        x, y = WC.buffers(c)
        SC.put(b, "in_x", x)
        SC.put(b, "in_lengths", c["lengths"])
        SC.out(b, "out_y", y.shape, TORCH_DT[y.dtype])
        if c["op"] == "decode" and c["stage"] == WM.QUANTIZE:
            SC.put(b, "table", WM.inv_mulaw_table(c["mu"]))

    def call(b, c0):
        from nnmnkwii_amd import _wave_hip as WH
        ld_x, off_x, ld_y, off_y = WC.layout_of(c0)
        xs, ys = b["in_x"][:, off_x:off_x + Lmax], b["out_y"][:, off_y:off_y + Lmax]
        if c0["op"] == "encode":
            WH.encode(xs, b["in_lengths"], c0["coef"], c0["stage"], c0["mu"], ys)
        else:
            WH.decode(xs, b["in_lengths"], c0["stage"], c0["mu"], b.get("table"), c0["coef"], min(c0["segment"], NONE), ys)

    def verdict(c, b):
        return WC.verdict(c, (0, host(b["in_x"]), host(b["out_y"])))

    for tag, op, coef, stage, mu, segment, dtypes in (("encode-float", "encode", 0.97, WM.MULAW, 256, 0, (F32, F32)),
                                                      ("encode-class", "encode", 0.97, WM.QUANTIZE, 256, 0, (F64, np.int16)),
                                                      ("decode-float", "decode", 0.5, WM.PLAIN, 256, 1024, (F64, F64)),
                                                      ("decode-class", "decode", float(np.float32(0.97)), WM.QUANTIZE, 256, NONE, (np.int32, F32))):
        make = maker(tag, op, coef, stage, mu, segment, dtypes)
        cell("wave.%s" % tag, ["_wave_hip.%s" % op], make=make, load=load, call=functools.partial(call, c0=make(1)), verdict=verdict,
             expected=lambda c: [WC.expected(c)], sentinel=WC.SENTINEL)


# ---- objective metrics (csrc/frame_metrics.hip): a caller-owned workspace, per-utterance sums ---------------------------------------------

def metrics_case(seed):
    """(X, Y, lengths, terms) at (4, 2 * BLOCK + 3, 187) with the eight terms of tests/metrics_cases.py; seeds 3 and 4: a larger and a
    smaller batch."""
    import metrics_cases as C
    Tmax = 2 * C.BLOCK + 3
    lens = {1: [Tmax, C.BLOCK, 1, 130], 2: [0, Tmax, C.BLOCK + 1, 7], 3: [3 * C.BLOCK + 1, 5, 0, 3 * C.BLOCK, C.BLOCK, 77], 4: [100, 17]}[seed]
    terms = C.eight_terms()
    X, Y, L = C.kernel_case(900 + seed, lens, max(lens), 187, F32, F64, terms)
    return dict(X=X, Y=Y, L=L, terms=terms)


def metrics_model(c):
    import metrics_cases as C
    return C.MM.kernel_order(c["X"], c["Y"], c["L"], c["terms"])


def metrics_load(b, c):
    from nnmnkwii_amd import _metrics_hip as M
    SC.put(b, "in_x", c["X"])
    SC.put(b, "in_y", c["Y"])
    SC.put(b, "in_lengths", c["L"])
    if b.get("ws") is None:
        B, Tmax = c["X"].shape[:2]
        b["ws"] = torch.empty(M.metrics_workspace(B, Tmax, len(c["terms"])), dtype=torch.uint8, device="cuda")
    if "terms" not in b:
        b["terms"] = [M.term(**{k: (None if k == "threshold" and v != v else v) for k, v in t.items()}) for t in c["terms"]]


def metrics_call(b):
    from nnmnkwii_amd import _metrics_hip as M
    b["out_totals"], b["out_per"] = M.metrics_batch(b["in_x"], b["in_y"], b["terms"], b["in_lengths"], per_utt=True, workspace=b["ws"])


def metrics_verdict(c, b):
    import metrics_cases as C
    C.check_against_model(host(b["out_totals"]), host(b["out_per"]), c["X"], c["Y"], c["L"], c["terms"], want(c, metrics_model))
    return []


def _metrics():
    cell("metrics.metrics_batch", ["_metrics_hip.metrics_batch"], make=metrics_case, load=metrics_load, call=metrics_call,
         verdict=metrics_verdict, expected=lambda c: [want(c, metrics_model)[1], want(c, metrics_model)[0]])


# ---- the entries of _hip.py ----------------------------------------------------------------------------------------------------------

EPS = np.finfo(np.float64).eps


def dist(a, ref):
    """max |a - ref| as a share of max |ref| (tests/gmm_em64.py's)."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - ref)) / max(np.max(np.abs(ref)), np.finfo(np.float64).tiny))


def far_fails(*quads):
    """The texts of the (name, device tensor or array, reference, bound) whose distance from the reference exceeds the bound."""
    fails = []
    for name, got, ref, bound in quads:
        got = host(got) if torch.is_tensor(got) else np.asarray(got)
        if got.shape != np.shape(ref):
            fails.append("%s: shape %s, not %s" % (name, got.shape, np.shape(ref)))
        elif not np.isfinite(got).all():
            fails.append("%s: not finite" % name)
        elif dist(got, ref) > bound:
            fails.append("%s: %.3g above the bound %.3g" % (name, dist(got, ref), bound))
    return fails


def padded_rows_fail(name, got, live, value=0.0):
    """Rows at or past each length must hold `value` exactly (and no negative zero)."""
    got = host(got) if torch.is_tensor(got) else got
    bad = [b for b in range(len(live)) if (got[b, live[b]:] != value).any() or np.signbit(got[b, live[b]:]).any()]
    return ["%s: pad rows of utterances %s" % (name, bad)] if bad else []


def _postfilter():
    import postfilter_model as PM
    TILE = 64                                               # MLPG_HIP_POSTFILTER_FRAME_TILE (asserted in load)
    B, D, alpha, order, fftlen = 3, 25, 0.42, 31, 64
    Tmax = 2 * TILE + 3
    LENS = {1: [Tmax, 11, TILE + 6], 2: [0, Tmax, TILE + 1]}

    def make(seed):
        rng = np.random.RandomState(170 + seed)
        clean = rng.randn(B, Tmax, D) / (1.0 + np.arange(D))
        clean[:, :, 0] += rng.uniform(-8.0, 2.0, (B, Tmax))
        lens = np.array(LENS[seed], dtype=np.int32)
        x = clean.copy()
        for b in range(B):
            x[b, lens[b]:] = np.nan
        return dict(x=x, lens=lens, ref=PM.post_filter_batch(clean, alpha, order, fftlen, lengths=lens))

    def load(b, c):
        from nnmnkwii_amd import _hip
        assert _hip.POSTFILTER_FRAME_TILE == TILE
        SC.put(b, "in_x", c["x"])
        SC.put(b, "in_lengths", c["lens"])
        SC.put(b, "in_weight", PM.default_weight(D))
        SC.out(b, "out_y", (B, Tmax, D), torch.float64)

    def call(b):
        from nnmnkwii_amd import _hip
        G = _hip.postfilter_table(b["in_x"].device, D, alpha, order, fftlen)       # built and uploaded on the first sight of its key
        _hip.merlin_post_filter(b["in_x"], alpha, b["in_weight"], G, fftlen, lengths=b["in_lengths"], out=b["out_y"])

    cell("merlin_post_filter", ["_hip.merlin_post_filter"], make=make, load=load, call=call,
         verdict=lambda c, b: far_fails(("y", b["out_y"], c["ref"], 1e-11)) + padded_rows_fail("y", b["out_y"], c["lens"]),
         expected=lambda c: [c["ref"]])


def _msfilter():
    import modspec_batch64 as R
    import msfilter_model as MM
    n, B, D = 64, 4, 5
    nb, Tmax = n // 2 + 1, n - 3
    limit_bin = nb - 1
    LENS = {1: [Tmax, n // 2 + 1, 0, (3 * n) // 4], 2: [0, Tmax, 40, 7]}
    trng = np.random.RandomState(171)
    A, C = trng.uniform(0.43, 2.7, (nb, D)), trng.uniform(-2 * np.log(16.0), 2 * np.log(16.0), (nb, D))

    def make(seed):
        rng = np.random.RandomState(172 + seed)
        x = R.make_batch(rng, B, Tmax, D, LENS[seed])
        live = MM.live_frames(LENS[seed], B, Tmax)
        for b in range(B):                                   # the condition tests/test_msfilter_gpu.py asserts on its inputs
            if live[b]:
                mag = np.abs(np.fft.rfft(x[b, :live[b]], n=n, axis=0))
                assert (mag.min(axis=0) / mag.max(axis=0)).min() >= 1e-6
        return dict(x=x, lens=np.array(LENS[seed], dtype=np.int32), live=live,
                    ref=MM.filter_batch(x, n, None, LENS[seed], A, C, limit_bin, True))

    def load(b, c):
        from nnmnkwii_amd import _hip
        assert _hip.modspec_filter_form(n) == 1
        SC.put(b, "in_x", c["x"])
        SC.put(b, "in_lengths", c["lens"])
        SC.put(b, "in_A", A)
        SC.put(b, "in_C", C)
        SC.out(b, "out_y", (B, Tmax, D), torch.float64)

    def call(b):
        from nnmnkwii_amd import _hip
        _hip.modspec_filter(b["in_x"], n, b["in_A"], b["in_C"], limit_bin, True, False, lengths=b["in_lengths"], out=b["out_y"])

    cell("modspec_filter", ["_hip.modspec_filter"], make=make, load=load, call=call,
         verdict=lambda c, b: far_fails(("y", b["out_y"], c["ref"], 1e-10)) + padded_rows_fail("y", b["out_y"], c["live"]),
         expected=lambda c: [c["ref"]])


def _gmmtraj():
    import gmmtraj_model as GM
    TILE = GM.ROW_TILE
    B, T, D, M = 3, (2 * TILE + 3 + 4) // 3, 17, 5           # 135 rows of the (B * Tmax) axis: two tiles and seven rows
    LENS = {1: [T, 0, 20], 2: [7, T, T - 1]}
    trng = np.random.RandomState(173)
    scales = trng.permutation(np.linspace(0.5, 3.0, D))
    mu_x, mu_y = trng.randn(M, D) * scales, trng.randn(M, D) * scales[::-1]
    A = np.ascontiguousarray(trng.randn(M, D, D) / np.sqrt(D) * scales[None, :, None] / scales[None, None, :])
    cvar = trng.rand(M, D) + 0.1

    def make(seed):
        rng = np.random.RandomState(174 + seed)
        lens = np.array(LENS[seed], dtype=np.int32)
        live = (np.arange(T)[None] < lens[:, None]).reshape(B * T)
        x = rng.randn(B * T, D) * 2.0
        lab = ((np.arange(B * T) + seed) % M).astype(np.int32)
        x[~live] = np.nan                                    # a pad row's x is not read, nor is its label
        lab[~live] = np.where(np.arange((~live).sum()) % 2 == 0, -7, M + 9)
        x = x.reshape(B, T, D)
        rm, rv = GM.stats_padded(x, LENS[seed], lab, mu_x, mu_y, A, cvar)
        return dict(x=x, lens=lens, lab=lab, live=live, rm=rm.reshape(B * T, D), rv=rv.reshape(B * T, D))

    def load(b, c):
        from nnmnkwii_amd import _hip
        assert _hip.GMM_TRAJ_ROW_TILE == TILE
        SC.put(b, "in_x", c["x"])
        SC.put(b, "in_lengths", c["lens"])
        SC.put(b, "in_idx_labels", c["lab"])
        for k, a in (("mu_x", mu_x), ("mu_y", mu_y), ("A", A), ("cvar", cvar)):
            SC.put(b, "in_" + k, a)
        SC.out(b, "out_mean", (B, T, D), torch.float64)
        SC.out(b, "out_var", (B, T, D), torch.float64)

    def call(b):
        from nnmnkwii_amd import _hip
        _hip.gmm_trajectory_stats(b["in_x"], b["in_lengths"], b["in_idx_labels"], b["in_mu_x"], b["in_mu_y"], b["in_A"], b["in_cvar"],
                                  mean=b["out_mean"], var=b["out_var"])

    def verdict(c, b):
        """tests/test_gmmtraj_gpu.py's: pad rows 0 and 1, variances the bits of cvar[label], means within 2 (D + 4) eps S."""
        gm, gv, ok = host(b["out_mean"]).reshape(B * T, D), host(b["out_var"]).reshape(B * T, D), c["live"]
        fails = []
        if not ((gm[~ok] == 0).all() and (gv[~ok] == 1).all()):
            fails.append("pad rows")
        if gv[ok].tobytes() != c["rv"][ok].tobytes():
            fails.append("variances")
        if not np.isfinite(gm[ok]).all():
            fails.append("means not finite")
        elif ok.any():
            S = GM.error_scale(c["x"].reshape(B * T, D)[ok], c["lab"][ok], mu_x, mu_y, A)
            ratio = float((np.abs(gm[ok] - c["rm"][ok]) / (2 * (D + 4) * EPS * S)).max())
            if ratio > 1.0:
                fails.append("means: %.3f of the bound" % ratio)
        return fails

    cell("gmm_trajectory_stats", ["_hip.gmm_trajectory_stats"], make=make, load=load, call=call, verdict=verdict,
         expected=lambda c: [c["rm"], c["rv"]])


def _gv():
    import gvmlpg_cases as C
    GV = C.GV
    B, Tmax, sd, n_iter = 4, 2 * GV.LANES + 3, 3, 5
    LENS = {1: [Tmax, 65, 1, 64], 2: [0, Tmax, 77, 2]}

    # ---- gv
    def make_gv(seed):
        rng = np.random.RandomState(175 + seed)
        x = rng.randn(B, Tmax, 5) * np.linspace(0.5, 4, 5) + 2.0
        lens = np.array(LENS[seed], dtype=np.int32)
        for b in range(B):
            x[b, lens[b]:] = np.nan
        return dict(x=x, lens=lens, ref=GV.gv_padded(np.nan_to_num(x), LENS[seed]), big=float(np.nanmax(np.abs(x))))

    def load_gv(b, c):
        SC.put(b, "in_x", c["x"])
        SC.put(b, "in_lengths", c["lens"])

    def call_gv(b):
        from nnmnkwii_amd import _hip
        b["out_gv"] = _hip.gv(b["in_x"], b["in_lengths"])

    def verdict_gv(c, b):
        g = host(b["out_gv"])
        fails = [] if np.isfinite(g).all() and np.abs(g - c["ref"]).max() <= 4 * Tmax * C.EPS * c["big"] ** 2 else ["gv"]
        return fails + ([] if (g[c["lens"] <= 1] == 0).all() else ["utterances of 0 or 1 frames"])

    cell("gv", ["_hip.gv"], make=make_gv, load=load_gv, call=call_gv, verdict=verdict_gv, expected=lambda c: [c["ref"]])

    # ---- gv_ascent, a few iterations, into a tensor of its own
    def make(seed):
        c = C.make_case(176 + seed, B, Tmax, sd, "std3", GV.VAR_FRAME, np.float64, LENS[seed])
        c["model"] = C.model(c, n_iter=n_iter)
        live = GV.live_frames(c["lengths"], B, Tmax)
        for k in ("mean", "var", "y_in"):                     # what lies past a length is never read
            c[k] = c[k].copy()
            for b in range(B):
                c[k][b, live[b]:] = np.nan
        return c

    def load(b, c):
        from nnmnkwii_amd import _hip
        SC.put(b, "in_mean", c["mean"])
        SC.put(b, "in_var", c["var"])
        SC.put(b, "in_y", c["y_in"])
        SC.put(b, "in_gv_mean", c["gv_mean"])
        SC.put(b, "in_gv_prec", c["gv_prec"])
        SC.put(b, "in_lengths", np.asarray(c["lengths"], dtype=np.int32))
        SC.out(b, "out_y", (B, Tmax, sd), torch.float64)
        b["windows"] = _hip.prepack_windows(c["windows"])

    def call(b):
        from nnmnkwii_amd import _hip
        _, b["out_report"], b["out_status"] = _hip.gv_ascent(b["in_mean"], b["in_var"], b["windows"], b["in_y"], b["in_gv_mean"], b["in_gv_prec"],
                                                             b["in_lengths"], n_iter=n_iter, out=b["out_y"])

    def verdict(c, b):
        """tests/test_gvmlpg_gpu.py's check_against_model."""
        y, rep, st = host(b["out_y"]), host(b["out_report"]), host(b["out_status"])
        y_m, rep_m, st_m = c["model"]
        live = GV.live_frames(c["lengths"], B, Tmax)
        pad = np.arange(Tmax)[None, :] >= live[:, None]
        fails = [] if (y[pad] == 0).all() else ["pad frames"]
        if not np.array_equal(st, st_m):
            fails.append("status")
        err = float(np.abs(y - y_m).max())
        if not err <= C.tolerance(y_m, np.float64):
            fails.append("y: %.3g above %.3g" % (err, C.tolerance(y_m, np.float64)))
        scale = np.abs(rep_m).max(axis=(0, 1)) + 1e-300
        if not (np.abs(rep - rep_m) <= 64 * C.BOUND_RATIO * C.EPS * scale).all():
            fails.append("report")
        if not ((rep[live == 0] == 0).all() and (st[live == 0] == 0).all()):
            fails.append("the empty utterance's report")
        return fails

    cell("gv_ascent", ["_hip.gv_ascent"], make=make, load=load, call=call, verdict=verdict,
         expected=lambda c: [c["model"][0], c["model"][1]])


def gmm_case(seed, N=131, F=17, K=3):
    """A random mixture with distinct column scales (tests/test_gmm_em_gpu.py's), N rows drawn from it and random responsibilities."""
    import gmm_em64 as R
    rng = np.random.RandomState(1000 * F + K + seed)
    scales = rng.permutation(np.linspace(0.5, 3.0, F))
    Am = rng.randn(K, F, F) / np.sqrt(F)
    cov = (Am @ Am.transpose(0, 2, 1) + 0.5 * np.eye(F)) * np.outer(scales, scales)
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    means = 2.0 * rng.randn(K, F) / np.sqrt(F) * scales
    weights = rng.dirichlet(np.full(K, 5.0))
    U, log_det = R.precisions(cov)
    lab = rng.randint(K, size=N)
    X = means[lab] + np.einsum("nfg,ng->nf", np.linalg.cholesky(cov)[lab], rng.randn(N, F))
    resp = rng.dirichlet(np.full(K, 0.7), size=N)
    return dict(X=X, weights=weights, means=means, cov=cov, U=U, log_det=log_det, cond=R.cond(cov), resp=resp,
                e=R.e_step(X, weights, means, U, log_det), m=R.m_step(X, resp, 1e-6))


def gmm_estep_load(b, c):
    from nnmnkwii_amd import _hip
    for k in ("X", "weights", "means", "U", "log_det"):
        SC.put(b, "in_" + k, c[k])
    if b.get("ws") is None:
        N, F = c["X"].shape
        b["ws"] = _hip.gmm_workspace("cuda", N, F, c["means"].shape[0])


def gmm_estep_call(b):
    from nnmnkwii_amd import _hip
    b["out_resp"], b["out_lpn"], b["out_labels"], b["out_mean"] = _hip.gmm_estep(
        b["in_X"], b["in_weights"], b["in_means"], b["in_U"], b["in_log_det"], want_resp=True, want_log_prob_norm=True, want_labels=True,
        want_mean=True, workspace=b["ws"])


def gmm_estep_verdict(c, b):
    resp_r, lpn_r, _, mean_r = c["e"]
    fails = far_fails(("resp", b["out_resp"], resp_r, 1e-10), ("log_prob_norm", b["out_lpn"], lpn_r, 1e-10), ("mean", b["out_mean"], mean_r, 1e-10))
    top = np.sort(resp_r, axis=1)[:, ::-1]
    clear = top[:, 0] - top[:, 1] > 1e-9
    if (~clear).mean() > 0.01 or not np.array_equal(host(b["out_labels"])[clear], resp_r.argmax(axis=1)[clear]):
        fails.append("labels")
    return fails


def gmm_mstep_load(b, c):
    from nnmnkwii_amd import _hip
    SC.put(b, "in_X", c["X"])
    SC.put(b, "in_resp", c["resp"])
    if b.get("ws") is None:
        N, F = c["X"].shape
        b["ws"] = _hip.gmm_workspace("cuda", N, F, c["resp"].shape[1])


def gmm_mstep_call(b):
    from nnmnkwii_amd import _hip
    b["out_weights"], b["out_means"], b["out_cov"] = _hip.gmm_mstep(b["in_X"], b["in_resp"], 1e-6, workspace=b["ws"])


def gmm_mstep_verdict(c, b):
    w_r, mu_r, cov_r = c["m"]
    fails = far_fails(("weights", b["out_weights"], w_r, 1e-10), ("means", b["out_means"], mu_r, 1e-10), ("covariances", b["out_cov"], cov_r, 1e-10))
    return fails + ([] if torch.equal(b["out_cov"], b["out_cov"].transpose(1, 2)) else ["covariances not symmetric"])


def _gmm():
    cell("gmm_estep", ["_hip.gmm_estep"], make=gmm_case, load=gmm_estep_load, call=gmm_estep_call, verdict=gmm_estep_verdict,
         expected=lambda c: [c["e"][0], c["e"][1], np.asarray(c["e"][3])])
    cell("gmm_mstep", ["_hip.gmm_mstep"], make=gmm_case, load=gmm_mstep_load, call=gmm_mstep_call, verdict=gmm_mstep_verdict,
         expected=lambda c: list(c["m"]))

    def call_prec(b):
        from nnmnkwii_amd import _hip
        b["out_U"], b["out_log_det"], b["out_status"] = _hip.gmm_precisions(b["in_cov"])

    def verdict_prec(c, b):
        fails = far_fails(("U", b["out_U"], c["U"], max(1e-10, 8 * EPS * c["cond"])), ("log_det", b["out_log_det"], c["log_det"], 1e-10))
        if b["out_status"].any().item():
            fails.append("status")
        return fails + ([] if torch.equal(b["out_U"], torch.triu(b["out_U"])) else ["U not upper triangular"])

    def load_prec(b, c):
        SC.put(b, "in_cov", c["cov"])

    cell("gmm_precisions", ["_hip.gmm_precisions"], make=gmm_case, load=load_prec, call=call_prec,
         verdict=verdict_prec, expected=lambda c: [c["U"], c["log_det"]])

    # ---- gmm_convert, the posterior form (tests/test_embed_entries_gpu.py's inputs and bound)
    N, D, Dy, M = 2 * 64 + 3, 3, 3, 4

    def make_conv(seed):
        rng = np.random.RandomState(177 + seed)
        x, mu_x, mu_y, A = rng.randn(N, D), rng.randn(M, D), rng.randn(M, Dy), rng.randn(M, Dy, D)
        post = rng.dirichlet(np.ones(M), size=N)
        per = mu_y[None] + np.einsum("myd,nmd->nmy", A, x[:, None, :] - mu_x[None])
        return dict(x=x, mu_x=mu_x, mu_y=mu_y, A=A, post=post, ref=np.einsum("nm,nmy->ny", post, per))

    def load_conv(b, c):
        for k in ("x", "post", "mu_x", "mu_y", "A"):
            SC.put(b, "in_" + k, c[k])

    def call_conv(b):
        from nnmnkwii_amd import _hip
        b["out_y"] = _hip.gmm_convert(b["in_x"], b["in_post"], None, b["in_mu_x"], b["in_mu_y"], b["in_A"])

    cell("gmm_convert", ["_hip.gmm_convert"], make=make_conv, load=load_conv, call=call_conv,
         verdict=lambda c, b: far_fails(("out", b["out_y"], c["ref"], 1e-10)), expected=lambda c: [c["ref"]])


def kmeans_case(seed, N=131, F=17, K=3, C=5):
    """tests/kmeans64.py's step_case with what both steps must give."""
    import kmeans64 as R
    c = R.step_case(N, F, K, C, 178 + seed)
    Xc = c["X"] - c["shift"]
    c["seed_ref"] = R.seed_step(Xc, c["cand"], c["closest"])
    c["lloyd_ref"] = R.step_expected(c)
    return c


def kmeans_load(b, c):
    from nnmnkwii_amd import _hip
    N, F = c["X"].shape
    SC.put(b, "in_X", c["X"])
    SC.put(b, "in_shift", c["shift"])
    SC.put(b, "in_idx_cand", c["cand"].astype(np.int32))
    SC.put(b, "in_closest", c["closest"])
    SC.put(b, "in_centers", c["centers"])
    SC.put(b, "in_prev", c["prev"])
    if b.get("ws") is None:
        b["ws"] = _hip.kmeans_workspace("cuda", N, F, c["centers"].shape[0])


def kmeans_seed_call(b):
    from nnmnkwii_amd import _hip
    b["out_d"], b["out_pots"] = _hip.kmeans_seed_step(b["in_X"], b["in_shift"], b["in_idx_cand"], b["in_closest"], workspace=b["ws"])


def kmeans_seed_verdict(c, b):
    return far_fails(("d", b["out_d"], c["seed_ref"][0], 1e-10), ("pots", b["out_pots"], c["seed_ref"][1], 1e-10))


def kmeans_lloyd_call(b):
    from nnmnkwii_amd import _hip
    (b["out_labels"], b["out_min_dist"], b["out_sums"], b["out_counts"], b["out_centers"], b["out_stats"]) = _hip.kmeans_lloyd_step(
        b["in_X"], b["in_shift"], b["in_centers"], b["in_prev"], want_min_dist=True, workspace=b["ws"])


def kmeans_lloyd_verdict(c, b):
    import kmeans64 as R
    from nnmnkwii_amd import _hip
    move, inertia, changed, empty = _hip.kmeans_stats(b["out_stats"])
    R.check_step(c, c["lloyd_ref"], dict(labels=host(b["out_labels"]), min_dist=host(b["out_min_dist"]), sums=host(b["out_sums"]),
                                         counts=host(b["out_counts"]), centers=host(b["out_centers"]), shift=move, inertia=inertia,
                                         changed=changed, empty=empty))
    return []


def _kmeans():
    cell("kmeans_seed_step", ["_hip.kmeans_seed_step"], make=kmeans_case, load=kmeans_load, call=kmeans_seed_call, verdict=kmeans_seed_verdict,
         expected=lambda c: list(c["seed_ref"]))
    cell("kmeans_lloyd_step", ["_hip.kmeans_lloyd_step"], make=kmeans_case, load=kmeans_load, call=kmeans_lloyd_call,
         verdict=kmeans_lloyd_verdict,
         expected=lambda c: [c["lloyd_ref"]["labels"].astype(np.int32), c["lloyd_ref"]["sums"], c["lloyd_ref"]["centers"]])


def _small_entries():
    import gvmlpg_cases
    windows = gvmlpg_cases.WINDOWS["std3"]
    B, T, D = 3, 2 * 64 + 3, 5
    LENS = {1: [T, 16, 0], 2: [0, T, 70]}

    # ---- delta_features
    def make_delta(seed):
        from oracle import mlpg as O
        rng = np.random.RandomState(179 + seed)
        x = rng.randn(B, T, D)
        ref = np.zeros((B, T, D * 3))
        for b, n in enumerate(LENS[seed]):
            if n:
                ref[b, :n] = O.delta_features(x[b, :n], windows)
            x[b, n:] = np.nan
        return dict(x=x, lens=np.array(LENS[seed], dtype=np.int32), ref=ref)

    def load_delta(b, c):
        SC.put(b, "in_x", c["x"])
        SC.put(b, "in_lengths", c["lens"])

    def call_delta(b):
        from nnmnkwii_amd import _hip
        b["out_y"] = _hip.delta_features(b["in_x"], windows, b["in_lengths"])

    def verdict_delta(c, b):
        got = host(b["out_y"])
        fails = padded_rows_fail("out", got, c["lens"])
        live = np.arange(T)[None, :] < c["lens"][:, None]
        if not np.allclose(got[live], c["ref"][live], rtol=1e-12, atol=1e-14):       # tests/test_embed_entries_gpu.py's float64 bound
            fails.append("out")
        return fails

    cell("delta_features", ["_hip.delta_features"], make=make_delta, load=load_delta, call=call_delta, verdict=verdict_delta,
         expected=lambda c: [c["ref"]])

    # ---- backward (the route AUTO picks): oracle/grad64.py with the bound and the padding rule of tests/test_backward_routes_gpu.py
    sd = 5

    def make_backward(seed):
        from oracle.grad64 import mlpg_grad64
        rng = np.random.RandomState(180 + seed)
        lens = np.array([T, 16, 0, 70] if seed == 1 else [0, T, 65, 1], dtype=np.int32)
        var, go = rng.rand(4, T, 3 * sd) + 0.1, rng.randn(4, T, sd)
        ref = mlpg_grad64(var, go, windows, lens)
        for b, n in enumerate(lens):
            var[b, n:] = np.nan
            go[b, n:] = np.nan
        return dict(var=var, go=go, lens=lens, ref=ref)

    def load_backward(b, c):
        SC.put(b, "in_var", c["var"])
        SC.put(b, "in_go", c["go"])
        SC.put(b, "in_lengths", c["lens"])

    def call_backward(b):
        from nnmnkwii_amd import _hip
        b["out_grad"], b["out_status"] = _hip.backward(b["in_var"], b["in_go"], windows, 3 * sd, b["in_lengths"], out_dtype=torch.float64)

    def verdict_backward(c, b):
        grad, ref = host(b["out_grad"]), c["ref"]
        fails = padded_rows_fail("grad", grad, c["lens"])
        if not np.isfinite(grad).all() or not (np.abs(grad - ref).max(axis=(1, 2)) <= 1e-10 * np.abs(ref).max(axis=(1, 2))).all():
            fails.append("grad")
        return fails + ([] if not host(b["out_status"]).any() else ["status"])

    cell("backward", ["_hip.backward"], make=make_backward, load=load_backward, call=call_backward, verdict=verdict_backward,
         expected=lambda c: [c["ref"]])

    # ---- trim_lengths
    def make_trim(seed):
        from oracle import dtw as OD
        rng = np.random.RandomState(181 + seed)
        X = rng.rand(4, T, 3) + 0.1
        cut = {1: [T - 40, 0, T, 70], 2: [1, T - 1, 64, 0]}[seed]
        for n, k in enumerate(cut):
            X[n, k:] = 0
        X[2, 5:9] = 0                                           # zeros inside stay
        if cut[3] > 4:
            X[3, cut[3] - 1] = 1e-9                             # below eps: trimmed, with the zero frames in front of it
            X[3, cut[3] - 4:cut[3] - 1] = 0
        return dict(X=X, ref=np.array([len(OD.trim_zeros_frames(X[n])) for n in range(4)], dtype=np.int32))

    def call_trim(b):
        from nnmnkwii_amd import _hip
        b["out_lengths"] = _hip.trim_lengths(b["in_X"])

    def load_trim(b, c):
        SC.put(b, "in_X", c["X"])

    cell("trim_lengths", ["_hip.trim_lengths"], make=make_trim, load=load_trim, call=call_trim,
         verdict=lambda c, b: bit_fails(("lengths", b["out_lengths"], c["ref"])), expected=lambda c: [c["ref"]])

    # ---- gather_path
    N, Tsrc, Tout, P = 3, 70, 2 * 64 + 3, 2 * 64 + 9

    def make_gather(seed):
        rng = np.random.RandomState(183 + seed)
        src = rng.randn(N, Tsrc, D)
        plen = np.array({1: [Tout, 9, 1], 2: [0, Tout, 65]}[seed], dtype=np.int32)
        path = np.full((N, P), 7, dtype=np.int32)
        ref = np.zeros((N, Tout, D))
        for n in range(N):
            path[n, :plen[n]] = np.sort(rng.randint(0, Tsrc, size=plen[n]))
            ref[n, :plen[n]] = src[n, path[n, :plen[n]]]
        return dict(src=src, path=path, plen=plen, ref=ref)

    def load_gather(b, c):
        SC.put(b, "in_src", c["src"])
        SC.put(b, "in_idx_path", c["path"])
        SC.put(b, "in_idx_plen", c["plen"])

    def call_gather(b):
        from nnmnkwii_amd import _hip
        b["out_y"] = _hip.gather_path(b["in_src"], b["in_idx_path"], b["in_idx_plen"], Tout)

    cell("gather_path", ["_hip.gather_path"], make=make_gather, load=load_gather, call=call_gather,
         verdict=lambda c, b: bit_fails(("out", b["out_y"], c["ref"])), expected=lambda c: [c["ref"]])

    # ---- stream_copy (the measurement aid: a copy is exact)
    def make_copy(seed):
        return dict(x=np.random.RandomState(185 + seed).randn(3, 1000, 6))

    def load_copy(b, c):
        SC.put(b, "in_x", c["x"])
        SC.out(b, "out_y", c["x"].shape, torch.float64)

    def call_copy(b):
        from nnmnkwii_amd import _hip
        _hip.stream_copy(b["in_x"], b["out_y"])

    cell("stream_copy", ["_hip.stream_copy"], make=make_copy, load=load_copy, call=call_copy,
         verdict=lambda c, b: bit_fails(("copy", b["out_y"], c["x"])), expected=lambda c: [c["x"]])


def _dtw():
    """fastdtw_l2 under both tie rules, the paths bit-exact against the C oracle (tests/test_dtw_gpu.py); A and B differ in lenx and
    leny.  First-minimum: continuous tracks, the cost within 1e-12; diagonal-last: quantised tracks full of ties, the cost exact."""
    N, D, Tx, Ty = 4, 4, 130, 130
    SIZES = {1: [(130, 120), (64, 130), (33, 17), (100, 129)], 2: [(7, 130), (130, 64), (129, 130), (1, 1)]}

    def maker(tie):
        def make(seed):
            from oracle import dtw as OD
            rng = np.random.RandomState(187 + seed + 10 * tie)
            X, Y = np.zeros((N, Tx, D)), np.zeros((N, Ty, D))
            paths = []
            for n, (tx, ty) in enumerate(SIZES[seed]):
                x, y = np.cumsum(rng.randn(tx, D), 0) * 0.1, np.cumsum(rng.randn(ty, D), 0) * 0.1
                if tie:
                    x, y = np.round(x * 4) / 4, np.round(y * 4) / 4
                X[n, :tx], Y[n, :ty] = x, y
                paths.append(OD.fastdtw(x, y, 1, tie=tie))
            lens = np.array(SIZES[seed], dtype=np.int32)
            return dict(X=X, Y=Y, lenx=np.ascontiguousarray(lens[:, 0]), leny=np.ascontiguousarray(lens[:, 1]), paths=paths)
        return make

    def load(b, c):
        SC.put(b, "in_X", c["X"])
        SC.put(b, "in_Y", c["Y"])
        SC.put(b, "in_idx_lenx", c["lenx"])
        SC.put(b, "in_idx_leny", c["leny"])

    def call(b, tie):
        from nnmnkwii_amd import _hip
        b["out_pi"], b["out_pj"], b["out_pl"], b["out_cost"] = _hip.fastdtw_l2(b["in_X"], b["in_Y"], b["in_idx_lenx"], b["in_idx_leny"], 1, tie_rule=tie)

    def verdict(c, b, tie):
        pi, pj, pl, cost = (host(b[k]) for k in ("out_pi", "out_pj", "out_pl", "out_cost"))
        fails = []
        for n, (d, path) in enumerate(c["paths"]):
            k = int(pl[n])
            if k != len(path) or not (np.array_equal(pi[n, :k], path[:, 0]) and np.array_equal(pj[n, :k], path[:, 1])):
                fails.append("path %d" % n)
            elif not (cost[n] == d if tie else abs(cost[n] - d) <= 1e-12 * max(d, 1e-300)):
                fails.append("cost %d" % n)
        return fails

    def expected(c):
        pi = np.zeros((N, Tx + Ty), dtype=np.int32)
        pj = np.zeros((N, Tx + Ty), dtype=np.int32)
        for n, (_, path) in enumerate(c["paths"]):
            pi[n, :len(path)], pj[n, :len(path)] = path[:, 0], path[:, 1]
        return [pi, pj, np.array([len(p) for _, p in c["paths"]], dtype=np.int32), np.array([d for d, _ in c["paths"]])]

    def defined(b):
        """The path's slots up to its length (the header promises nothing behind it), the lengths and the costs."""
        pi, pj, pl, cost = (host(b[k]) for k in ("out_pi", "out_pj", "out_pl", "out_cost"))
        behind = np.arange(pi.shape[1])[None, :] >= pl[:, None]
        return dict(pi=np.where(behind, 0, pi), pj=np.where(behind, 0, pj), pl=pl, cost=cost)

    for tie, name in ((0, "first_min"), (1, "diag_last")):
        cell("fastdtw_l2[%s]" % name, ["_hip.fastdtw_l2"], make=maker(tie), load=load, call=functools.partial(call, tie=tie),
             verdict=functools.partial(verdict, tie=tie), expected=expected, defined=defined)

    # ---- fastdtw_callable: the host evaluates every level's costs, so no capture
    CS = {1: [(40, 33), (17, 40)], 2: [(9, 40), (40, 38)]}

    def make_callable(seed):
        from oracle import dtw as OD
        rng = np.random.RandomState(189 + seed)
        xs = [np.cumsum(rng.randn(tx, 3), 0) * 0.1 for tx, _ in CS[seed]]
        ys = [np.cumsum(rng.randn(ty, 3), 0) * 0.1 for _, ty in CS[seed]]
        return dict(xs=xs, ys=ys, paths=[OD.fastdtw(x, y, 1) for x, y in zip(xs, ys)])

    def load_callable(b, c):
        b["case"] = c

    def call_callable(b):
        from oracle import dtw as OD
        from nnmnkwii_amd import _hip
        pi, pj, pl, cost = _hip.fastdtw_callable(b["case"]["xs"], b["case"]["ys"], 1, OD.l2)
        b["out_pi"], b["out_pj"], b["out_pl"], b["out_cost"] = (torch.from_numpy(a).cuda() for a in (pi, pj, pl, cost))

    def expected_callable(c):
        pi = np.zeros((len(c["paths"]), 100), dtype=np.int32)
        for n, (_, path) in enumerate(c["paths"]):
            pi[n, :len(path)] = path[:, 0]
        return [pi, np.array([len(p) for _, p in c["paths"]], dtype=np.int32), np.array([d for d, _ in c["paths"]])]

    cell("fastdtw_callable", ["_hip.fastdtw_callable"], make=make_callable, load=load_callable, call=call_callable,
         verdict=functools.partial(verdict, tie=0), expected=expected_callable, defined=defined, capture=False,
         why="level by level from the coarsest, the local costs of each level's window cells evaluated HERE by ``dist`` -- one call per "
             "cell, as upstream fastdtw does")


def _modspec():
    """modspec, inv_modspec, modspec_smoothing and modspec_backward at one DFT length per route -- 0 the in-LDS FFT, 2 chirp-z, 1 the
    direct transform, each asked of modspec_route -- against oracle/modspec.py with the bounds of tests/test_modspec_chirp_gpu.py:
    spectrum and inverse 1e-11, smoothing 1e-9, gradient 1e-10 of the reference's maximum, phases within 1e-8 where the bin is not
    vanishing."""
    B, D = 3, 5
    ROUTES = ((64, 0), (100, 2), (2050, 1))

    def maker(n):
        def make(seed):
            from oracle import modspec as OM
            rng = np.random.RandomState(190 + seed + n)
            T = n - 3
            x = 0.1 * np.cumsum(rng.randn(B, T, D), axis=-2) + rng.rand(B, T, D)
            w = rng.rand(B, n // 2 + 1, D)
            limit_bin = min(int(n * 25 / 200) + 1, n // 2 + 1)
            per = lambda f, *arrs: np.stack([f(*[a[b] for a in arrs]) for b in range(B)])  # noqa: E731
            ms = per(lambda a: OM.modspec(a, n=n), x)
            ph = per(lambda a: OM.modspec(a, n=n, return_phase=True)[1], x)
            return dict(x=x, w=w, n=n, limit_bin=limit_bin, ms=ms, ph=ph, inv=per(lambda m, p: OM.inv_modspec(m, p), ms, ph),
                        smooth=per(lambda a: OM.modspec_smoothing(a, 200, n=n, cutoff=25, log_domain=True), x),
                        grad=per(lambda a, g: OM.modspec_grad(a, g, n, None), x, w))
        return make

    def load(b, c):
        SC.put(b, "in_x", c["x"])
        SC.put(b, "in_w", c["w"])
        SC.put(b, "in_ms", c["ms"])
        ph = c["ph"]
        SC.put(b, "in_ph", np.stack([ph.real, ph.imag], axis=-1) if np.iscomplexobj(ph) else ph)

    def call_modspec(b, n):
        from nnmnkwii_amd import _hip
        b["out_ms"], b["out_ph"] = _hip.modspec(b["in_x"], n, want_phase=True)

    def verdict_modspec(c, b):
        fails = far_fails(("ms", b["out_ms"], c["ms"], 1e-11))
        ph = host(b["out_ph"])
        ph = ph[..., 0] + 1j * ph[..., 1]
        big = c["ms"] > 1e-6 * c["ms"].max()
        po = c["ph"] if np.iscomplexobj(c["ph"]) else c["ph"][..., 0] + 1j * c["ph"][..., 1]
        return fails + ([] if np.abs(ph - po)[big].max() < 1e-8 else ["phase"])

    def call_inv(b, n):
        from nnmnkwii_amd import _hip
        b["out_x"] = _hip.inv_modspec(b["in_ms"], b["in_ph"])

    def call_smooth(b, n, limit_bin):
        from nnmnkwii_amd import _hip
        b["out_y"] = _hip.modspec_smoothing(b["in_x"], n, limit_bin, log_domain=True)

    def call_backward(b, n):
        from nnmnkwii_amd import _hip
        b["out_g"] = _hip.modspec_backward(b["in_x"], b["in_w"], n)

    for n, route in ROUTES:
        make = maker(n)
        tag = "[n=%d,route=%d]" % (n, route)

        def load_checked(b, c, n=n, route=route):
            from nnmnkwii_amd import _hip
            assert _hip.modspec_route(n) == route, (n, _hip.modspec_route(n), route)
            load(b, c)
        cell("modspec" + tag, ["_hip.modspec"], make=make, load=load_checked, call=functools.partial(call_modspec, n=n), verdict=verdict_modspec,
             expected=lambda c: [c["ms"]])
        cell("inv_modspec" + tag, ["_hip.inv_modspec"], make=make, load=load_checked, call=functools.partial(call_inv, n=n),
             verdict=lambda c, b: far_fails(("x", b["out_x"], c["inv"], 1e-11)), expected=lambda c: [c["inv"]])
        cell("modspec_smoothing" + tag, ["_hip.modspec_smoothing"], make=make, load=load_checked,
             call=functools.partial(call_smooth, n=n, limit_bin=min(int(n * 25 / 200) + 1, n // 2 + 1)),
             verdict=lambda c, b: far_fails(("y", b["out_y"], c["smooth"], 1e-9)), expected=lambda c: [c["smooth"]])
        cell("modspec_backward" + tag, ["_hip.modspec_backward"], make=make, load=load_checked, call=functools.partial(call_backward, n=n),
             verdict=lambda c, b: far_fails(("grad", b["out_g"], c["grad"], 1e-10)), expected=lambda c: [c["grad"]])


def _modspec_batch():
    """modspec_batch and modspec_batch_backward on both routes, and the fused loss step -- on side streams only -- against
    tests/modspec_batch64.py with the float64 bounds of tests/test_modspec_batch_gpu.py: spectrum and loss 1e-11, gradients 1e-10."""
    import modspec_batch64 as R
    B, D = 4, 5

    def maker(n):
        T = n + 8
        LENS = {1: [T, n // 2 + 1, 0, (3 * n) // 4], 2: [0, T, n - 1, 5]}

        def make(seed):
            rng = np.random.RandomState(191 + seed + n)
            x = R.make_batch(rng, B, T, D, LENS[seed])
            w = rng.rand(B, n // 2 + 1, D)
            tgt = R.modspec(R.make_batch(rng, B, T, D, LENS[seed]), n, None, LENS[seed]) + 0.01
            return dict(x=x, w=w, tgt=tgt, n=n, lens=np.array(LENS[seed], dtype=np.int32), live=R.live_frames(LENS[seed], B, T, n),
                        ms=R.modspec(x, n, None, LENS[seed]), grad=R.modspec_grad(x, w, n, None, LENS[seed]),
                        loss=R.loss_and_grad(x, tgt, n, None, LENS[seed], True, 1e-10))
        return make

    def load(b, c):
        SC.put(b, "in_x", c["x"])
        SC.put(b, "in_w", c["w"])
        SC.put(b, "in_tgt", c["tgt"])
        SC.put(b, "in_lengths", c["lens"])

    def call_ms(b, n):
        from nnmnkwii_amd import _hip
        b["out_ms"] = _hip.modspec_batch(b["in_x"], n, lengths=b["in_lengths"])

    def call_bwd(b, n):
        from nnmnkwii_amd import _hip
        b["out_g"] = _hip.modspec_batch_backward(b["in_x"], b["in_w"], n, lengths=b["in_lengths"])

    def call_loss(b, n):
        from nnmnkwii_amd import _hip
        assert _hip.modspec_loss_form(n) == 1
        b["out_loss"], b["out_g"] = _hip.modspec_loss_step(b["in_x"], b["in_tgt"], n, False, b["in_lengths"], True, 1e-10)

    for n in (64, 100):
        make = maker(n)
        tag = "[n=%d]" % n
        cell("modspec_batch" + tag, ["_hip.modspec_batch"], make=make, load=load, call=functools.partial(call_ms, n=n),
             verdict=lambda c, b: far_fails(("ms", b["out_ms"], c["ms"], 1e-11)), expected=lambda c: [c["ms"]])
        cell("modspec_batch_backward" + tag, ["_hip.modspec_batch_backward"], make=make, load=load, call=functools.partial(call_bwd, n=n),
             verdict=lambda c, b: far_fails(("grad", b["out_g"], c["grad"], 1e-10)) + padded_rows_fail("grad", b["out_g"], c["live"]),
             expected=lambda c: [c["grad"]])
    # (the step takes its stream from the helper that keeps its workspace: that helper is the one that asks for the stream)
    cell("modspec_loss_step[n=64]", ["_hip._ms_loss_workspace"], documented_by="_hip.modspec_loss_step", make=maker(64), load=load,
         call=functools.partial(call_loss, n=64),
         verdict=lambda c, b: far_fails(("loss", b["out_loss"], np.asarray(c["loss"][0]), 1e-11), ("grad", b["out_g"], c["loss"][1], 1e-10))
         + padded_rows_fail("grad", b["out_g"], c["live"]),
         expected=lambda c: [np.asarray(c["loss"][0]), c["loss"][1]], capture=False,
         why="The per-(device, stream) workspace is allocated on first use and again when a batch outgrows it: capturing the step "
             "into a graph is not supported.")


for _family in (_frontend, _silence, _joint, _f0, _wave, _metrics, _postfilter, _msfilter, _gmmtraj, _gv, _gmm, _kmeans, _small_entries,
                _dtw, _modspec, _modspec_batch):
    _family()


# The wrappers that pass a stream to the library and have their stream or capture test elsewhere (tests/test_stream_contract_cpu.py
# requires every such wrapper to be in the table above or here, and every target to exist).
COVERED_ELSEWHERE = {
    "_hip.forward": "tests/test_strip_gpu.py::test_strip_kernel_inside_a_hip_graph",
    "_hip.backward_var": "tests/test_var_grad_gpu.py::test_graph_capture_and_repeatability",
    "_hip.forward_streams": "tests/test_stream_routes_gpu.py::test_graph_capture_with_side_streams_and_a_merged_launch_replays_bit_identically",
    "_hip.backward_streams": "tests/test_backward_streams_gpu.py::test_graph_capture_replays_equal_eager",
    "_hip.unit_mse_form": "tests/test_autograd_gpu.py::test_fused_step_inside_a_stream_capture_needs_a_warm_up_and_says_so",
    "_hip._mse_workspace": "tests/test_autograd_gpu.py::test_fused_step_inside_a_stream_capture_needs_a_warm_up_and_says_so",
    "_hip.column_stats": "tests/test_norm_gpu.py::test_capturable_into_a_graph_once_the_workspace_exists",
    "_hip.column_affine": "tests/test_norm_gpu.py::test_capturable_into_a_graph_once_the_workspace_exists",
}


# ---- the three checks over the table ---------------------------------------------------------------------------------------------------

CAPTURED = [c for c in CELLS if c.capture]


@pytest.mark.parametrize("cell", CAPTURED, ids=[c.name for c in CAPTURED])
def test_replayed_on_new_data(cell):
    SC.replayed_on_new_data(cell)


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_two_streams_interleaved(cell):
    SC.two_streams_interleaved(cell)


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_behind_a_late_producer(cell):
    SC.behind_a_late_producer(cell)


SCRATCH_USERS = [c for c in CELLS if c.name.split("[")[0] in ("modspec", "inv_modspec", "modspec_smoothing", "modspec_backward", "modspec_batch",
                                                              "modspec_batch_backward", "fastdtw_l2", "fastdtw_callable", "backward")]


def test_calls_of_other_entries_and_shapes_share_one_stream_s_scratch():
    """The entries that keep tables or control words in the library's per-(device, stream) scratch -- the DTW kernels, the DTW cost
    levels, the direct and chirp-z modspec routes at two lengths, the MLPG solve -- back to back on one stream, forwards and
    backwards: the slot they share is grown, refilled and reused between them."""
    assert len(SCRATCH_USERS) == 20
    SC.one_stream_shared(SCRATCH_USERS)


# ---- the checks themselves: a well-behaved stand-in passes, planted contract bugs are caught ---------------------------------------------

def _stand_in(kind):
    """y = 2 x on the live frames, 0 behind them, written with torch operations: "good" on the current stream from device lengths;
    "other stream": the same work sent to a stream of its own, as a launch on the wrong stream would be; "host lengths": the
    lengths read on the host when the buffers were loaded first, as a wrapper that bakes device data into its launch would."""
    B, Tmax, D = 3, 40, 4
    LENS = {1: [Tmax, 7, 0], 2: [0, Tmax, 21]}

    def make(seed):
        x = np.random.RandomState(195 + seed).randn(B, Tmax, D)
        lens = np.array(LENS[seed], dtype=np.int32)
        return dict(x=x, lens=lens, ref=np.where((np.arange(Tmax)[None, :] < lens[:, None])[:, :, None], 2 * x, 0.0))

    def load(b, c):
        SC.put(b, "in_x", c["x"])
        SC.put(b, "in_lengths", c["lens"])
        SC.out(b, "out_y", (B, Tmax, D), torch.float64)
        if "other" not in b:
            b["other"], b["host_lengths"] = torch.cuda.Stream(), [int(n) for n in c["lens"]]
            b["frames"] = torch.arange(Tmax, dtype=torch.int32, device="cuda")[None, :].expand(B, Tmax).contiguous()
            b["dead"] = torch.empty((B, Tmax), dtype=torch.bool, device="cuda")

    def work(b):
        """(no allocation: the stream this runs on may not be the one a capture routes to its pool)"""
        torch.ge(b["frames"], b["in_lengths"][:, None], out=b["dead"])
        torch.mul(b["in_x"], 2.0, out=b["out_y"])
        b["out_y"].masked_fill_(b["dead"][:, :, None], 0.0)

    def call(b):
        if kind == "good":
            work(b)
        elif kind == "other stream":
            with torch.cuda.stream(b["other"]):
                work(b)
        else:
            b["out_y"].zero_()
            for u, n in enumerate(b["host_lengths"]):
                b["out_y"][u, :n] = 2 * b["in_x"][u, :n]

    return SC.Cell("stand-in, " + kind, [], make=functools.lru_cache(maxsize=None)(make), load=load, call=call,
                   verdict=lambda c, b: bit_fails(("y", b["out_y"], c["ref"])), expected=lambda c: [c["ref"]])


def test_a_well_behaved_stand_in_passes_the_three_checks():
    good = _stand_in("good")
    assert SC.pair_conditions(good) == []
    SC.replayed_on_new_data(good)
    SC.two_streams_interleaved(good)
    SC.behind_a_late_producer(good)


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_work_sent_to_another_stream_is_caught():
    """Not recorded by the capture: the replay leaves the poison.  Not behind the late producer: it reads the poison."""
    with pytest.raises(AssertionError, match="the replay on case B"):
        SC.replayed_on_new_data(_stand_in("other stream"))
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match="behind a late producer"):
        SC.behind_a_late_producer(_stand_in("other stream"))
    torch.cuda.synchronize()


def test_device_data_read_on_the_host_is_caught():
    """Right on the data it was loaded with, wrong on the first replay with other lengths."""
    with pytest.raises(AssertionError, match="the replay on case B"):
        SC.replayed_on_new_data(_stand_in("host lengths"))
    torch.cuda.synchronize()
