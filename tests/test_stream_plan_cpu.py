"""The restated stream plan (tests/stream_plan.py) on the layouts the comments of streams_api.hip plan_streams work by
hand.  No GPU: this pins the restatement that tests/test_stream_routes_gpu.py predicts launch counters with."""
import numpy as np
import pytest

import stream_plan as SP
from cases import WINDOW_SETS


def _table(spec):
    """spec: [(static_dim, window-set name or None)] -> (streams, l[], u[], coeff[], ld_in); one table entry per distinct name,
    streams packed side by side in the input and the output."""
    wl, wu, wc, first = [], [], [], {}
    streams, col, oc = [], 0, 0
    for sd, name in spec:
        nw = 0
        if name is not None:
            if name not in first:
                first[name] = len(wl)
                base = WINDOW_SETS[name.split("#")[0]]
                for l, u, c in base:
                    wl.append(l)
                    wu.append(u)
                    wc.extend(np.asarray(c, dtype=np.float64).ravel().tolist())
            nw = len(WINDOW_SETS[name.split("#")[0]])
        streams.append(dict(in_col=col, out_col=oc, static_dim=sd, num_windows=nw, win_first=first.get(name, 0)))
        col += max(nw, 1) * sd
        oc += sd
    return streams, np.array(wl, dtype=np.int32), np.array(wu, dtype=np.int32), np.array(wc), col


def _plan(spec, algo=SP.STRIP, mode=SP.VAR_FRAME, B=6, T=300, tweak=None):
    streams, wl, wu, wc, ld = _table(spec)
    if tweak is not None:
        tweak(wc)
    return SP.merge_plan(streams, wl, wu, wc, algo, mode, SP.F64, B, T, ld, ld)


def test_merlin_row_fills_64_lanes_and_cuts_bap():
    p = _plan([(60, "std3"), (1, "std3"), (1, None), (5, "std3")])
    assert p.merged and p.cap == 64
    assert p.lanes == [(0, 0, 60), (1, 60, 1), (3, 61, 3)]
    assert (p.piece, p.piece_first) == (3, 3)               # bap dims 0-2 on the lanes, 3-4 as a piece
    assert p.alone == [2, 3]                                # vuv (pass-through) and bap's piece


def test_two_wide_and_one_narrow_trim_to_128_lanes():
    p = _plan([(60, "std3"), (60, "std3"), (10, "std3")])
    assert p.merged and p.cap == 128                        # 130 % 64 = 2 < 32
    assert p.lanes == [(0, 0, 60), (1, 60, 60), (2, 120, 8)]
    assert (p.piece, p.piece_first) == (2, 8)               # a piece of 2 dims
    assert p.alone == [2]


def test_four_member_cap_leaves_the_fifth_alone():
    p = _plan([(60, "std3")] + [(1, "std3")] * 4)
    assert p.merged and p.cap == 64
    assert p.members == [0, 1, 2, 3] and p.piece == -1
    assert p.alone == [4]


def test_sixty_and_forty_make_two_groups_without_a_trim():
    p = _plan([(60, "std3"), (40, "std3")])
    assert p.merged and p.cap == 100 and p.piece == -1      # 100 % 64 = 36 >= 32
    assert p.lanes == [(0, 0, 60), (1, 60, 40)] and p.alone == []


def test_equal_windows_in_distinct_entries_merge_one_ulp_apart_do_not():
    spec = [(30, "std3"), (20, "std3#copy")]
    p = _plan(spec)
    assert p.merged and p.members == [0, 1]
    # the second entry's last coefficient moved by one ulp: memcmp differs
    p = _plan(spec, tweak=lambda wc: wc.__setitem__(-1, np.nextafter(wc[-1], 2.0)))
    assert not p.merged and p.alone == [0, 1]


def test_wide3_member_is_not_eligible():
    p = _plan([(30, "std3"), (20, "wide3"), (10, "std3")])
    assert p.merged and p.members == [0, 2] and p.alone == [1]
    p = _plan([(30, "wide3"), (20, "wide3")], algo=SP.AUTO, T=1100)
    assert not p.merged


def test_zero_dim_streams_and_pass_through_are_skipped():
    p = _plan([(40, "std3"), (0, "std3"), (3, None), (20, "std3")])
    assert p.merged and p.members == [0, 3] and p.alone == [2]


def test_merge_conditions_per_family():
    spec = [(60, "std3"), (1, "std3"), (5, "std3")]
    assert not _plan(spec, algo=SP.WAVE).attempted
    assert not _plan(spec, algo=SP.CONST, mode=SP.VAR_FRAME).attempted
    assert not _plan(spec, algo=SP.STRIP, mode=SP.VAR_GLOBAL).attempted
    assert _plan(spec, algo=SP.CONST, mode=SP.VAR_UNIT, B=1).merged
    # AUTO: per-frame variances merge for long utterances or enough strips, global / unit ones from 192 (utterance, group)s
    assert not _plan(spec, algo=SP.AUTO, T=300, B=6).merged
    assert _plan(spec, algo=SP.AUTO, T=1100, B=1).merged
    assert _plan(spec, algo=SP.AUTO, T=65, B=256).merged                 # 256 x 2 strips >= 512
    assert not _plan(spec, algo=SP.AUTO, mode=SP.VAR_GLOBAL, B=191).merged
    assert _plan(spec, algo=SP.AUTO, mode=SP.VAR_GLOBAL, B=192).merged
    # strip kernel beyond 256 strips: no merged launch even when forced
    assert not _plan(spec, algo=SP.STRIP, T=256 * 64 + 1).merged


def test_forced_family_counters_and_refusals():
    streams, wl, wu, wc, ld = _table([(60, "std3"), (1, "std3"), (1, None), (5, "std3")])
    # STRIP, per-frame: merged launch + bap's 2-dim piece on the transposed form (B >= 2), the wave kernel (B = 1, T <= 2048),
    # the natural-order kernel (B = 1, T > 2048)
    for B, T, kind in ((6, 300, SP.K_STRIP_TR), (1, 300, SP.K_WAVE), (1, 2100, SP.K_GENERIC)):
        plan, kinds, n = SP.predict(streams, wl, wu, wc, SP.STRIP, SP.VAR_FRAME, SP.F64, B, T, ld, ld, False)
        assert kinds == {SP.K_STRIP_MULTI: 1, kind: 1} and n == 2, (B, T, kinds)
    # CONST, global: the piece goes to AUTO's choice for a piece
    plan, kinds, n = SP.predict(streams, wl, wu, wc, SP.CONST, SP.VAR_GLOBAL, SP.F64, 6, 300, ld, ld, True)
    assert kinds == {SP.K_CONST_MULTI: 1, SP.K_WAVE: 1}
    plan, kinds, n = SP.predict(streams, wl, wu, wc, SP.CONST, SP.VAR_UNIT, SP.F32, 192, 1100, ld, ld, False)
    assert kinds == {SP.K_CONST_MULTI: 1, SP.K_STRIP_TR: 1}
    # AUTO: not exact, but the number of launches is
    plan, kinds, n = SP.predict(streams, wl, wu, wc, SP.AUTO, SP.VAR_FRAME, SP.F64, 6, 300, ld, ld, True)
    assert kinds is None and not plan.merged and n == 3
    mixed, wl, wu, wc, ld = _table([(8, "std3"), (6, "wide3"), (4, "asym2"), (3, "static"), (5, "zero2"), (2, None)])
    for algo in (SP.WAVE, SP.STRIP, SP.CONST):
        with pytest.raises(SP.Refused) as ei:
            SP.predict(mixed, wl, wu, wc, algo, SP.VAR_GLOBAL if algo == SP.CONST else SP.VAR_FRAME, SP.F64, 6, 300, ld, ld, True)
        assert str(ei.value) == "MLPG_HIP_ALGO_" + SP.ALGO_NAME[algo]
    plan, kinds, n = SP.predict(mixed, wl, wu, wc, SP.GENERIC, SP.VAR_FRAME, SP.F64, 6, 300, ld, ld, True)
    assert kinds == {SP.K_GENERIC: 5} and not plan.attempted


# ---------------------------------------------------------------------------------------------------- the 2 GB window rule

def test_rows_fit_buffer_is_the_rule_of_common_h():
    """Tmax * ld * 8 < 2^31 - 1 whatever the dtype: 130 rows of 2064888 elements are 2^31 - 128 bytes, one element more per
    row is past the line."""
    assert 130 * 2064888 * 8 == 2 ** 31 - 128
    assert SP.rows_fit_buffer(130, 2064888) and not SP.rows_fit_buffer(130, 2064889)
    assert SP.rows_fit_buffer(1, 268435455) and not SP.rows_fit_buffer(1, 268435456)      # 2^31 - 8 | 2^31 bytes
    assert SP.rows_fit_buffer(0, 0) and SP.rows_fit_buffer(2048, 131071) and not SP.rows_fit_buffer(2048, 131072)


def test_every_family_that_needs_the_window_is_refused_beyond_it_and_the_plan_does_not_merge():
    spec = [(60, "std3"), (1, "std3"), (5, "std3")]
    streams, wl, wu, wc, _ = _table(spec)
    wide_streams, wl2, wu2, wc2, _ = _table([(24, "wide3")])
    for ld, fits in ((2064888, True), (2064889, False)):
        for algo, mode, dt, tab in ((SP.STRIP, SP.VAR_FRAME, SP.F64, (streams, wl, wu, wc)),
                                    (SP.CONST, SP.VAR_GLOBAL, SP.F64, (streams, wl, wu, wc)),
                                    (SP.CHUNK, SP.VAR_FRAME, SP.F64, (wide_streams, wl2, wu2, wc2)),
                                    (SP.FIR, SP.VAR_UNIT, SP.F32, (streams, wl, wu, wc))):
            for ld_in, ld_out in ((ld, 66), (200, ld)):                                   # the wide side is either one
                if fits:
                    plan, kinds, n = SP.predict(*tab, algo, mode, dt, 3, 130, ld_in, ld_out, False)
                    assert plan.merged == (algo in (SP.STRIP, SP.CONST)), (algo, ld_in, ld_out)
                else:
                    with pytest.raises(SP.Refused) as ei:
                        SP.predict(*tab, algo, mode, dt, 3, 130, ld_in, ld_out, False)
                    assert str(ei.value) == "MLPG_HIP_ALGO_" + SP.ALGO_NAME[algo]
        # the families that take any stride, and AUTO, which then has only those: no merged launch
        for algo, kind in ((SP.WAVE, SP.K_WAVE), (SP.GENERIC, SP.K_GENERIC)):
            plan, kinds, n = SP.predict(streams, wl, wu, wc, algo, SP.VAR_FRAME, SP.F64, 3, 130, ld, 66, False)
            assert kinds == {kind: 3} and not plan.attempted
        for mode, B, T in ((SP.VAR_FRAME, 1, 1100), (SP.VAR_GLOBAL, 192, 130)):
            ld_t = ld if T == 130 else (244032 if fits else 244033)                       # 1100 * 244033 * 8 >= 2^31 - 1
            plan, kinds, n = SP.predict(streams, wl, wu, wc, SP.AUTO, mode, SP.F64, B, T, ld_t, 66, False)
            assert plan.attempted and plan.merged == fits and n == (2 if fits else 3), (mode, fits, plan)
    # the transposed form has the rule for its group of u = 64 // sd utterances
    ws = SP.Win(wl, wu, wc, 0, 3)
    assert 12 * 130 * 172074 * 8 < 2147483647 <= 12 * 130 * 172075 * 8
    assert SP.strip_tr_supported(24, 130, 5, 172074, ws) and not SP.strip_tr_supported(24, 130, 5, 172075, ws)
    assert SP.strip_supported(130, ws, 172075)                                            # the plain form still takes it
    assert SP.solo_kind(None, ws, SP.STRIP, SP.VAR_FRAME, SP.F64, 24, 130, False, 172074, 5, False) == SP.K_STRIP_TR
    assert SP.solo_kind(None, ws, SP.STRIP, SP.VAR_FRAME, SP.F64, 24, 130, False, 172075, 5, False) == SP.K_STRIP


def test_the_rule_changes_no_prediction_of_the_route_tests(monkeypatch):
    """Every problem tests/test_stream_routes_gpu.py builds lies inside the window, for the transposed form's group too, and
    is predicted as it was before the rule was restated."""
    import test_stream_routes_gpu as R
    cells = list(R.CELLS) + list(R.SWEEP)
    assert len(cells) > 300
    with_rule = []
    for lname, dt, mode, ragged, algo, T, B, _ in cells:
        lay = R.layout(lname)
        ld = max(lay.ld_in, lay.ld_out)
        assert SP.rows_fit_buffer(T, ld) and 64 * T * ld * 8.0 < 2147483647.0, (lname, T, ld)
        with_rule.append(lay.predict(algo, mode, dt, B, T, ragged))
    monkeypatch.setattr(SP, "rows_fit_buffer", lambda T, ld: True)
    for cell, want in zip(cells, with_rule):
        lname, dt, mode, ragged, algo, T, B, _ = cell
        assert R.layout(lname).predict(algo, mode, dt, B, T, ragged) == want, cell
    for spec in (R.LAY_SIDE,):
        lay = R.Layout(spec, 11)
        assert SP.rows_fit_buffer(1100, max(lay.ld_in, lay.ld_out))
