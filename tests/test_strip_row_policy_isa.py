"""The cache policy of level 1's row loads (row_load_aux, csrc/mlpg_strip_impl.h), statically (needs hipcc, no GPU).

The standard-window forward float64 unit is compiled to device assembly twice, with the default MLPG_STRIP_ROW_POLICY and with
-DMLPG_STRIP_ROW_POLICY=0.  The policy may change nothing but the suffix of buffer_load lines: the two texts must be equal once
that suffix is removed (tools/strip_isa_stats.py, policy_blind), and the registers must be the same.  In the default text the
interior copy of level 1 -- one basic block of straight-line code -- must hold `nt` loads for the 14 frames of a chunk that no
other chunk reads and plain loads for the 4 boundary frames -1, 0, kM-1, kM; the EDGE copy, which clamps its rows at run
time, stays plain throughout.

The expected counts come from the rule and from what the standard set loads per frame, not from the compiled text: a frame is
three windows of variance and of mean, six loads; window 0 of the standard set has the single tap [1], so frames -1 and kM,
which only reach the chunk's rows through the two dynamic windows, are four loads each (the compiler drops the loads nothing
reads)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import strip_isa_stats as S  # noqa: E402

pytestmark = pytest.mark.skipif(S.find_hipcc() is None, reason="hipcc not found")

UNIT = "mlpg_strip_std_fwd_f64.hip"
STD = ["d", "d", "Lb0E", "Li0E", "Lb0E", "Lb1E", "Lb0E", "Lb1E"]  # <TIN, TOUT, BWD, VM, MULTI, NW3, TR, STD>
KM = 16  # frames per chunk (MLPG_STRIP_M)
FRAMES = range(-1, KM + 1)


def row_load_aux(i, policy=1):
    """The rule of mlpg_strip_impl.h, restated: 0 for the four boundary frames, 2 (nt) for the others."""
    return 2 if policy and i not in (-1, 0, KM - 1, KM) else 0


def std_loads(i):
    """Row loads of frame i in the STD forward instance with per-frame variances: (variance + mean) x windows that reach the chunk."""
    return 2 * (2 if i in (-1, KM) else 3)


def _loads_by_block(asm):
    """[(block label, nt loads, plain loads)] of the strip_kernel instance, for blocks with row loads; and the descriptors seen."""
    blocks, descs, inside, cur = {}, set(), False, None
    for line in asm.splitlines():
        t = line.strip()
        m = re.match(r"\.type\s+(\S+),@function", t)
        if m:
            inside = S.template_args(m.group(1)) == STD
            cur = "entry"
            continue
        if not inside:
            continue
        if t.startswith(".Lfunc_end"):
            inside = False
            continue
        m = re.match(r"(\.LBB\w+):", t)
        if m:
            cur = m.group(1)
            continue
        if t.startswith("buffer_load_"):
            code = t.split(";")[0]
            d = re.search(r"s\[\d+:\d+\]", code)
            assert d, t
            descs.add(d.group(0))
            n = blocks.setdefault(cur, [0, 0])
            n[0 if re.search(r"\snt\b", code) else 1] += 1
    return [(b, n[0], n[1]) for b, n in blocks.items()], descs


@pytest.fixture(scope="module")
def texts():
    return S.assembly(UNIT), S.assembly(UNIT, extra=["-DMLPG_STRIP_ROW_POLICY=0"])


def test_policy_blind_on_a_snippet():
    a = "\tbuffer_load_dwordx2 v[0:1], v2, s[8:11], s3 offen nt\n\tbuffer_store_dwordx2 v[0:1], v2, s[8:11], s3 offen nt\n\tv_mov_b32 v1, v2 ; nt\n"
    b = a.replace("s3 offen nt\n\tbuffer_store", "s3 offen\n\tbuffer_store")
    assert a != b and S.policy_blind(a) == S.policy_blind(b)
    assert "buffer_store_dwordx2 v[0:1], v2, s[8:11], s3 offen nt" in S.policy_blind(a)  # stores keep theirs
    assert S.policy_blind(a) != S.policy_blind(a.replace("s3 offen nt\n\tbuffer_store", "s4 offen nt\n\tbuffer_store"))
    assert S.policy_blind("\tbuffer_load_dword v0, v2, s[8:11], 0 offen sc0 sc1 nt\n") == "\tbuffer_load_dword v0, v2, s[8:11], 0 offen"


def test_the_rule_holds_14_nt_frames_and_4_plain_ones():
    assert [i for i in FRAMES if row_load_aux(i) == 0] == [-1, 0, KM - 1, KM]
    assert sum(1 for i in FRAMES if row_load_aux(i) == 2) == 14
    assert all(row_load_aux(i, policy=0) == 0 for i in FRAMES)
    # the header states the same rule
    with open(os.path.join(S.CSRC, "mlpg_strip_impl.h")) as f:
        src = f.read()
    assert "MLPG_STRIP_ROW_POLICY && !(i == -1 || i == 0 || i == kM - 1 || i == kM) ? 2 : 0" in src
    with open(os.path.join(S.CSRC, "mlpg_strip_geom.h")) as f:
        assert re.search(r"#define MLPG_STRIP_M %d\b" % KM, f.read())


def test_policy_changes_nothing_but_the_suffix(texts):
    on, off = texts
    assert S.digest(on) != S.digest(off)
    assert S.digest(S.policy_blind(on)) == S.digest(S.policy_blind(off))
    assert S.policy_blind(off).splitlines() == [line for line in off.splitlines()]  # policy 0: no suffix on any load


def test_interior_copy_loads_by_the_rule(texts):
    on, off = texts
    blocks, descs = _loads_by_block(on)
    print("blocks with row loads (label, nt, plain):", blocks, "descriptors:", sorted(descs))
    assert len(descs) == 2  # means and variances
    want_nt = sum(std_loads(i) for i in FRAMES if row_load_aux(i) == 2)
    want_plain = sum(std_loads(i) for i in FRAMES if row_load_aux(i) == 0)
    assert (want_nt, want_plain) == (14 * 6, 2 * 6 + 2 * 4)
    with_nt = [b for b in blocks if b[1]]
    assert len(with_nt) == 1, blocks  # level 1's interior copy: straight-line code
    assert with_nt[0][1:] == (want_nt, want_plain)
    # the EDGE copy: every frame plain
    others = [b for b in blocks if not b[1]]
    assert sum(b[2] for b in others) == sum(std_loads(i) for i in FRAMES), blocks
    # the A side: no nt load anywhere
    blocks0, _ = _loads_by_block(off)
    assert sum(b[1] for b in blocks0) == 0 and sum(b[2] for b in blocks0) == sum(b[1] + b[2] for b in blocks)


def test_no_scratch_and_the_same_registers(texts):
    on, off = (S.parse(t) for t in texts)
    pick = lambda st: [v for k, v in st.items() if S.template_args(k) == STD]
    (a,), (b,) = pick(on), pick(off)
    assert a["scratch_bytes"] == 0 and a.get("vgpr_spills", 0) == 0
    assert a["vgprs"] == b["vgprs"] <= 256
    assert a["sgprs"] == b["sgprs"] and a["sgpr_spills"] == b["sgpr_spills"]
    assert a["instructions"] == b["instructions"]
