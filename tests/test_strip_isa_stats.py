"""Static checks on the strip kernel's standard-window instantiation (tools/strip_isa_stats.py; needs hipcc, no GPU).

The forward float64 instance compiled for the standard windows must stay launchable two workgroups per CU and must really
have lost the arithmetic of the zero coefficients: 11 of 27 multiply-adds per frame, 18 frames per chunk, two copies of
level 1 (interior and edge chunks) in the kernel."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import strip_isa_stats as S  # noqa: E402

pytestmark = pytest.mark.skipif(S.find_hipcc() is None, reason="hipcc not found")

# <TIN, TOUT, BWD, VM (0: per-frame variances), MULTI, NW3, TR, STD>
GENERAL = ["d", "d", "Lb0E", "Li0E", "Lb0E", "Lb1E", "Lb0E", "Lb0E"]
STD = ["d", "d", "Lb0E", "Li0E", "Lb0E", "Lb1E", "Lb0E", "Lb1E"]


def _pick(stats, args):
    hits = [st for name, st in stats.items() if S.template_args(name) == args]
    assert len(hits) == 1, (args, sorted(stats))
    return hits[0]


@pytest.fixture(scope="module")
def pair():
    gen = _pick(S.stats("mlpg_strip_fwd_f64.hip"), GENERAL)
    std = _pick(S.stats("mlpg_strip_std_fwd_f64.hip"), STD)
    print("general:", gen)
    print("std:    ", std)
    return gen, std


def test_parser_on_a_snippet():
    asm = """
	.type	_ZN4mlpg5strip12strip_kernelIddLb0ELi0ELb0ELb1ELb0ELb1EEEvNS_7ProblemENS_6WinSetENS0_4ArgsE,@function
_ZN4mlpg5strip12strip_kernelIddLb0ELi0ELb0ELb1ELb0ELb1EEEvNS_7ProblemENS_6WinSetENS0_4ArgsE:
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
	v_fma_f64 v[0:1], v[2:3], v[4:5], v[0:1]
	v_add_f64 v[0:1], v[0:1], v[2:3]
	v_readlane_b32 s2, v9, 3
	buffer_load_dwordx2 v[0:1], v2, s[8:11], s3 offen
	s_endpgm
.Lfunc_end0:
; codeLenInByte = 44
; TotalNumSgprs: 12
; NumVgprs: 10
; ScratchSize: 0
  - .name:           _ZN4mlpg5strip12strip_kernelIddLb0ELi0ELb0ELb1ELb0ELb1EEEvNS_7ProblemENS_6WinSetENS0_4ArgsE
    .sgpr_spill_count: 5
"""
    st = S.parse(asm)
    assert len(st) == 1
    (name, k), = st.items()
    assert S.template_args(name) == STD
    assert (k["instructions"], k["valu"], k["f64_arith"], k["v_readlane"], k["smem"], k["waitcnt"], k["vmem"], k["salu"]) == (7, 3, 2, 1, 1, 1, 1, 1)
    assert (k["vgprs"], k["scratch_bytes"], k["sgpr_spills"]) == (10, 0, 5)


def test_std_instance_has_no_scratch(pair):
    gen, std = pair
    assert std["scratch_bytes"] == 0 and std.get("vgpr_spills", 0) == 0


def test_std_instance_needs_no_more_vgprs(pair):
    gen, std = pair
    assert std["vgprs"] <= gen["vgprs"] <= 256  # two workgroups of four wavefronts per CU: 512 / 2 registers per lane


def test_std_instance_spills_fewer_scalar_registers(pair):
    gen, std = pair
    assert std["sgpr_spills"] < gen["sgpr_spills"]


def test_std_instance_lost_the_zero_terms(pair):
    gen, std = pair
    assert gen["f64_arith"] - std["f64_arith"] >= 11 * 18 * 2


def test_std_instance_fetches_no_coefficient(pair):
    """No scalar load placed by karg_f64x9 (three per copy of level 1 in the general instance, two instructions each)."""
    gen, std = pair
    assert std["smem"] <= gen["smem"] - 6
