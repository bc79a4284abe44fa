"""The line filter of tools/strip_isa_stats.py --digest (no compile run): two assembly texts that differ only in their
__hip_cuid_ lines -- the identifier hipcc makes up per compilation -- must digest equal, and any other difference must show."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import strip_isa_stats as S  # noqa: E402

SNIPPET = """
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_fma_f64 v[0:1], v[2:3], v[4:5], v[0:1]
	s_endpgm
	.type	__hip_cuid_%(id)s,@object
	.globl	__hip_cuid_%(id)s
__hip_cuid_%(id)s:
	.byte	0
	.size	__hip_cuid_%(id)s, 1
	.ident	"clang"
"""


def test_digest_ignores_the_cuid_lines():
    a, b = SNIPPET % {"id": "1f2e3d4c5b6a7988"}, SNIPPET % {"id": "8899aabbccddeeff"}
    assert a != b
    assert S.digest(a) == S.digest(b)
    assert len(S.digest(a)) == 64
    assert S.digest(a) != S.digest(a.replace("v_fma_f64", "v_mul_f64"))
    assert S.digest(a) != S.digest(a.replace("\ts_endpgm\n", ""))
