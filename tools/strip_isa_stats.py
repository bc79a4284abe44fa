#!/usr/bin/env python
"""Static ISA statistics of the strip kernels (needs hipcc, no GPU).

Compiles strip translation units of nnmnkwii_amd/csrc for gfx950 with the build's own flags, device side only, to
assembly (--cuda-device-only -S) and prints per kernel: VGPRs, scalar registers, spilled scalar registers, scratch bytes
and instruction counts by class.  What it is for: a change to the strip kernel's level 1 is judged by the instructions a
wavefront executes (profiles/r06_notes.md section 3), and the register figures decide whether two workgroups still fit
a CU (<= 256 VGPRs, no scratch).

    python tools/strip_isa_stats.py                      # forward float64: general and standard-window units
    python tools/strip_isa_stats.py mlpg_strip_bwd_f32.hip mlpg_strip_std_bwd_f32.hip
    python tools/strip_isa_stats.py --json ...
    python tools/strip_isa_stats.py --digest [--csrc DIR] [UNIT ...]   # sha256 of each unit's device assembly (all units if none named)
    python tools/strip_isa_stats.py --digest-policy-blind --strip-units   # the same, blind to the cache policy of buffer loads
    python tools/strip_isa_stats.py --digest --strip-units -D MLPG_STRIP_ROW_POLICY=0

--digest is the proof that a refactor left the device code alone: run it on two trees (this one, and another tree's csrc through
--csrc) and compare the two outputs with diff.  --digest-policy-blind proves the same of a change that may only alter the cache policy
of row loads (row_load_aux in mlpg_strip_impl.h): the digest is taken after the nt / sc0 / sc1 suffix of buffer_load lines is removed.

tests/test_strip_isa_stats.py pins the standard-window forward-float64 instance against the general one with it.
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nnmnkwii_amd", "csrc")
DEFAULT = ["mlpg_strip_fwd_f64.hip", "mlpg_strip_std_fwd_f64.hip"]

_F64_ARITH = re.compile(r"^v_(add|mul|fma|fmac)_f64")
_KERNEL_ARGS = re.compile(r"strip_kernelI(.*?)EEvNS_7ProblemE")


def find_hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def _flags(src):
    sys.path.insert(0, ROOT)
    try:
        from nnmnkwii_amd.csrc import build as B
    finally:
        sys.path.pop(0)
    return [*B.FLAGS, *B.FILE_FLAGS.get(src, ["-ffp-contract=fast"]), *B.EXTRA]


def assembly(src, hipcc=None, csrc=None, extra=()):
    """The device-side assembly text of one translation unit of csrc/ (or of another tree's csrc directory); extra: more compiler
    flags, such as -DMLPG_STRIP_ROW_POLICY=0."""
    hipcc = hipcc or find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    cmd = [hipcc, "-x", "hip", *_flags(src), *extra, "--cuda-device-only", "-S", os.path.join(csrc or CSRC, src), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return r.stdout


def digest(asm):
    """sha256 of an assembly text without its __hip_cuid_ lines (a per-compilation identifier, the only part that differs between
    two runs over the same source)."""
    kept = [line for line in asm.splitlines() if "__hip_cuid_" not in line]
    return hashlib.sha256("\n".join(kept).encode()).hexdigest()


_POLICY = re.compile(r"\s+(?:nt|sc0|sc1)\b")


def policy_blind(asm):
    """The assembly text with the cache-policy suffix (nt, sc0, sc1) of every buffer_load line removed: two builds that differ only in
    the policy of their row loads (MLPG_STRIP_ROW_POLICY) give the same text.  The scope bits sc0 / sc1 go with it, so this text is
    blind to a changed scope of a buffer load too: its digest proves something only beside the plain --digest of the
    -DMLPG_STRIP_ROW_POLICY=0 build, which must equal the other tree's."""
    out = []
    for line in asm.splitlines():
        t = line.lstrip()
        if t.startswith("buffer_load_"):
            code, sep, comment = line.partition(";")
            line = _POLICY.sub("", code) + sep + comment
        out.append(line)
    return "\n".join(out)


def digests(sources, csrc=None, jobs=16, blind=False, extra=()):
    """[(unit, digest)] in the order given, compiling at most `jobs` units at a time.  blind: of the policy-blind text."""
    from concurrent.futures import ThreadPoolExecutor

    def one(src):
        asm = assembly(src, csrc=csrc, extra=extra)
        return digest(policy_blind(asm) if blind else asm)
    with ThreadPoolExecutor(max_workers=max(1, min(jobs, 16))) as ex:
        return list(zip(sources, ex.map(one, sources)))


def _classify(op):
    if op.startswith("v_readlane") or op.startswith("v_writelane"):
        return op.split("_b32")[0]
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def template_args(mangled):
    """strip_kernel's template arguments as they are mangled, e.g. ['d', 'd', 'Lb0E', 'Li0E', 'Lb0E', 'Lb1E', 'Lb0E', 'Lb1E']
    = <TIN, TOUT, BWD, VM, MULTI, NW3, TR, STD>; None for other kernels."""
    m = _KERNEL_ARGS.search(mangled)
    if not m:
        return None
    return re.findall(r"L[bi]\d+E|[df]", m.group(1) + "E")


def parse(asm):
    """{mangled kernel name: stats} for every kernel of an assembly text."""
    out = {}
    cur = None
    for line in asm.splitlines():
        t = line.strip()
        m = re.match(r"\.type\s+(\S+),@function", t)
        if m:
            cur = {"mangled": m.group(1), "instructions": 0, "valu": 0, "f64_arith": 0, "v_readlane": 0, "v_writelane": 0, "salu": 0,
                   "smem": 0, "waitcnt": 0, "lds": 0, "vmem": 0, "other": 0}
            continue
        if cur is None:
            continue
        if t.startswith(".Lfunc_end"):
            out[cur["mangled"]] = cur
            cur["_closed"] = True
            continue
        if cur.get("_closed"):
            for key, pat in (("sgprs", r"; TotalNumSgprs: (\d+)"), ("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"),
                             ("scratch_bytes", r"; ScratchSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)"),
                             ("code_bytes", r"; codeLenInByte = (\d+)")):
                mm = re.match(pat, t)
                if mm:
                    cur[key] = int(mm.group(1))
            continue
        if not t or t[0] in ".;" or t.endswith(":") or t.startswith("//"):
            continue
        op = t.split()[0]
        if not re.match(r"^[a-z][a-z0-9_]*$", op):
            continue
        cur["instructions"] += 1
        cur[_classify(op)] += 1
        if op.startswith(("v_readlane", "v_writelane")):
            cur["valu"] += 1  # lane moves of spilled scalar registers are vector instructions too
        if _F64_ARITH.match(op):
            cur["f64_arith"] += 1
    # spilled scalar registers: from the code object's metadata (one document per unit, kernels by .name)
    name = None
    for line in asm.splitlines():
        t = line.strip()
        m = re.match(r"-?\s*\.name:\s+(\S+)", t)
        if m:
            name = m.group(1)
        m = re.match(r"\.sgpr_spill_count:\s+(\d+)", t)
        if m and name in out:
            out[name]["sgpr_spills"] = int(m.group(1))
        m = re.match(r"\.vgpr_spill_count:\s+(\d+)", t)
        if m and name in out:
            out[name]["vgpr_spills"] = int(m.group(1))
    for st in out.values():
        st.pop("_closed", None)
    return out


def stats(src, hipcc=None):
    return parse(assembly(src, hipcc))


def _label(mangled):
    a = template_args(mangled)
    if a is None:
        return mangled[:60]
    names = ("TIN", "TOUT", "BWD", "VM", "MULTI", "NW3", "TR", "STD")
    val = lambda x: {"d": "f64", "f": "f32"}.get(x, x[2:-1])
    return "strip_kernel<" + ", ".join("%s=%s" % (n, val(x)) for n, x in zip(names, a)) + ">"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="*", help="translation units of nnmnkwii_amd/csrc (default: %s; --digest: all of build.SOURCES)" % " ".join(DEFAULT))
    ap.add_argument("--digest", action="store_true", help="one line 'sha256  unit' per unit: the device assembly without its __hip_cuid_ lines")
    ap.add_argument("--digest-policy-blind", action="store_true",
                    help="as --digest, of the text without the cache-policy suffix (nt, sc0, sc1) of its buffer_load lines")
    ap.add_argument("--strip-units", action="store_true", help="--digest: the mlpg_strip*.hip units of build.SOURCES instead of all")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME=VALUE", help="a macro for the compiler (repeatable)")
    ap.add_argument("--csrc", metavar="DIR", help="compile the units of this csrc directory (another tree's) with this tree's flags")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1), help="--digest: units compiled at a time (at most 16)")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    ap.add_argument("--all", action="store_true", help="every kernel of the unit, not only strip_kernel instances")
    args = ap.parse_args()
    if find_hipcc() is None:
        print("hipcc not found", file=sys.stderr)
        return 2
    csrc = os.path.abspath(args.csrc) if args.csrc else None
    extra = ["-D" + d for d in args.defines]
    if args.digest or args.digest_policy_blind:
        if not args.sources:
            _flags("")  # (imports build)
            args.sources = [s for s in sys.modules["nnmnkwii_amd.csrc.build"].SOURCES if not args.strip_units or s.startswith("mlpg_strip")]
        for src, dg in digests([os.path.basename(s) for s in args.sources], csrc, args.jobs, blind=args.digest_policy_blind, extra=extra):
            print("%s  %s" % (dg, src))
        return 0
    res = {}
    for src in args.sources or DEFAULT:
        res[src] = {k: v for k, v in parse(assembly(os.path.basename(src), csrc=csrc)).items() if args.all or template_args(k) is not None}
    if args.json:
        print(json.dumps(res, indent=1, sort_keys=True))
        return 0
    cols = ("vgprs", "sgpr_spills", "scratch_bytes", "instructions", "valu", "f64_arith", "v_readlane", "v_writelane", "salu", "smem", "waitcnt", "vmem", "lds")
    for src, ks in res.items():
        print(src)
        for k, st in ks.items():
            print("  " + _label(k))
            print("    " + "  ".join("%s=%s" % (c, st.get(c, "?")) for c in cols))
    return 0


if __name__ == "__main__":
    sys.exit(main())
