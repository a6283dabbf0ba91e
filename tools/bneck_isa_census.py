"""Instruction census of the fused Bottleneck kernels (csrc/bottleneck.hip), from the compiler's gfx950 assembly.  No GPU needed.
    python tools/bneck_isa_census.py [--source FILE.hip] [--kernels SUBSTR[,SUBSTR]] [--json]
The source is compiled with the flags of the build (`_lib.device_asm`) and `-gline-tables-only`; every instruction is given
the phase of the last `.loc` line that points into the source file itself (inlined helpers of the headers take the phase of their
outermost call site).  Phases are opened in the source by comments of the form `// [census: NAME]` or `// [census: NAME xN]` (N = how often the
phase runs per tile, e.g. a rolled tap loop) and last to the next marker or to the end of the kernel; N weighs only the instructions
inside a loop of the assembly (label ... backward branch), what the compiler hoisted out of it counts once.  Classes go by mnemonic prefix:
MFMA (v_mfma), transcendental VALU (v_exp / v_rcp / v_log / v_rsq / v_sqrt / v_sin / v_cos), other VALU (v_), LDS (ds_), VMEM
(global_ / buffer_ / flat_ / scratch_), SMEM (s_load / s_buffer_load), SYNC (s_waitcnt / s_barrier / s_nop), other SALU (s_).
The instruction scheduler moves instructions across phase borders, so a phase's numbers are good to a few instructions; a kernel's
totals are exact.  `per tile` weighs every phase by its repeat count: what one wave issues for one tile when every branch is taken."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msod_amd  # noqa: E402, F401
from msod_amd import _lib  # noqa: E402
SOURCE = os.path.join(ROOT, "multispectral-object-detection_amd", "csrc", "bottleneck.hip")
CLASSES = ("MFMA", "TRANS", "VALU", "SALU", "SYNC", "LDS", "VMEM", "SMEM")
_TRANS = ("v_exp", "v_rcp", "v_log", "v_rsq", "v_sqrt", "v_sin", "v_cos")
_MARK = re.compile(r"//\s*\[census:\s*([^\]]+?)(?:\s+x(\d+))?\s*\]")


def classify(mnemonic):
    if mnemonic.startswith("v_mfma") or mnemonic.startswith("v_smfma"):
        return "MFMA"
    if mnemonic.startswith(_TRANS):
        return "TRANS"
    if mnemonic.startswith("v_"):
        return "VALU"
    if mnemonic.startswith("ds_"):
        return "LDS"
    if mnemonic.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if mnemonic.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if mnemonic.startswith(("s_waitcnt", "s_barrier", "s_nop")):
        return "SYNC"
    if mnemonic.startswith("s_"):
        return "SALU"
    return None


def compile_asm(source, extra=()):
    """The listing with line tables: the project's one compile recipe (_lib.device_asm) plus -gline-tables-only."""
    return _lib.device_asm(source, ("-gline-tables-only", "-I", os.path.dirname(SOURCE), *extra))


def source_phases(source):
    """[(first line, name, repeat)] of the markers of the source, in line order."""
    marks = []
    with open(source) as fh:
        for n, line in enumerate(fh, 1):
            m = _MARK.search(line)
            if m:
                marks.append((n, m.group(1).strip(), int(m.group(2) or 1)))
    return marks


def phase_of(marks, line):
    cur = ("(unmarked)", 1)
    for n, name, rep in marks:
        if n > line:
            break
        cur = (name, rep)
    return cur


def census(asm, source):
    """{kernel symbol: {"phases": [(name, repeat, {class: n})], "static": {class: n}, "per_tile": {class: n}, "meta": {...}}}"""
    marks = source_phases(source)
    base = os.path.basename(source)
    files = {}                       # .file number -> is it the source itself
    result, kernel, phase = {}, None, None
    for line in asm.splitlines():
        s = line.strip()
        if not s or s.startswith(";"):
            continue
        m = re.match(r"\.file\s+(\d+)\s+(.*)", s)
        if m:
            quoted = re.findall(r'"([^"]*)"', m.group(2))
            files[int(m.group(1))] = bool(quoted) and os.path.basename(quoted[-1]) == base
            continue
        m = re.match(r"(_Z\w+):", s)
        if m and not line.startswith((" ", "\t")):
            kernel = {"order": [], "counts": {}, "insts": [], "labels": {}, "loops": []}
            result[m.group(1)] = kernel
            phase = ("(unmarked)", 1)
            continue
        if s.startswith(".Lfunc_end"):
            kernel = None
            continue
        if kernel is None:
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            # a line of the source itself, or - for code inlined from a header - the outermost call site named in the comment
            lineno = int(m.group(2)) if files.get(int(m.group(1))) else 0
            sites = re.findall(re.escape(base) + r":(\d+):", s.partition(";")[2])
            if not files.get(int(m.group(1))) and sites:
                lineno = int(sites[-1])
            if lineno > 0:
                phase = phase_of(marks, lineno)
            continue
        m = re.match(r"(\.LBB\w+):", s)
        if m:
            kernel["labels"][m.group(1)] = len(kernel["insts"])
            continue
        if s.startswith(".") or s.endswith(":"):
            continue
        cls = classify(s.split()[0])
        if cls is None:
            continue
        if s.startswith("s_cbranch") or s.startswith("s_branch"):
            target = s.split()[-1]
            if target in kernel["labels"]:           # a backward branch closes a loop of the assembly
                kernel["loops"].append((kernel["labels"][target], len(kernel["insts"])))
        kernel["insts"].append((phase, cls))
    for kernel in result.values():
        # a phase's repeat count holds for the instructions inside a loop of the assembly; what the compiler hoisted out of
        # the loop (but still attributes to its lines) runs once
        for n, ((name, rep), cls) in enumerate(kernel["insts"]):
            phase = (name, rep if any(a <= n <= z for a, z in kernel["loops"]) else 1)
            if phase not in kernel["counts"]:
                kernel["order"].append(phase)
                kernel["counts"][phase] = dict.fromkeys(CLASSES, 0)
            kernel["counts"][phase][cls] += 1
    meta = _lib.kernel_notes(asm)
    out = {}
    for name, k in result.items():
        order = sorted(k["order"], key=lambda ph: (next((i for i, mk in enumerate(marks) if mk[1] == ph[0]), -1), ph[1]))
        phases = [(ph[0], ph[1], k["counts"][ph]) for ph in order]
        out[name] = {
            "phases": phases,
            "static": {c: sum(cnt[c] for _, _, cnt in phases) for c in CLASSES},
            "per_tile": {c: sum(rep * cnt[c] for _, rep, cnt in phases) for c in CLASSES},
            "meta": meta.get(name, {}),
        }
    return out


def demangled(names):
    try:
        out = subprocess.run(["c++filt"] + list(names), check=True, capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def table(name, k):
    rows = ["### `%s`" % name, "",
            "VGPRs %(vgpr_count)s, VGPR spills %(vgpr_spill_count)s, SGPR spills %(sgpr_spill_count)s, scratch %(private_segment_fixed_size)s B, static LDS %(group_segment_fixed_size)s B" % k["meta"] if k["meta"] else "",
            "", "| phase | runs | " + " | ".join(CLASSES) + " |", "|---|---|" + "---|" * len(CLASSES)]
    for ph, rep, cnt in k["phases"]:
        rows.append("| %s | %d | " % (ph, rep) + " | ".join(str(cnt[c]) for c in CLASSES) + " |")
    rows.append("| **static total** | | " + " | ".join("**%d**" % k["static"][c] for c in CLASSES) + " |")
    rows.append("| **per wave and tile** | | " + " | ".join("**%d**" % k["per_tile"][c] for c in CLASSES) + " |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default=SOURCE)
    ap.add_argument("--kernels", default="bottleneck128c_kernel,bottleneck64r_kernel", help="substrings of the demangled kernel names")
    ap.add_argument("--define", action="append", default=[], help="extra -D flags")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    res = census(compile_asm(a.source, ["-D" + d for d in a.define]), a.source)
    names = demangled(list(res))
    keep = {names[n]: k for n, k in res.items() if any(w in names[n] for w in a.kernels.split(","))}
    if a.json:
        json.dump({n: {"static": k["static"], "per_tile": k["per_tile"], "meta": k["meta"],
                       "phases": [{"phase": p, "runs": r, **c} for p, r, c in k["phases"]]} for n, k in keep.items()}, sys.stdout, indent=1)
        print()
        return
    for n in sorted(keep):
        print(table(n, keep[n]))


if __name__ == "__main__":
    main()
