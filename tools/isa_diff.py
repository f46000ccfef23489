#!/usr/bin/env python
"""Per-function comparison of the device code of two source trees (no GPU needed):
    tools/isa_diff.py [--flags "-D..."] OLD_TREE [NEW_TREE]
e.g. a `git worktree` of the parent commit and this tree (the default); --flags is appended to both trees' compile
lines, so measurement builds (-DPCORE_GICP_PROFILE, ...) can be compared too.
Every entry of each tree's build.SOURCES is compiled device-only with that tree's build.flags(); every function symbol
(kernels and the device functions the compiler did not inline) is printed with `same` or `differs (N lines)` and the
new tree's resource usage.  Compared are the instruction streams: `;` comments removed, basic-block label numbers
(.LBB<n>_, which count the functions of the translation unit) normalised.  Exit status 1 if anything differs."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

RES = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def tree_info(tree):
    code = "from perception_amd import build; print(build.hipcc()); print(build.CSRC); print(*build.SOURCES); print(*build.flags())"
    out = subprocess.run([sys.executable, "-c", code], cwd=tree, check=True, capture_output=True, text=True).stdout.split("\n")
    return out[0], out[1], out[2].split(), [f for f in out[3].split() if f not in ("-shared", "-fPIC")]


def functions(tree, extra=()):
    """{symbol: (instruction lines, {resource: value})} over every source of the tree"""
    hipcc, csrc, sources, flags = tree_info(tree)
    flags = flags + list(extra)
    def compile_one(src):
        with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
            r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", os.path.join(csrc, src), "-o", tmp.name,
                                                  "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
            if r.returncode:
                sys.exit(r.stderr)
            return r.stderr, open(tmp.name).read().split("\n")

    funcs = {}
    with ThreadPoolExecutor(8) as pool:
        compiled = list(pool.map(compile_one, sources))
    for remarks, asm in compiled:
        res, cur = {}, None
        for l in remarks.split("\n"):
            m = re.search(r"remark: Function Name: (\S+)", l)
            if m:
                cur = res.setdefault(m.group(1), {})
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", l)
            if m and cur is not None and m.group(1) in RES:
                cur[m.group(1)] = m.group(2)
        cur = None
        for l in asm:
            m = re.match(r"([A-Za-z_][\w.$]*):", l)
            if m and not l.startswith(".L"):
                cur = funcs.setdefault(m.group(1), ([], res.get(m.group(1), {})))[0]
            elif l.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                l = re.sub(r"\bL?BB\d+_", "BB_", l.split(";")[0]).strip()
                if l:
                    cur.append(l)
    return {k: v for k, v in funcs.items() if v[0] and v[1]}  # code with a resource remark: not data symbols


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args, extra = sys.argv[1:], []
    if "--flags" in args:
        i = args.index("--flags")
        extra = args[i + 1].split()
        del args[i:i + 2]
    old, new = functions(args[0], extra), functions(args[1] if len(args) > 1 else here, extra)
    names = sorted(n for n in set(old) | set(new) if "rocprim" not in n)  # the radix sort's kernels are the library's
    pretty, bad = demangle(names), 0
    print(f"{'function':72s} {'result':20s} " + " / ".join(RES))
    for n in names:
        if n not in old or n not in new:
            verdict = "only in " + ("old" if n in old else "new")
        elif old[n][0] == new[n][0]:
            verdict = "same"
        else:
            d = [l for l in difflib.unified_diff(old[n][0], new[n][0], n=0, lineterm="") if l[0] in "+-" and l[:3] not in ("+++", "---")]
            verdict = f"differs ({len(d)} lines)"
        bad += verdict != "same"
        r = (new.get(n) or old[n])[1]
        print(f"{re.sub(r'^void pcore::', '', pretty[n])[:72]:72s} {verdict:20s} " + " / ".join(r.get(k, "-") for k in RES))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
