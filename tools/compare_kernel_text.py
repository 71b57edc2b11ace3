#!/usr/bin/env python
"""Compare the instruction streams of kernels in two builds' device assembly: a plain diff per kernel, after what does not
execute is dropped.

    hipcc <HIPCC_FLAGS of pymgrid_amd/_lib.py> --cuda-device-only -S -DMGX_EPISODE_PART=p <unit>.hip -o <dir>/<unit>_p.s
    python tools/compare_kernel_text.py OLD NEW --map OLD_NAME=NEW_NAME[,ARG...] [--map ...]

OLD / NEW: an assembly file, or a directory of ``*.s`` files (the kernels of all of them together).  Every kernel of OLD whose
demangled template name is OLD_NAME is compared with the kernel of NEW named NEW_NAME with the same template arguments and ARG...
appended (``--map rollout_policy_sample_episodes_kernel=rollout_policy_head_episodes_kernel,2``); ``true`` / ``false`` among the
old arguments and ARG may be mapped as well: ``--map 'old<..,false>=new,4'`` drops a trailing ``false`` of the old kernel first.
Of each kernel's text, comments, directives and blank lines are dropped and the block labels (``.LBB<n>_<m>``, numbered by the
function's position in its file) renumbered; what is left is compared line by line.  Prints one line per kernel: ``identical`` or
the number of differing lines; exits 1 if any differs or a kernel has no partner."""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys


def kernels_of(path):
    """{mangled name: [instruction lines]} of every function of the file / of the ``*.s`` files of the directory ``path``."""
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]:
        cur = None
        with open(f) as fh:
            for ln in fh:
                ln = ln.split(";")[0].strip()                      # (comments: `;` to the end of the line)
                m = re.match(r"^([A-Za-z_][\w$.]*):$", ln)
                if m and not m.group(1).startswith(".L"):          # a function's label
                    cur = out.setdefault(m.group(1), [])
                    continue
                if ln.startswith(".Lfunc_end"):
                    cur = None
                if cur is None or not ln or (ln.startswith(".") and not ln.startswith(".LBB")):
                    continue                                       # (directives; block labels stay)
                cur.append(ln)
    for lines in out.values():                                     # block labels: numbered in the order the kernel's text names them
        seen = {}
        lines[:] = [re.sub(r"\.LBB\d+_\d+", lambda m: ".LBB_%d" % seen.setdefault(m.group(0), len(seen)), ln) for ln in lines]
    return out


def demangled(names):
    """{mangled: 'name<args>'} (c++filt; without the parameter list, the namespace and the return type)."""
    text = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, text):
        d = re.sub(r"^void ", "", d)
        d = d[:d.index(">(") + 1] if ">(" in d else d.split("(")[0]
        out[n] = re.sub(r"^(\w+::)+", "", d.replace(" ", ""))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", required=True, metavar="OLD=NEW[,ARG...]")
    ap.add_argument("--show", type=int, default=0, help="print up to this many differing lines per kernel")
    a = ap.parse_args()
    old, new = kernels_of(a.old), kernels_of(a.new)
    old_names, new_names = demangled(list(old)), demangled(list(new))
    new_by_name = {d: n for n, d in new_names.items()}
    bad = 0
    for m in a.map:
        left, right = m.split("=")
        old_kernel, _, old_tail = left.partition("<..,")
        old_tail = old_tail.rstrip(">")
        new_kernel, *extra = right.split(",")
        found = 0
        for n, d in sorted(old_names.items(), key=lambda kv: kv[1]):
            if d.split("<")[0] != old_kernel:
                continue
            args = d[d.index("<") + 1:-1].split(",")
            if old_tail:
                if args[-1] != old_tail:
                    continue
                args = args[:-1]
            found += 1
            want = f"{new_kernel}<{','.join(args + extra)}>"
            if want not in new_by_name:
                print(f"{d} -> {want}: no such kernel")
                bad += 1
                continue
            x, y = old[n], new[new_by_name[want]]
            diff = [ln for ln in difflib.unified_diff(x, y, lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
            print(f"{d} -> {want}: " + ("identical" if not diff else f"{len(diff)} differing lines") + f" ({len(x)} / {len(y)} lines)")
            for ln in diff[:a.show]:
                print("    " + ln)
            bad += bool(diff)
        if not found:
            print(f"{left}: no such kernel in {a.old}")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
