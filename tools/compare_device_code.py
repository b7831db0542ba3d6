#!/usr/bin/env python3
"""Has a change touched the device code or the library's exported symbols?

    python tools/compare_device_code.py OTHER_TREE [--rename OLD=NEW ...] [--lib]

OTHER_TREE is a checkout of the commit to compare with (for instance `git worktree add /tmp/parent HEAD~1`).  Every
.hip source its csrc/Makefile and this tree's list in SRCS is compiled to device-only assembly with the Makefile's own
flags (-S --cuda-device-only); per function the instruction stream and per kernel the .amdhsa_* resource block are
compared, symbol names, local label numbers, comments and the order of functions in a file apart.  --rename maps a
function's (demangled) name in OTHER_TREE to its name here when a kernel was renamed on purpose.  --lib also compares
`nm -D --defined-only` of the two built libblurrily_hip.so, names only (the compiler's per-translation-unit
__hip_cuid_* markers apart: one per .hip source, whatever it holds).  Exit status 0: identical.
"""
import argparse
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_var(makefile, name):
    text = open(makefile).read().replace("\\\n", " ")
    m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, flags=re.M)
    return m.group(1).strip() if m else ""


def device_asm(csrc, src):
    mk = os.path.join(csrc, "Makefile")
    flags = make_var(mk, "FLAGS").replace("$(ARCH)", make_var(mk, "ARCH")).replace("$(EXTRA)", "")
    cmd = [make_var(mk, "HIPCC"), *flags.split(), "-S", "--cuda-device-only", "-o", "-", src]
    return subprocess.run(cmd, cwd=csrc, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def functions(asm):
    """{mangled name: normalised text} of every function and kernel descriptor block of one assembly file"""
    names = re.findall(r"^\s*\.type\s+([\w.$]+),@function", asm, flags=re.M)
    found = {}
    for name in names:
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), asm, flags=re.M | re.S)
        body = m.group(0) if m else ""
        k = re.search(r"^\s*\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % re.escape(name), asm, flags=re.M | re.S)
        text = body + "\n" + (k.group(0) if k else "")
        text = re.sub(r";.*$", "", text, flags=re.M)                       # comments
        text = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+(_\d+)?", lambda x: ".L%s%s" % (x.group(1), x.group(2) or ""), text)
        for other in names:                                               # symbol names (calls, descriptors, own label)
            text = text.replace(other, "SYM")
        found[name] = "\n".join(l.strip() for l in text.split("\n") if l.strip())
    return found


def tree_functions(root):
    csrc = os.path.join(root, "blurrily_amd", "csrc")
    srcs = [s for s in make_var(os.path.join(csrc, "Makefile"), "SRCS").split() if s.endswith(".hip")]
    found = {}
    for src in srcs:
        f = functions(device_asm(csrc, src))
        names = demangle(list(f)) if f else {}
        for mangled, text in f.items():
            found[names[mangled]] = (src, text)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--lib", action="store_true")
    args = ap.parse_args()
    rename = dict(r.split("=", 1) for r in args.rename)
    old = {rename.get(n, n): v for n, v in tree_functions(args.other).items()}
    new = tree_functions(HERE)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in new or name not in old:
            print("ONLY IN %s: %s" % ("other" if name in old else "this tree", name))
            bad += 1
        elif old[name][1] != new[name][1]:
            print("DIFFERS: %s (%s -> %s)" % (name, old[name][0], new[name][0]))
            bad += 1
    same = len(set(old) & set(new)) - sum(1 for n in set(old) & set(new) if old[n][1] != new[n][1])
    print("device code: %d functions identical, %d not" % (same, bad))
    if args.lib:
        def exported(root):
            lib = os.path.join(root, "blurrily_amd", "libblurrily_hip.so")
            out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
            return sorted(l.split()[-1] for l in out.splitlines() if l.strip() and "__hip_cuid_" not in l)
        a, b = exported(args.other), exported(HERE)
        for s in sorted(set(a) ^ set(b)):
            print("EXPORTED ONLY IN %s: %s" % ("other" if s in a else "this tree", s))
            bad += 1
        print("exported symbols: %d here, %d there, %d differ" % (len(b), len(a), len(set(a) ^ set(b))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
