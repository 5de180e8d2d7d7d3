#!/usr/bin/env python3
"""Diff of the gfx950 code of one .hip file between two checkouts, kernel by kernel.

    tools/compare_kernel_codegen.py OLD_CHECKOUT NEW_CHECKOUT align.hip [--map 'OLD_KERNEL=NEW_KERNEL' ...] [--out FILE]

Both checkouts' csrc/Makefile is asked (make -n) for the command that compiles the file, so the flags are the build's own; the command is run
with -S on the device side only, into a temporary directory.  Kernels are named by their demangled names without the parameter list, e.g.
'vdf::align_seed_kernel<2, 14>'; a kernel whose name changed is matched through --map, every other one by its own name.  For every pair the
tool prints the instruction count, the VGPR and SGPR counts, scratch, LDS and code bytes of both builds, and then either IDENTICAL - the same
instructions in the same order once local labels are renumbered - or every opcode whose count differs, with both counts; --where adds every
differing run of instructions, registers blanked, and whether it stands in a loop.  It looks for nothing in particular: what it prints is what
differs.  No GPU is needed."""
import argparse
import collections
import difflib
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("vid_dup_finder_lib_amd", "csrc")
STATS = (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
         ("bytes", r"; codeLenInByte = (\d+)"))


def compile_command(checkout, hip_file):
    """The Makefile's own command for the file's object, turned into one that writes device assembly to stdout's stand-in `out`."""
    csrc = os.path.join(checkout, CSRC)
    obj = "_build/" + os.path.splitext(hip_file)[0] + ".o"
    lines = subprocess.check_output(["make", "-n", "-B", obj], cwd=csrc, text=True).splitlines()
    cmd = next(shlex.split(ln) for ln in lines if hip_file in shlex.split(ln) and "-c" in shlex.split(ln))
    at = cmd.index("-o")
    del cmd[at:at + 2]
    cmd[cmd.index("-c")] = "-S"
    return csrc, cmd + ["--cuda-device-only"]


def assembly(checkout, hip_file, tmp, tag):
    csrc, cmd = compile_command(checkout, hip_file)
    out = os.path.join(tmp, tag + ".s")
    subprocess.check_call(cmd + ["-o", out], cwd=csrc)
    with open(out) as f:
        return f.read(), " ".join(cmd)


def short_name(demangled):
    """'void vdf::k<A, B>(vdf::A::Args, unsigned int)' -> 'vdf::k<A, B>': the parameter list is the last balanced (...) group."""
    s = demangled.strip()
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += s[i] == ")"
            depth -= s[i] == "("
            if depth == 0:
                s = s[:i]
                break
    return s[5:] if s.startswith("void ") else s


def kernels(asm):
    """name -> {'ins': [normalised instruction lines], 'ops': Counter of opcodes, stats ...} for every kernel of the assembly."""
    symbols = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    names = subprocess.check_output(["c++filt"] + symbols, text=True).splitlines() if symbols else []
    found = {}
    for sym, name in zip(symbols, names):
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:(.*?)^; Occupancy" % re.escape(sym), asm, re.M | re.S)
        if not body:
            raise SystemExit("no body for kernel " + sym)
        text, tail = body.group(0), body.group(1)
        labels, ins = {}, []
        for ln in text.split("\n")[1:]:
            ln = ln.split(";")[0].strip()
            if ln.startswith(".Lfunc_end"):
                break
            if not ln:
                continue
            m = re.match(r"(\.L\w+):$", ln)
            if m:
                labels.setdefault(m.group(1), "L%d" % len(labels))
                ins.append(m.group(1) + ":")
            elif not ln.startswith("."):
                ins.append(re.sub(r"\s+", " ", ln))
        # local labels by order of definition, so that a kernel that moved inside the file compares equal
        ins = [re.sub(r"\.L\w+", lambda m: labels.get(m.group(0), m.group(0)), ln) for ln in ins]
        k = {"ins": ins, "ops": collections.Counter(ln.split(" ")[0] for ln in ins if not ln.endswith(":"))}
        k["n"] = sum(k["ops"].values())
        for key, pat in STATS:
            m = re.search(pat, tail)
            k[key] = int(m.group(1)) if m else -1
        found[short_name(name)] = k
    return found


def loops(ins):
    """[first, last] instruction index of every loop: a branch to a label that stands in front of it"""
    at, n, found = {}, 0, []
    for ln in ins:
        if ln.endswith(":"):
            at[ln[:-1]] = n
            continue
        target = ln.split(" ")[-1]
        if "branch" in ln.split(" ")[0] and target in at:
            found.append((at[target], n))
        n += 1
    return found


def where(a, b):
    """the runs of instructions that differ, registers blanked, with the old build's instruction indices and whether a loop of it holds them"""
    blank = lambda ins: [re.sub(r"\b[sv]\[\d+:\d+\]|\b[sv]\d+\b", "R", ln) for ln in ins if not ln.endswith(":")]
    x, y = blank(a["ins"]), blank(b["ins"])
    inside = loops(a["ins"])
    lines = ["    loops of the old build, by instruction index: " + (", ".join("%d-%d" % lp for lp in inside) or "none")]
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes():
        if tag != "equal":
            place = "in a loop" if any(lo <= i1 <= hi for lo, hi in inside) else "outside the loops"
            lines.append("    at %d (%s): %s  ->  %s" % (i1, place, " / ".join(x[i1:i2]) or "-", " / ".join(y[j1:j2]) or "-"))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("hip_file")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="a kernel whose name changed (may repeat; one OLD per NEW)")
    ap.add_argument("--where", action="store_true", help="for a kernel that differs, also every differing run of instructions and where it stands")
    ap.add_argument("--out")
    args = ap.parse_args()
    renamed = dict(m.split("=", 1) for m in args.map)
    with tempfile.TemporaryDirectory() as tmp:
        old_asm, cmd = assembly(args.old, args.hip_file, tmp, "old")
        new_asm, _ = assembly(args.new, args.hip_file, tmp, "new")
    old, new = kernels(old_asm), kernels(new_asm)
    lines = ["# %s, old -> new; compiled with: %s" % (args.hip_file, cmd)]
    matched = set()
    for name in old:
        to = renamed.get(name, name)
        if to not in new:
            lines.append("%s\n  only in old" % name)
            continue
        matched.add(to)
        a, b = old[name], new[to]
        lines.append(name if to == name else "%s\n  = %s" % (name, to))
        lines.append("  instructions %d -> %d   " % (a["n"], b["n"]) + "   ".join("%s %d -> %d" % (key, a[key], b[key]) for key, _ in STATS))
        if a["ins"] == b["ins"]:
            lines.append("  IDENTICAL")
        else:
            diff = ["%s %d -> %d" % (op, a["ops"][op], b["ops"][op]) for op in sorted(set(a["ops"]) | set(b["ops"])) if a["ops"][op] != b["ops"][op]]
            lines.append("  " + ("; ".join(diff) if diff else "same opcode counts, another order or other operands"))
            if args.where:
                lines += where(a, b)
    lines += ["%s\n  only in new" % name for name in new if name not in matched]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
