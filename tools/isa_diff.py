#!/usr/bin/env python3
"""Compare the device assembly of two builds, function by function.

usage: isa_diff.py DIR_A DIR_B     (each holds NAME.s made with the Makefile's flags plus --offload-device-only -S)

For every function that both sides define, the instruction text (label to .Lfunc_end) and, for a kernel, its .amdhsa_kernel descriptor
block and the compiler's resource figures must be equal after the numbers of local labels are taken out (.LBB<n>_ -- also where a loop comment names it as BB<n>_ --, .Ltmp<n>, and the per-expansion suffix of the
inline-assembly labels .Lnwi_*<n>; the padding between such a label and its comment): those number the functions and inline-assembly expansions of a translation unit, nothing else.
Prints one line per file and the functions that differ or exist on one side only; exit status 1 if a common function differs."""
import os, re, subprocess, sys

def normal(line):
    line = re.sub(r"(\.L|\b)BB\d+_", r"\1BB_", line.rstrip())      # .LBB<n>_<k>, and BB<n>_<k> in the compiler's loop comments
    line = re.sub(r"^(\.LBB_\d+:) +;", r"\1 ;", line)              # the comment's column moves with the digits taken out
    line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
    return re.sub(r"(\.Lnwi_[a-z]+)\d+", r"\1", line)


def functions(path):
    """{name: [lines]}: every function's body (label to .Lfunc_end), and for a kernel '<name> descriptor' (its .amdhsa_kernel block) and
    '<name> resources' (the comment block of register, scratch, LDS and occupancy figures the compiler prints after it)"""
    out, types = {}, set()
    name, body, desc, info = None, None, None, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            types.add(m.group(1))
        elif desc is not None:
            if re.match(r"\s*\.end_amdhsa_kernel", line):
                out[name + " descriptor"], desc = desc, None
            else:
                desc.append(normal(line))
        elif body is not None:
            if re.match(r"\.Lfunc_end\d+:", line):
                out[name], body, info = body, None, []
            elif re.match(r"\s*\.amdhsa_kernel\s", line):
                desc = []
            else:
                body.append(normal(line))
        elif re.match(r"(\S+):", line) and re.match(r"(\S+):", line).group(1) in types:
            name, body, info = re.match(r"(\S+):", line).group(1), [], None
        elif info is not None and re.match(r"; \w[\w :]*: ", line):
            info.append(line.rstrip())
            out[name + " resources"] = info
    return out


def demangle(names):
    if not names:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(n.split(" ")[0] for n in names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"idhmc::|\(idhmc::DevState.*", "", d) + n[len(n.split(" ")[0]):] for n, d in zip(names, r)]


def main(a, b):
    bad = 0
    tot = [0, 0, 0, 0]
    for f in sorted(os.listdir(a)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(b, f)):
            continue
        fa, fb = functions(os.path.join(a, f)), functions(os.path.join(b, f))
        common = [n for n in fa if n in fb]
        differ = [n for n in common if fa[n] != fb[n]]
        gone, new = [n for n in fa if n not in fb], [n for n in fb if n not in fa]
        lines = [len(fa[n]) for n in common if " " not in n]
        print("%s: %d functions, descriptors and resource blocks compared (functions of %d to %d lines), %d identical, %d differ, %d only in A, %d only in B" % (
            f, len(common), min(lines, default=0), max(lines, default=0), len(common) - len(differ), len(differ), len(gone), len(new)))
        for tag, names in (("differs", differ), ("only in A", gone), ("only in B", new)):
            for d in demangle([n for n in names if tag == "differs" or " " not in n]):     # a missing function: one line, not three
                print("    %s: %s" % (tag, d))
        bad += len(differ)
        for i, n in enumerate((len(common), len(differ), len(gone), len(new))):
            tot[i] += n
    print("total: %d compared, %d identical, %d differ, %d only in A, %d only in B" % (tot[0], tot[0] - tot[1], tot[1], tot[2], tot[3]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
