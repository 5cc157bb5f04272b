"""Which kernels does a change touch?  Compares the gfx950 assembly of two builds kernel by kernel.
    make asm                                   (in both trees: build/asm/<unit>.s, the Makefile's device flags)
    python tools/kernel_isa_diff.py DIR_A DIR_B
A kernel is its mangled name, whatever unit it is compiled in — so a kernel may move between units.  Compared per kernel: the
function body (its label to .Lfunc_end) and the .amdhsa_kernel descriptor (registers, scratch, LDS), after dropping what carries no
instruction: `;` comments, the per-unit function index in BB<n>_ / JTI<n>_ / CPI<n>_ / .Ltmp<n> labels, trailing blanks.
Prints the kernel count of each side, the names on one side only and the names whose body or descriptor differs; exit status 1 if any."""
import glob
import os
import re
import subprocess
import sys


def normalise(lines):
    out = []
    for line in lines:
        line = re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1_", line.split(";")[0])
        line = re.sub(r"\.Ltmp\d+", ".Ltmp", line).rstrip()
        if line:
            out.append(line)
    return out


def kernels(directory):
    """mangled name -> (body, descriptor), over every .s of the directory"""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        start = {m.group(1): i for i, line in enumerate(lines) for m in [re.match(r"(\S+):\s*; @\1$", line)] if m}
        at = 0
        while at < len(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[at])
            if m:
                name, first = m.group(1), at
                while not lines[at].strip().startswith(".end_amdhsa_kernel"):
                    at += 1
                body = lines[start[name]:next(i for i in range(start[name], len(lines)) if lines[i].startswith(".Lfunc_end"))]
                kernel = (normalise(body), normalise(lines[first:at + 1]))
                if found.setdefault(name, kernel) != kernel:  # (a library template two units instantiate: one and the same, or say so)
                    sys.exit("%s: kernel %s is compiled in two units, differently" % (directory, name))
            at += 1
    return found


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    lists = [("only in " + sys.argv[1], sorted(set(a) - set(b))), ("only in " + sys.argv[2], sorted(set(b) - set(a))),
             ("body differs", sorted(n for n in set(a) & set(b) if a[n][0] != b[n][0])),
             ("descriptor differs", sorted(n for n in set(a) & set(b) if a[n][1] != b[n][1]))]
    print("kernels: %d in %s, %d in %s" % (len(a), sys.argv[1], len(b), sys.argv[2]))
    for title, names in lists:
        print("%s: %d" % (title, len(names)))
        if names:
            readable = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True).stdout.split("\n")
            for raw, name in zip(names, readable):
                print("    %s    %s" % (raw, name))
    return 1 if any(names for _, names in lists) else 0


if __name__ == "__main__":
    sys.exit(main())
