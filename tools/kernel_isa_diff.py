#!/usr/bin/env python3
"""Do two builds of a .hip file hold the same kernels?

    hipcc <the library's FLAGS + KERNEL_FLAGS (statmc_amd/build.py)> --cuda-device-only -S file.hip -o a.s     (once per build)
    tools/kernel_isa_diff.py a.s b.s

prints one line per kernel: `same` or `DIFF`, the instruction counts of both sides, the kernel's (demangled, where c++filt is
there) name; kernels that only one side has are `ONLY-A` / `ONLY-B`.  What is compared is each kernel's instruction stream in
order: comments and assembler directives dropped, local labels renumbered by first appearance, so that a kernel does not differ
because another function of the file gained a basic block.  Exit status 0 when every kernel is the same on both sides."""
import re
import subprocess
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(path):
    """{kernel symbol: [instruction or label lines]} of one device-assembly file."""
    names, bodies, cur = set(), {}, None
    with open(path, errors="replace") as f:
        for raw in f:
            line = raw.split(";", 1)[0].split("//", 1)[0].strip()
            if not line:
                continue
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
            if m:
                names.add(m.group(1))
            m = re.match(r"\.type\s+([^,\s]+),@function", line)
            if m:
                cur = bodies.setdefault(m.group(1), [])
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
            if cur is None or (line.startswith(".") and not line.endswith(":")) or re.match(r"[A-Za-z_$][\w$.]*:$", line):
                continue        # outside a function, a directive, or the function's own label
            cur.append(" ".join(line.split()))
    out = {}
    for name in names:
        seen = {}
        out[name] = [LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), l) for l in bodies.get(name, [])]
    return out


def demangled(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    a, b = kernels(argv[1]), kernels(argv[2])
    names = sorted(set(a) | set(b))
    pretty = demangled(names)
    count = lambda body: sum(1 for l in body if not l.endswith(":"))
    bad = 0
    for n in names:
        if n not in a or n not in b:
            verdict = "ONLY-A" if n in a else "ONLY-B"
        else:
            verdict = "same" if a[n] == b[n] else "DIFF"
        bad += verdict != "same"
        print("%-6s %7s %7s  %s" % (verdict, count(a[n]) if n in a else "-", count(b[n]) if n in b else "-", pretty[n]))
    print("%d kernels, %d not the same" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
