#!/usr/bin/env python3
"""Per-kernel comparison of two `make asm` outputs (hkv_kernels.s of two builds).

Instructions only: directives, labels and comment lines are set aside, and
label numbers in branch operands are blanked, so a renumbered block alone is
no difference. Every differing instruction of the first file (or, for pure
insertions, the instruction they precede) is placed in that file's loop tree,
read from the compiler's own block comments as tools/isa_census.py reads them.

  python tools/asm_kernel_diff.py parent.s this.s            # summary per kernel
  python tools/asm_kernel_diff.py parent.s this.s --lines    # ... with the differing lines
  python tools/asm_kernel_diff.py parent.s this.s --kernel yverdict --lines
"""
import argparse
import collections
import difflib
import re
import sys


def kernel_lines(path):
    """{mangled kernel name: its raw lines up to .Lfunc_end}"""
    out, name, body = {}, None, []
    for raw in open(path):
        line = raw.rstrip("\n")
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        body.append(line)
    return out


def instructions(lines):
    """[(instruction with label numbers blanked, loop header or None, depth)]"""
    res, loop, depth = [], None, 0
    for line in lines:
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):?(.*)$", line)
        if m:
            rest = m.group(2)
            loop, depth = None, 0
            header = re.search(r"Loop Header: Depth=(\d+)", rest)
            inside = re.search(r"in Loop: Header=(\w+) Depth=(\d+)", rest)
            if header:
                loop, depth = m.group(1).lstrip(".L"), int(header.group(1))
            elif inside:
                loop, depth = inside.group(1), int(inside.group(2))
            continue
        header = re.match(r"^\s*;\s*=>\s*This (Inner )?Loop Header: Depth=(\d+)", line)
        if header:
            loop, depth = loop or "header", int(header.group(2))
            continue
        text = line.split(";")[0].strip()
        if not text or text.startswith(".") or re.match(r"^\w+:$", text):
            continue
        res.append((re.sub(r"\.LBB\d+_\d+", "L", text), loop, depth))
    return res


def where(entry):
    return "outside every loop" if entry[1] is None else "in loop %s depth %d" % (entry[1], entry[2])


def compare(name, a, b, show_lines):
    """Prints the kernel's differences; returns True if it is identical."""
    xs, ys = [t[0] for t in a], [t[0] for t in b]
    if xs == ys:
        return True
    per_loop = collections.Counter()
    differing = 0
    shown = []
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, xs, ys, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        differing += max(i2 - i1, j2 - j1)
        if i2 > i1:  # each replaced or removed instruction counts where it sits
            for i in range(i1, i2):
                per_loop[where(a[i])] += 1
            extra = (j2 - j1) - (i2 - i1)
            if extra > 0:
                per_loop[where(a[i2 - 1])] += extra
        else:  # insertions count where the instruction they precede sits
            per_loop[where(a[min(i1, len(a) - 1)])] += j2 - j1
        if show_lines:
            shown.append("  @ %d (%s)" % (i1, where(a[min(i1, len(a) - 1)])))
            shown += ["  - " + t for t in xs[i1:i2]] + ["  + " + t for t in ys[j1:j2]]
    print("%s: %d / %d instructions, %d differing" % (name, len(xs), len(ys), differing))
    for place, n in sorted(per_loop.items(), key=lambda t: -t[1]):
        print("    %5d  %s" % (n, place))
    for line in shown:
        print(line)
    return False


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("first", help="hkv_kernels.s of the reference build (its loop tree places the differences)")
    ap.add_argument("second", help="hkv_kernels.s of the build under test")
    ap.add_argument("--kernel", default="", help="only kernels whose mangled name contains this")
    ap.add_argument("--lines", action="store_true", help="print the differing instructions")
    args = ap.parse_args()
    a, b = kernel_lines(args.first), kernel_lines(args.second)
    same = total = 0
    for name in a:
        if args.kernel not in name:
            continue
        total += 1
        if name not in b:
            print("%s: only in %s" % (name, args.first))
            continue
        same += compare(name, instructions(a[name]), instructions(b[name]), args.lines)
    for name in b:
        if args.kernel in name and name not in a:
            total += 1
            print("%s: only in %s" % (name, args.second))
    print("identical: %d of %d" % (same, total))
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())
