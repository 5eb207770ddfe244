#!/usr/bin/env python3
"""Compare the instruction streams of the kernels two hipcc --save-temps .s files have in common:
   tools/isa_compare.py BEFORE.s AFTER.s
Labels are renumbered per kernel (.LBB<function>_<block> carries the function's index in the file) and comments dropped, so a kernel
that compiles to the same instructions compares equal wherever it sits in the file.  Prints the kernels only one file has, then
`same N diff M` and the names of the kernels that differ."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        if name is None:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = normalise(body)
            name = None
            continue
        body.append(line)
    return out


def normalise(body):
    labels, out = {}, []
    for line in body:
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):
            if not re.match(r"^\.LBB\d+_\d+:", t):
                continue
        for lab in re.findall(r"\.LBB\d+_\d+", t):
            labels.setdefault(lab, "L%d" % len(labels))
        out.append(re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], t))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print("kernels: %d before, %d after" % (len(a), len(b)))
    for k in only_a:
        print("only before:", k[:110])
    for k in only_b:
        print("only after: ", k[:110])
    common = sorted(set(a) & set(b))
    diff = [k for k in common if a[k] != b[k]]
    print("same %d diff %d" % (len(common) - len(diff), len(diff)))
    for k in diff:
        print("differs:", k[:110])
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
