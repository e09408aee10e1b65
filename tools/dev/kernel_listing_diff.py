#!/usr/bin/env python3
"""development: do two device listings (hipcc ... --cuda-device-only -S) hold the same code for their kernels?

    kernel_listing_diff.py OLD.s NEW.s [NEW2.s ...]

Per mangled kernel name (the symbols an .amdhsa_kernel block names) the function body, from its label to its .Lfunc_end, is compared
after the `;` comments and the per-function numbers of the .LBB<n>_<m> labels are taken out.  The kernels of OLD.s are looked up in
the NEW files together (a source file split into several).  Prints equal / DIFFERS / missing per kernel with the line count of the
body and, where they differ, the first differing lines; exit status 1 unless every kernel of OLD.s was found equal."""
import re
import sys


def bodies(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).strip() for ln in m.group(0).split("\n")[1:-1]]
        out[name] = [ln for ln in lines if ln]
    return out


def main(old, *new):
    want, got, bad = bodies(old), {}, 0
    for p in new:
        got.update(bodies(p))
    for name, a in sorted(want.items()):
        b = got.get(name)
        if b == a:
            print("equal    %6d lines  %s" % (len(a), name))
            continue
        bad += 1
        if b is None:
            print("missing                %s" % name)
            continue
        i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print("DIFFERS  %6d / %d lines  %s\n  line %d:\n    < %s\n    > %s" % (
            len(a), len(b), name, i + 1, a[i] if i < len(a) else "(end)", b[i] if i < len(b) else "(end)"))
    return 1 if bad or not want else 0


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
