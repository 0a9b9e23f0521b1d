"""Are the kernels of two sets of gfx950 assembly files the same machine code?  kernel_code_diff.py --old A.s [..] --new B.s [..]

The files come from the build's own flags (kokorox_amd/build.py: FLAGS) plus `--offload-device-only -S`, one per translation unit:
    hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -Wall -Wno-unused-result --offload-device-only -S unit.hip -o unit.s
A kernel is compared by its instruction text, function-local labels renumbered in order of appearance and comments dropped, and
by its .amdhsa_kernel block (registers, LDS, scratch).  One line per kernel: `same`, or `DIFF` with the instruction counts and the
first line that differs.  Exit status 1 on any DIFF or any kernel that only one side has.  Equality is all it looks at.
Data sections are not compared: a __device__ constant table (taps, steps, coefficients) that a kernel reads is matched by the
symbol the code names, not by its contents, and a table that two units include is emitted in both.
"""
import argparse, re, subprocess, sys


def kernels(paths):
    out = {}
    for path in paths:
        text = open(path).read()
        desc = {m.group(1): [ln.strip() for ln in m.group(2).splitlines() if ln.strip()]
                for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S)}
        for name in desc:
            body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
            labels, code = {}, []
            for ln in body.splitlines():
                ln = ln.split(";")[0].strip()
                if ln:
                    code.append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln))
            assert name not in out, "kernel %s twice" % name
            out[name] = (code, desc[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    names = sorted(set(old) | set(new))
    pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    bad = 0
    for name, p in zip(names, pretty):
        p = re.sub(r"\(.*", "", p).replace("void kx::", "")
        if name not in old or name not in new:
            print("%-40s only in %s" % (p, "--new" if name in new else "--old"))
            bad += 1
            continue
        (c0, d0), (c1, d1) = old[name], new[name]
        if c0 == c1 and d0 == d1:
            print("%-40s same  (%d instructions and labels)" % (p, len(c0)))
            continue
        bad += 1
        x, y = (c0, c1) if c0 != c1 else (d0, d1)
        i = next((i for i, (u, v) in enumerate(zip(x, y)) if u != v), min(len(x), len(y)))
        print("%-40s DIFF  %d -> %d lines of code, first at %s line %d: `%s` -> `%s`" %
              (p, len(c0), len(c1), "code" if c0 != c1 else "descriptor", i, x[i] if i < len(x) else "<end>", y[i] if i < len(y) else "<end>"))
    print("%d kernels, %d not the same" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
