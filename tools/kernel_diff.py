"""Per-kernel ISA comparison of two trees of kernel sources: every .hip of both
directories compiled to gfx950 assembly, each kernel's body with its labels
renumbered and comments / debug directives dropped, matched across the trees
by mangled name (whatever file it came from); for a kernel that differs, the
compiler's resource usage of both.  A plain text comparison; needs no GPU.
Exit status 1 if a kernel differs or is in one tree only.

usage: python tools/kernel_diff.py PARENT_CSRC [BRANCH_CSRC]
  (the parent's sources: git archive HEAD~ cppserver_amd/csrc | tar -x -C DIR)
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = re.compile(r"\s*(;|\.loc\s|\.file\s|\.cfi_)")
LABEL = re.compile(r"\.L[A-Za-z0-9_$]+")


def normalised(body):
    names = {}
    out = []
    for line in body:
        if DROP.match(line):
            continue
        line = line.split(";", 1)[0].rstrip()
        if line:
            out.append(LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line))
    return out


def kernels(csrc):
    """{mangled name: (source, normalised body, resource usage)} of every kernel of every .hip in csrc."""
    inc = os.path.join(csrc, "..", "..", "include")
    inc = inc if os.path.isdir(inc) else os.path.join(ROOT, "include")
    found = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        with tempfile.TemporaryDirectory() as d:
            s = os.path.join(d, "k.s")
            r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
                                "-S", "-I" + inc, "-I" + csrc, "-o", s, path, "-Rpass-analysis=kernel-resource-usage"],
                               check=True, capture_output=True, text=True)
            with open(s) as f:
                lines = f.read().split("\n")
        wanted = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(_ZN3wsg\S+)", x) for x in lines) if m}
        use = {}   # name -> [(field, value)] from the remarks that follow "Function Name: name"
        for field, value in re.findall(r"remark:\s+(.+?): (\S+) \[-Rpass", r.stderr):
            if field == "Function Name":
                cur = use.setdefault(value, [])
            else:
                cur.append((field, value))
        name, body = None, []
        for x in lines:
            m = re.match(r"(_ZN3wsg\w+):", x)
            if name is None and m and m.group(1) in wanted:
                name, body = m.group(1), []
            elif name is not None and re.match(r"\.Lfunc_end\d+:", x):
                found[name] = (os.path.basename(path)[:-4], normalised(body), use.get(name, []))
                name = None
            elif name is not None:
                body.append(x)
    return found


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    a = kernels(os.path.abspath(sys.argv[1]))
    b = kernels(os.path.abspath(sys.argv[2] if len(sys.argv) == 3 else os.path.join(ROOT, "cppserver_amd", "csrc")))
    dem = subprocess.run(["c++filt"], input="\n".join(sorted(set(a) | set(b))),
                         capture_output=True, text=True).stdout.split("\n")
    pretty = {k: v.split("(")[0].replace("void ", "") for k, v in zip(sorted(set(a) | set(b)), dem)}
    both = sorted(set(a) & set(b), key=pretty.get)
    same = [k for k in both if a[k][1] == b[k][1]]
    diff = [k for k in both if a[k][1] != b[k][1]]
    print("kernels parent %d branch %d\n\nIDENTICAL:" % (len(a), len(b)))
    for k in same:
        print("  %-44s %-16s -> %-16s %5d lines" % (pretty[k], a[k][0], b[k][0], len(a[k][1])))
    print("\nDIFFERENT:")
    for k in diff:
        print("  %-44s %-16s -> %-16s %5d -> %5d lines" % (pretty[k], a[k][0], b[k][0], len(a[k][1]), len(b[k][1])))
    print("\nRESOURCES of the different ones (parent -> branch):")
    for k in diff:
        print("  " + pretty[k])
        for (f, x), (_, y) in zip(a[k][2], b[k][2]):
            print("      %-28s %s -> %s%s" % (f, x, y, "" if x == y else "   <<<"))
    for side, own, other in (("PARENT", a, b), ("BRANCH", b, a)):
        print("\nONLY IN %s:" % side)
        for k in sorted(set(own) - set(other), key=pretty.get):
            print("  %-44s %-16s %5d lines" % (pretty[k], own[k][0], len(own[k][1])))
    return 1 if diff or set(a) != set(b) else 0


if __name__ == "__main__":
    sys.exit(main())
