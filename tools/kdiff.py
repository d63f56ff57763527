"""Kernel-by-kernel comparison of two builds' gfx950 device assembly.

    python tools/kdiff.py A B [-j N] [--show NAME]

A and B are each a directory of `hipcc -save-temps` output (its *.s files of
the device side) or a checkout, whose .hip units this script then compiles with
that checkout's Makefile flags (OBJS, HIPFLAGS, HIPCC as `make -pn` prints
them).  Kernels are matched by mangled name across all units, so a kernel that
moved to another unit is compared with itself.

Compared per kernel: the instruction text from its label to its end, and its
.amdhsa_kernel descriptor block (register counts, scratch, LDS).  Normalised
away, because only a function's place in its unit sets them: the function index
in local labels (.LBB<fn>_<bb> and the like), comments, blank lines.  Nothing
else: it is a text differ, and knows no instruction.

Prints the counts of identical, different, only-in-A and only-in-B kernels and
the names of the last three groups; exit status 1 unless every kernel is
identical.  Device functions that are not kernels (a helper the compiler did not
inline) are compared the same way and reported on a line of their own.
"""
import argparse
import concurrent.futures
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

DEV_S = "*-hip-amdgcn-amd-amdhsa-gfx*.s"


def make_vars(root):
    """OBJS, HIPFLAGS and HIPCC of root's Makefile, expanded by make itself."""
    db = subprocess.run(["make", "-pn", "-C", root, "--no-print-directory", "-q"], capture_output=True, text=True).stdout
    out = {}
    for name in ("OBJS", "HIPFLAGS", "HIPCC", "SRC"):
        m = re.search(rf"^{name} :?= (.*)$", db, re.M)
        if not m:
            sys.exit(f"kdiff: {root}/Makefile defines no {name}")
        out[name] = m.group(1).strip()
    return out


def compile_checkout(root, jobs, keep):
    root = os.path.abspath(root)
    v = make_vars(root)
    hipcc = v["HIPCC"].replace("$(ROCM)", os.environ.get("ROCM", "/opt/rocm"))
    units = []
    for o in v["OBJS"].split():
        src = os.path.join(root, v["SRC"], os.path.basename(o)[:-2] + ".hip")
        if os.path.exists(src):
            units.append(src)
    out = tempfile.mkdtemp(prefix="kdiff_", dir=keep)

    def one(src):
        obj = os.path.join(out, os.path.basename(src)[:-4] + ".o")
        cmd = [hipcc, *v["HIPFLAGS"].split(), "-save-temps=obj", "-c", src, "-o", obj]
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
        if r.returncode:
            sys.exit(f"kdiff: {' '.join(cmd)}\n{r.stderr}")

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, units))
    return out


def asm_files(path, jobs, keep):
    if os.path.exists(os.path.join(path, "Makefile")):
        path = compile_checkout(path, jobs, keep)
        print(f"kdiff: compiled into {path}", file=sys.stderr)
    files = sorted(glob.glob(os.path.join(path, "**", DEV_S), recursive=True))
    if not files:
        sys.exit(f"kdiff: no device assembly ({DEV_S}) under {path}")
    return files


LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


def norm(lines):
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip():
            continue
        out.append(LOCAL.sub(lambda m: f".L{m.group(1)}{m.group(2) or ''}", ln))
    return out


def functions(files):
    """{name: (unit, is_kernel, text lines, descriptor lines)} of every device function."""
    fns = {}
    for f in files:
        unit = os.path.basename(f).split("-hip-")[0]
        lines = open(f).read().split("\n")
        types = {m.group(1) for ln in lines if (m := re.match(r"\s*\.type\s+([^,\s]+),@function", ln))}
        body, desc = {}, {}
        cur = dcur = None  # the function / the descriptor block the line belongs to
        for ln in lines:
            if dcur is not None:  # (the assembler places a kernel's block before its .Lfunc_end)
                if re.match(r"\s*\.end_amdhsa_kernel", ln):
                    dcur = None
                else:
                    desc[dcur].append(ln)
            elif (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)):
                dcur = m.group(1)
                desc[dcur] = []
            elif cur is not None:
                if re.match(r"\.Lfunc_end\d+:", ln):
                    cur = None
                else:
                    body[cur].append(ln)
            else:
                head = ln.split(";", 1)[0].rstrip()
                if head.endswith(":") and head[:-1] in types:
                    cur = head[:-1]
                    body[cur] = []
        for name, text in body.items():
            if name in fns:
                sys.exit(f"kdiff: {name} is defined in {fns[name][0]} and in {unit}")
            fns[name] = (unit, name in desc, norm(text), norm(desc.get(name, [])))
    return fns


def report(what, a, b, names_a, names_b):
    both = [n for n in names_a if n in names_b]
    diff = [n for n in both if a[n][2:] != b[n][2:]]
    only_a = [n for n in names_a if n not in names_b]
    only_b = [n for n in names_b if n not in names_a]
    print(f"{what}: A {len(names_a)}, B {len(names_b)}: identical {len(both) - len(diff)}, "
          f"different {len(diff)}, only in A {len(only_a)}, only in B {len(only_b)}")
    for side, fns, names in (("A", a, names_a), ("B", b, names_b)):
        units = [fns[n][0] for n in names]
        print(f"  {side} by unit: " + ", ".join(f"{u} {units.count(u)}" for u in sorted(set(units))))
    for title, group in (("different", diff), ("only in A", only_a), ("only in B", only_b)):
        for n in group:
            where = f"{a[n][0]} / {b[n][0]}" if title == "different" else (a[n][0] if n in a else b[n][0])
            print(f"  {title}: {n}  [{where}]")
    return not (diff or only_a or only_b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("A")
    ap.add_argument("B")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--tmp", default=None, help="where a checkout's units are compiled (default: the system's)")
    ap.add_argument("--show", metavar="NAME", help="print the unified diff of this kernel's normalised text too")
    args = ap.parse_args()
    a = functions(asm_files(args.A, args.jobs, args.tmp))
    b = functions(asm_files(args.B, args.jobs, args.tmp))
    ok = report("kernels", a, b, [n for n in a if a[n][1]], [n for n in b if b[n][1]])
    ha, hb = [n for n in a if not a[n][1]], [n for n in b if not b[n][1]]
    if ha or hb:
        ok = report("other device functions", a, b, ha, hb) and ok
    if args.show and args.show in a and args.show in b:
        for k, part in ((2, "text"), (3, "descriptor")):
            sys.stdout.writelines(ln + "\n" for ln in difflib.unified_diff(
                a[args.show][k], b[args.show][k], f"A {part}", f"B {part}", lineterm=""))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
