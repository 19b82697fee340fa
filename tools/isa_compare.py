"""Per-kernel comparison of two sets of gfx950 device assembly (no GPU): did a source rearrangement change the machine code?

    hipcc <build.sh's flags> --cuda-device-only -S -o before.s before.hip        (one .s per translation unit)
    python tools/isa_compare.py --before before.s [...] --after after1.s after2.s [...] [--diff-lines N]
                                [--rename PATTERN=REPLACEMENT ...] [--resources]

Every kernel symbol (`.amdhsa_kernel NAME`) of the two sets is matched by name.  --rename (repeatable) is a `re.sub` on the demangled
BEFORE names, for a kernel whose symbol changed on purpose: with it the two sides are paired by demangled name, e.g.
`--rename 'k_x<(.*)>\(=k_x<\1, true>('` pairs k_x<a> with k_x<a, true>.  A kernel's own symbol inside its body is neutralised either way.
--resources appends VGPRs, scratch bytes and LDS bytes (before->after) to the line of every kernel that differs.
Compared per kernel: the instruction text of its body and every `.amdhsa_*` directive of its descriptor (VGPRs, AGPRs via accum_offset, SGPRs, LDS bytes, scratch bytes, ...).
Ignored: comments, `.file` / `.loc` / `.cfi` lines, blank lines, and the function index in local labels (`.LBB17_3` -> `.LBB_3`:
it counts the functions of a translation unit, so it moves when kernels move between files; likewise the per-unit counter
of `.Lpost_getpcN`).  Output: one line per kernel --
demangled name, instruction count, `equal` or `DIFFERENT` -- then the symbols that exist on one side only and a unified diff of
every kernel that differs.  Exit status 1 unless the symbol sets are identical and every kernel compares equal."""
import argparse, difflib, re, shutil, subprocess, sys


def kernels(paths):
    """name -> (body lines, descriptor lines), normalised"""
    out = {}
    for path in paths:
        lines = []
        for raw in open(path):
            l = re.sub(r"\s*;.*$", "", raw.rstrip("\n")).strip()
            l = re.sub(r"\s+", " ", l)
            if not l or re.match(r"\.(file|loc|cfi_\w+|ident)\b", l):
                continue
            lines.append(re.sub(r"\.L(BB|tmp|func_begin|func_end|JTI|post_getpc)\d+", r".L\1", l))
        desc = {}
        for i, l in enumerate(lines):
            if l.startswith(".amdhsa_kernel "):
                j = lines.index(".end_amdhsa_kernel", i)
                desc[l.split()[1]] = lines[i + 1:j]
        for name, d in desc.items():
            i = lines.index(name + ":")
            j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith(".Lfunc_end"))
            if name in out:
                sys.exit(f"{name}: defined twice on one side ({path})")
            out[name] = ([l.replace(name, "<kernel>") for l in lines[i + 1:j]], d)
    return out


def demangle(names, full=False):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    if full:                                            # the whole demangled name (the mangled one where the demangler leaves it)
        return dict(zip(names, res))
    # (a c++filt that does not know _Float16's `DF16_` leaves such a name mangled: shorten it the way tools/isa_scan.py does)
    return {n: re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", r.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", ""))[:72]
            for n, r in zip(names, res)}


def renamed(K, renames):
    """key the kernels of one side by demangled name, with every (pattern, replacement) applied"""
    full = demangle(sorted(K), full=True)
    out = {}
    for n, v in K.items():
        key = full[n]
        for pat, to in renames:
            key = re.sub(pat, to, key)
        if key in out:
            sys.exit(f"{key}: two kernels of one side after --rename")
        out[key] = v
    return out


def resources(desc):
    get = lambda d: next((l.split()[1] for l in desc if l.startswith(d + " ")), "?")
    return get(".amdhsa_next_free_vgpr"), get(".amdhsa_private_segment_fixed_size"), get(".amdhsa_group_segment_fixed_size")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    ap.add_argument("--diff-lines", type=int, default=200, help="lines of unified diff shown per differing kernel")
    ap.add_argument("--rename", action="append", default=[], metavar="PATTERN=REPLACEMENT",
                    help="re.sub on the demangled before names, to pair them with the after names (repeatable)")
    ap.add_argument("--resources", action="store_true", help="VGPRs, scratch and LDS bytes of every differing kernel")
    a = ap.parse_args()
    A, B = kernels(a.before), kernels(a.after)
    if a.rename:
        A, B = renamed(A, [r.split("=", 1) for r in a.rename]), renamed(B, [])
    both = sorted(set(A) & set(B))
    nice = demangle(sorted(set(A) | set(B)))
    n_ins = lambda body: sum(1 for l in body if not l.startswith(".") and not l.endswith(":"))
    differ = [n for n in both if A[n] != B[n]]
    print(f"{'kernel':72s} {'instructions':>14s}  result")
    for n in sorted(both, key=lambda n: nice[n]):
        a_, b_ = n_ins(A[n][0]), n_ins(B[n][0])
        res = ""
        if a.resources and n in differ:
            res = "  vgpr {}->{} scratch {}->{} lds {}->{}".format(*(x for p in zip(resources(A[n][1]), resources(B[n][1])) for x in p))
        print(f"{nice[n]:72s} {(str(b_) if n not in differ else f'{a_}->{b_}'):>14s}  {'DIFFERENT' if n in differ else 'equal'}{res}")
    for side, only in (("before", sorted(set(A) - set(B))), ("after", sorted(set(B) - set(A)))):
        for n in only:
            print(f"only {side}: {nice[n]}")
    print(f"{len(both)} kernels on both sides, {len(both) - len(differ)} equal, {len(differ)} different; "
          f"{len(set(A) - set(B))} only before, {len(set(B) - set(A))} only after")
    for n in differ:
        print(f"\n--- {nice[n]}")
        d = list(difflib.unified_diff(A[n][1] + A[n][0], B[n][1] + B[n][0], "before", "after", lineterm="", n=2))
        print("\n".join(d[:a.diff_lines]))
        if len(d) > a.diff_lines:
            print(f"... {len(d) - a.diff_lines} more lines")
    sys.exit(0 if not differ and set(A) == set(B) else 1)


if __name__ == "__main__":
    main()
