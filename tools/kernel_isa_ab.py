#!/usr/bin/env python3
"""Device assembly of two source trees, kernel by kernel (CPU only; for refactors that must not move a launched kernel's machine code):

    tools/kernel_isa_ab.py treeA treeB [file.hip ...] [--extra "-DFLAG ..."] [--jobs N]

compiles the named translation units of posediffusion_amd/csrc (default: every .hip of treeB's) in both trees to gfx950 assembly with the
Makefile's own command line for that file (`make -n`, so pd_ggs.hip gets its own flags), cuts the assembly into kernels -- the function
body and the .amdhsa_kernel block -- and compares them as text.  A kernel is keyed by its base name plus the template arguments that exist
in both trees: where a tree's instances have more arguments, the positions to drop (and the constant they held) are those that pair the
most instances.  Local labels are renumbered per kernel; nothing outside a kernel (__hip_cuid_*, .file, .ident, metadata) is compared.
Prints the kernels identical, differing and present in one tree only; exit status 1 if a kernel present in both trees differs."""
import argparse, itertools, os, re, shlex, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor


def assembly(tree, hip, extra, tmp):
    csrc = os.path.join(tree, "posediffusion_amd", "csrc")
    stem = os.path.splitext(os.path.basename(hip))[0]
    plan = subprocess.run(["make", "-C", csrc, "-n", "-B", f"build/{stem}.o", f"EXTRA={extra}"], capture_output=True, text=True, check=True).stdout
    cmd = next(shlex.split(l) for l in plan.splitlines() if f"-c {stem}.hip" in l)
    out = os.path.join(tmp, f"{stem}.s")
    cmd = cmd[:cmd.index("-c")] + ["--cuda-device-only", "-S", f"{stem}.hip", "-o", out]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree}: {' '.join(cmd)}\n{r.stderr[-3000:]}")
    return open(out).read()


def kernels(asm):
    """{mangled name: normalised text of the function body + its .amdhsa_kernel block}"""
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", asm, re.M):
        body = re.search(rf"^{re.escape(name)}:.*?^\.Lfunc_end\d+:", asm, re.M | re.S).group(0)
        desc = re.search(rf"^\s*\.amdhsa_kernel {re.escape(name)}$.*?\.end_amdhsa_kernel", asm, re.M | re.S).group(0)
        text, labels = (body + "\n" + desc).replace(name, "KERNEL"), {}
        out[name] = re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?|\bBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), text)
    return out


def split_name(demangled):
    m = re.match(r"(?:void )?([\w:]+?)(?:<(.*)>)?\(", demangled)
    args, depth, cur = [], 0, ""
    for ch in m.group(2) or "":
        depth += ch in "<("
        depth -= ch in ">)"
        if ch == "," and depth == 0:
            args.append(cur.strip()); cur = ""
        else:
            cur += ch
    return m.group(1), tuple(args + [cur.strip()]) if m.group(2) else ()


def keyed(ks):
    names = list(ks)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines() if names else []
    return {split_name(d): ks[n] for n, d in zip(names, dem)}


def pair(a, b):
    """keys of a -> keys of b for kernels whose template argument lists differ in length between the trees"""
    swap = {}
    for base in {k[0] for k in a} & {k[0] for k in b}:
        ta, tb = [k[1] for k in a if k[0] == base], [k[1] for k in b if k[0] == base]
        if not ta or not tb or len(ta[0]) == len(tb[0]):
            continue
        flip = len(ta[0]) < len(tb[0])
        lng, sht = (tb, ta) if flip else (ta, tb)
        best = {}
        for keep in itertools.combinations(range(len(lng[0])), len(sht[0])):
            for const in {tuple(v for i, v in enumerate(t) if i not in keep) for t in lng}:
                m = {t: tuple(t[i] for i in keep) for t in lng if tuple(v for i, v in enumerate(t) if i not in keep) == const}
                m = {t: s for t, s in m.items() if s in sht}
                if len(m) > len(best):
                    best = m
        for t, s in best.items():
            swap[(base, s) if flip else (base, t)] = (base, t) if flip else (base, s)
    return swap


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("treeA"); ap.add_argument("treeB"); ap.add_argument("files", nargs="*")
    ap.add_argument("--extra", default="", help="the Makefile's EXTRA for both trees")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    o = ap.parse_args()
    files = o.files or sorted(f for f in os.listdir(os.path.join(o.treeB, "posediffusion_amd", "csrc")) if f.endswith(".hip"))
    same, differ, only = [], [], {"A": [], "B": []}
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb, ThreadPoolExecutor(o.jobs) as pool:
        jobs = [(f, pool.submit(assembly, o.treeA, f, o.extra, ta), pool.submit(assembly, o.treeB, f, o.extra, tb)) for f in files]
        for f, ja, jb in jobs:
            a, b = keyed(kernels(ja.result())), keyed(kernels(jb.result()))
            a = {pair(a, b).get(k, k): v for k, v in a.items()}
            show = lambda k: f"{f}: {k[0]}<{', '.join(k[1])}>"
            for k in sorted(set(a) | set(b)):
                if k in a and k in b:
                    (same if a[k] == b[k] else differ).append(show(k))
                else:
                    only["A" if k in a else "B"].append(show(k))
    print(f"# {o.treeA} (A) against {o.treeB} (B), EXTRA='{o.extra}', {len(files)} translation units")
    for title, lst in ((f"identical ({len(same)})", same), (f"DIFFERING ({len(differ)})", differ),
                       (f"only in A ({len(only['A'])})", only["A"]), (f"only in B ({len(only['B'])})", only["B"])):
        print(title + ":")
        for line in lst:
            print("  " + line)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
