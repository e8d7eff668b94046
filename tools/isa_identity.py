#!/usr/bin/env python3
"""Is the gfx950 code of two source trees the same, symbol by symbol?

    python tools/isa_identity.py <tree_a> <tree_b>        -> stdout, exit 1 on any difference

For lfg.hip and lfg_pair_split.hip of each tree: the library's own compile
line (each tree's lfit_python_amd/_native.py: FLAGS / SPLIT_FLAGS without
-shared, no -DLFG_SRC_HASH) with --cuda-device-only -S, the assembly cut at
its symbols, and per symbol a comparison of
  * a function's instruction text, `;` comments stripped and local labels
    (.LBB<n>_<m>, .Lfunc_end<n>, .Ltmp<n>, ...) renumbered by their order of
    appearance in the function (their numbers count functions of the unit);
  * a kernel's .amdhsa_* descriptor block;
  * a data symbol's directives (its bytes), except lfg_src_hash_tag and the
    compiler's __hip_cuid_* marker, whose name is a hash of the source path.
Whole texts are compared; a verbatim move of code between files must leave
every line `identical`.  No GPU is needed.
Each tree's _native.py is executed (its module-level code, the LFG_LIB check
included) to read those flags and paths: point the tool at checkouts you trust.
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

SKIP_DATA = re.compile(r"lfg_src_hash_tag|^__hip_cuid_")
LOCAL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")


def native(tree, tag):
    spec = importlib.util.spec_from_file_location("_native_" + tag, os.path.join(tree, "lfit_python_amd", "_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_units(tree, tag, out):
    """[(unit name, assembly path, command)] of the tree's two units"""
    N = native(tree, tag)
    base = ["hipcc"] + [f for f in N.FLAGS if f != "-shared"]
    jobs = []
    for unit, src, extra in (("lfg.hip", N.SOURCES[0], []), ("lfg_pair_split.hip", N.SPLIT_SOURCE, N.SPLIT_FLAGS)):
        path = os.path.join(out, "%s_%s.s" % (tag, unit))
        jobs.append((unit, path, base + list(extra) + ["-I", N.INCLUDE, "--cuda-device-only", "-S", "-o", path, src]))
    return jobs


def strip_comment(line):
    return line.split(";", 1)[0].rstrip()


def renumber(lines):
    seen = {}

    def sub(m):
        key = m.group(0)
        if key not in seen:
            kind = m.group(1)
            seen[key] = ".L%s#%d" % (kind, sum(1 for k in seen.values() if k.startswith(".L%s#" % kind)))
        return seen[key]

    return [LOCAL.sub(sub, ln) for ln in lines]


def parse(path):
    """{(kind, symbol): [lines]} with kind in function / descriptor / data"""
    syms = {}
    kinds = {}
    cur = None   # (kind, name, lines) of the function or data symbol being read
    desc = None  # (name, lines) of a kernel descriptor (it sits inside its function's text)
    with open(path) as fh:
        for raw in fh:
            raw = raw.rstrip("\n")
            if raw.strip() == ".amdgpu_metadata":
                break
            m = re.match(r"\s*\.type\s+([^,\s]+),@(function|object)", raw)
            if m:
                kinds[m.group(1)] = m.group(2)
                continue
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", raw)
            if m:
                desc = (m.group(1), [])
                continue
            if desc:
                if raw.strip() == ".end_amdhsa_kernel":
                    syms[("descriptor", desc[0])] = desc[1]
                    desc = None
                else:
                    desc[1].append(" ".join(strip_comment(raw).split()))
                continue
            if cur and cur[0] == "function":
                if re.match(r"^\.Lfunc_end\d+:", raw):
                    syms[cur[:2]] = renumber(cur[2])
                    cur = None
                    continue
                ln = strip_comment(raw)
                # (the section switches inside a body go around the kernel descriptor)
                if ln.strip() and not re.match(r"\s*\.section\b", ln):
                    cur[2].append(" ".join(ln.split()))
                continue
            if cur and cur[0] == "data":
                if re.match(r"\s*\.size\s+%s\s*," % re.escape(cur[1]), raw):
                    cur[2].append(" ".join(strip_comment(raw).split()))
                    if not SKIP_DATA.search(cur[1]):
                        syms[cur[:2]] = cur[2]
                    cur = None
                else:
                    ln = raw if re.match(r"\s*\.(asci[iz]|string)\b", raw) else strip_comment(raw)
                    if ln.strip():
                        cur[2].append(" ".join(ln.split()))
                continue
            m = LABEL.match(raw)
            if m and m.group(1) in kinds:
                cur = ("function" if kinds[m.group(1)] == "function" else "data", m.group(1), [])
    return syms


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %s | %s" % (i + 1, x, y)
    return "line %d: %s | %s" % (min(len(a), len(b)) + 1, "<end>" if len(a) <= len(b) else a[len(b)],
                                 "<end>" if len(b) <= len(a) else b[len(a)])


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    tree_a, tree_b = os.path.abspath(argv[1]), os.path.abspath(argv[2])
    bad = 0
    with tempfile.TemporaryDirectory() as out:
        jobs = {"a": compile_units(tree_a, "a", out), "b": compile_units(tree_b, "b", out)}
        with ThreadPoolExecutor(4) as pool:
            runs = list(pool.map(lambda j: subprocess.run(j[2], stderr=subprocess.PIPE, text=True), jobs["a"] + jobs["b"]))
        for r in runs:
            if r.returncode:
                print("%s\nfailed:\n%s" % (" ".join(r.args), r.stderr))
                return 2
        for (unit, pa, _), (_, pb, _) in zip(jobs["a"], jobs["b"]):
            A, B = parse(pa), parse(pb)
            count = {"function": 0, "descriptor": 0, "data": 0}
            for key in sorted(set(A) | set(B)):
                kind, name = key
                count[kind] += 1
                if key not in A or key not in B:
                    verdict = "only in %s" % (tree_a if key in A else tree_b)
                elif A[key] == B[key]:
                    verdict = "identical"
                else:
                    verdict = "DIFFERS at " + first_difference(A[key], B[key])
                bad += verdict != "identical"
                print("%s %s %s: %s" % (unit, kind, name, verdict))
            print("%s: %d functions, %d kernel descriptors, %d data symbols compared" %
                  (unit, count["function"], count["descriptor"], count["data"]))
    print("IDENTICAL" if not bad else "%d symbols differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
