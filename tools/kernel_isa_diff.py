#!/usr/bin/env python3
"""Compare the gfx950 machine code of two build trees kernel by kernel.

    python tools/kernel_isa_diff.py TREE_A TREE_B [file stems ...] [OLD=NEW] > report.txt

Every `hipcc ... -c csrc/X.hip` line that `make -n -B` prints in a tree is re-run there as a device-only `-S` compile, so each
file gets exactly the flags of that tree's Makefile.  The assembly is cut at the function symbols (kernels and
non-inlined device functions; a kernel's descriptor block belongs to it), comments are dropped and the numbers of local
labels -- which count the functions of a translation unit -- are normalised.  Moving a kernel to another file must leave
it `identical`.  Exit status 1 when any symbol is not.  File stems restrict the compile to those files of either tree.
OLD=NEW: a regular expression and its replacement, applied to both trees' assembly before it is cut -- for a change that
renames a type and so the parameter suffix of every mangled kernel name, and nothing else.
"""
import concurrent.futures, os, re, subprocess, sys, tempfile

LOCAL = re.compile(r"\.L(BB|JTI|func_begin|func_end|tmp)\d+")
RENAME = []                          # [(OLD, NEW)] or empty


def compile_lines(tree, stems):
    out = subprocess.run(["make", "-n", "-B", "-C", tree], capture_output=True, text=True, check=True).stdout
    for line in out.splitlines():
        words = line.split()
        if "-c" in words and words[words.index("-c") + 1].endswith(".hip"):
            src = words[words.index("-c") + 1]
            if not stems or os.path.splitext(os.path.basename(src))[0] in stems:
                yield src, words[: words.index("-c")]


def functions(tree, src, cmd):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "out.s")
        subprocess.run(cmd + ["--cuda-device-only", "-S", src, "-o", asm], cwd=tree, check=True)
        text = open(asm).read()
    for old, new in RENAME:
        text = re.sub(old, new, text)
    found = {}
    for sym in re.findall(r"^\t\.type\t(\S+),@function$", text, re.M):
        body = re.search(rf"^{re.escape(sym)}:.*?^\.Lfunc_end\d+:", text, re.M | re.S).group(0)
        desc = re.search(rf"^\t\.amdhsa_kernel {re.escape(sym)}$.*?\.end_amdhsa_kernel", text, re.M | re.S)
        lines = (body + "\n" + (desc.group(0) if desc else "")).splitlines()
        lines = [LOCAL.sub(r".L\1", l.split(";")[0]).strip() for l in lines]
        found[sym] = "\n".join(l for l in lines if l)
    return found


def tree_functions(tree, stems=()):
    jobs = list(compile_lines(tree, stems))
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        parts = pool.map(lambda job: functions(tree, *job), jobs)
        merged = {}
        for (src, _), part in zip(jobs, parts):
            for sym, code in part.items():           # a header's kernel is in every file that uses it: one entry while the code agrees
                merged[sym if merged.get(sym, code) == code else f"{sym}@{os.path.basename(src)}"] = code
    return merged


def main(a, b, *stems):
    fa, fb = tree_functions(a, stems), tree_functions(b, stems)
    verdict = {s: "only in A" if s not in fb else "only in B" if s not in fa else "identical" if fa[s] == fb[s] else "differs"
               for s in sorted(set(fa) | set(fb))}
    for sym, v in verdict.items():
        print(f"{v:10s} {sym}")
    print("summary:", ", ".join(f"{list(verdict.values()).count(v)} {v}" for v in ("identical", "differs", "only in A", "only in B")))
    return 0 if set(verdict.values()) <= {"identical"} else 1


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    RENAME += [tuple(w.split("=", 1)) for w in sys.argv[3:] if "=" in w]
    sys.exit(main(*(w for w in sys.argv[1:] if "=" not in w)))
