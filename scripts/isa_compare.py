#!/usr/bin/env python3
"""Is the device code of every kernel the same in two builds?  The check of a refactor that must not change a kernel.

usage: isa_compare.py [--all] DIR_A DIR_B     (two directories of device assembly, one NAME.s per NAME.hip)

Such a directory comes out of the Makefile's own flags:  make -C geopurify_amd/csrc asm ASMDIR=/some/dir
(for another commit: export its geopurify_amd/ and include/ somewhere and run the same target there with `make -f` this Makefile).

For every function of every file -- each kernel (rocPRIM's included) and each non-inlined __device__ function -- it compares
  * the text from the function's label to its end,
  * for kernels the .amdhsa_kernel descriptor block and the entry in the amdhsa.kernels metadata (registers, spills, LDS, scratch),
and prints one line per function, `identical` or `differs`, then the totals.  Exit status 1 if anything differs or is missing.
The identical instantiations of rocPRIM's library kernels (some 1800: scans and sorts) are compared like the others but counted in one
line per file; one that differs gets its own line, and --all prints every one.

Ignored, because it carries no code: comment lines and trailing comments, .file / .ident / .loc / .cfi_* lines, the debug
sections (no function lives there), and the function index inside local labels (.LBB12_3 -> .LBB_3: it shifts when a function is
added to or removed from the file in front of this one).  Functions are matched by demangled name without
`(anonymous namespace)::`, and every mangled name inside the compared text is replaced the same way, so moving a kernel into the
anonymous namespace is not a difference.  Two builds of one commit, from two different directories, compare identical under
exactly these rules; outside the functions they differ only in the __hip_cuid_<hash> symbol, which is derived from the source path."""
import difflib
import hashlib
import os
import re
import shutil
import subprocess
import sys

CXXFILT = shutil.which("llvm-cxxfilt", path="/opt/rocm/lib/llvm/bin") or shutil.which("c++filt") or "c++filt"
DROP = re.compile(r"\s*(;|\.file\b|\.ident\b|\.loc\b|\.cfi_)")
LABEL_NO = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+")


def demangle_all(txt):
    """mangled name -> demangled name without the anonymous namespace, for every _Z... token of the text"""
    names = sorted(set(re.findall(r"\b_Z\w+", txt)))
    # (an older c++filt does not know DF16_ = _Float16; Dh = half is a builtin code too, so the substitution indices stay)
    ask = "\n".join(n.replace("DF16_", "Dh") for n in names)
    out = subprocess.run([CXXFILT], input=ask, capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"\bhalf\b", "_Float16", d.replace("(anonymous namespace)::", "")) for n, d in zip(names, out)}


def short(name):
    """rocPRIM's template names run to kilobytes: the head of the name and a digest of all of it"""
    return name if len(name) <= 160 else f"{name[:140]}...#{hashlib.sha1(name.encode()).hexdigest()[:10]}"


def clean(lines, names):
    res = []
    for ln in lines:
        if DROP.match(ln) or not ln.strip():
            continue
        ln = ln.split(" ; ")[0].rstrip()                    # trailing comment of an instruction line
        ln = LABEL_NO.sub(lambda m: ".L" + m.group(1), ln)
        ln = re.sub(r"\b_Z\w+", lambda m: names.get(m.group(0), m.group(0)), ln)
        res.append(" ".join(ln.split()))
    return res


def parse(path):
    """{function name: {"text": [...], "desc": [...], "meta": [...]}} of one assembly file"""
    txt = open(path).read()
    names = demangle_all(txt)
    lines = txt.split("\n")
    funcs = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if m:
            sym = m.group(1)
            start = next(j for j in range(i, len(lines)) if lines[j].startswith(sym + ":"))
            # (a kernel's descriptor sits in .rodata between its last instruction and .Lfunc_end)
            end = next(j for j in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:|\s*\.section\b", lines[j]))
            funcs[names.get(sym, sym)] = {"text": clean(lines[start:end], names), "desc": [], "meta": []}
            i = end
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
            funcs[names.get(m.group(1), m.group(1))]["desc"] = clean(lines[i:end], names)
            i = end
        i += 1
    if "amdhsa.kernels:" in txt:
        meta = txt[txt.index("amdhsa.kernels:"):txt.index("amdhsa.target:")]
        for blk in re.split(r"\n  - ", meta)[1:]:
            sym = re.search(r"\.name:\s+(\S+)", blk).group(1)
            funcs[names.get(sym, sym)]["meta"] = clean(blk.split("\n"), names)
    return funcs


def main():
    show_all = "--all" in sys.argv[1:]
    da, db = [a for a in sys.argv[1:] if a != "--all"]
    files = sorted(set(f for d in (da, db) for f in os.listdir(d) if f.endswith(".s")))
    same = differs = 0
    diffs = []
    for f in files:
        pa, pb = os.path.join(da, f), os.path.join(db, f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{f}: only in {da if os.path.exists(pa) else db}: differs")
            differs += 1
            continue
        fa, fb = parse(pa), parse(pb)
        lib_same = 0
        for name in sorted(set(fa) | set(fb)):
            a, b = fa.get(name), fb.get(name)
            kind = "kernel" if (a or b)["desc"] else "device function"
            if a == b:
                same += 1
                if "rocprim" in name and not show_all:
                    lib_same += 1
                else:
                    print(f"{f}: {kind} {short(name)}: identical ({len(a['text'])} lines)")
                continue
            differs += 1
            if a is None or b is None:
                print(f"{f}: {kind} {short(name)}: differs (only in {da if a else db})")
                continue
            parts = [k for k in ("text", "desc", "meta") if a[k] != b[k]]
            print(f"{f}: {kind} {short(name)}: differs ({', '.join(parts)})")
            for k in parts:
                diffs += list(difflib.unified_diff(a[k], b[k], f"{pa} {name} {k}", f"{pb} {name} {k}", lineterm="", n=2))
        if lib_same:
            print(f"{f}: {lib_same} rocPRIM library kernels: identical")
    print(f"total: {same + differs} functions in {len(files)} files, {same} identical, {differs} differ")
    if diffs:
        sys.stderr.write("\n".join(diffs[:400]) + "\n")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
