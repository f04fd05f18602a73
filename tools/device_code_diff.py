#!/usr/bin/env python3
"""Device-code diff of two csrc trees: is every kernel the compiler emits the same, instruction for instruction?

    python tools/device_code_diff.py A_CSRC B_CSRC [--diag] [--jobs N] [--only FILE ...] [--rename 'PATTERN=REPLACEMENT']

Compiles every .hip file of both trees for gfx950 with the library's own flags (_lib._build) plus
``-S --cuda-device-only``, cuts the text of each kernel symbol out of the assembly, drops comments, renumbers each
kernel's own labels (``.LBBn_m``, inline-assembly labels) in order of definition, and compares kernel by kernel: the instruction text and the kernel's ``.amdhsa_*``
resource lines (registers, scratch, LDS).  It compares text only; it knows no instruction.  Needs hipcc, no GPU.

A host-side refactor must print zero differences and the same symbol set; one differing kernel means a device edit
slipped in.  ``--diag`` compiles with -DVS_WITH_DIAG; both trees then need the generated ablation includes of the
one-wave-per-SIMD attention kernel (``python tools/gen_attn_w64.py --abl 1,2,4,8,14,15,512,1024`` writes them into
the repository's csrc; copy them to an exported tree).

``--rename`` is for a change that renames kernels without touching them (a template parameter removed): tree A's mangled
kernel names are rewritten with ``re.sub(PATTERN, REPLACEMENT, name)`` wherever they occur in A's assembly, before matching.

Exit status 0: identical.  1: a difference, or a file that did not compile.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_pkg = __import__("video-summarization_amd._lib", fromlist=["_lib"])

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-fno-slp-vectorize", "-pthread"]   # _lib._build

_TOKEN = re.compile(r"[\w.$]+")


def device_asm(csrc, src, extra, out_dir):
    out = os.path.join(out_dir, src + ".s")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(csrc))), "include")
    cmd = [_pkg.hipcc_path()] + FLAGS + ["-I" + include, "-I" + csrc] + extra + ["-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s%s" % (os.path.join(csrc, src), r.stdout, r.stderr))
    with open(out) as f:
        return f.read()


def kernels(asm):
    """{kernel symbol: (instruction lines, .amdhsa_ lines)} of one device assembly file"""
    lines = asm.split("\n")
    names, hsa = [], {}
    for i, l in enumerate(lines):
        t = l.strip()
        if t.startswith(".amdhsa_kernel "):
            name = t.split()[1]
            names.append(name)
            j = i + 1
            block = []
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                block.append(" ".join(lines[j].split(";")[0].split()))
                j += 1
            hsa[name] = [b for b in block if b]
    start = {}
    for i, l in enumerate(lines):
        t = l.split(";")[0].rstrip()
        if t.endswith(":") and not t.startswith((" ", "\t", ".")):
            start[t[:-1]] = i
    out = {}
    for name in names:
        body = []
        for l in lines[start[name] + 1:]:
            t = " ".join(l.split(";")[0].split())
            if t.startswith(".Lfunc_end"):
                break
            if t:
                body.append(t)
        # the kernel's own labels (compiler block labels, and inline-asm labels whose %= number depends on the order of
        # instantiation) -> L0, L1, ... in order of definition
        labels = {}
        for t in body:
            if t.endswith(":") and " " not in t:
                labels.setdefault(t[:-1], "L%d" % len(labels))
        out[name] = ([_TOKEN.sub(lambda m: labels.get(m.group(0), m.group(0)), t) for t in body], hsa[name])
    return out


def renamed(asm, pattern, repl):
    """the assembly with every kernel symbol `name` replaced by re.sub(pattern, repl, name)"""
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        asm = asm.replace(name, re.sub(pattern, repl, name))
    return asm


def tree(csrc, extra, jobs, only, rename=None):
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and (not only or f in only))
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        asms = list(pool.map(lambda s: device_asm(csrc, s, extra, tmp), srcs))
    if rename:
        asms = [renamed(a, *rename.split("=", 1)) for a in asms]
    return {s: kernels(a) for s, a in zip(srcs, asms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a_csrc")
    ap.add_argument("b_csrc")
    ap.add_argument("--diag", action="store_true", help="compile with -DVS_WITH_DIAG")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", nargs="*", default=[], metavar="FILE", help="compare these .hip files only")
    ap.add_argument("--rename", metavar="PATTERN=REPLACEMENT", help="rewrite tree A's kernel names with this regular expression first")
    args = ap.parse_args()
    extra = ["-DVS_WITH_DIAG"] if args.diag else []
    try:
        a, b = tree(args.a_csrc, extra, args.jobs, args.only, args.rename), tree(args.b_csrc, extra, args.jobs, args.only)
    except RuntimeError as e:
        print(e)
        return 1
    print("device code, %s build: A = first tree, B = second tree" % ("-DVS_WITH_DIAG" if args.diag else "product"))
    print("%-32s %8s %8s %9s %9s %9s" % ("file", "A", "B", "only in A", "only in B", "differing"))
    total = [0, 0, 0, 0, 0]
    bad = []
    for src in sorted(set(a) | set(b)):
        ka, kb = a.get(src, {}), b.get(src, {})
        only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        diff = sorted(n for n in set(ka) & set(kb) if ka[n] != kb[n])
        row = [len(ka), len(kb), len(only_a), len(only_b), len(diff)]
        total = [t + r for t, r in zip(total, row)]
        print("%-32s %8d %8d %9d %9d %9d" % tuple([src] + row))
        bad += [(src, "only in A", n) for n in only_a] + [(src, "only in B", n) for n in only_b]
        for n in diff:
            what = "instructions" if ka[n][0] != kb[n][0] else "resources"
            bad.append((src, "differs (%s)" % what, n))
    print("%-32s %8d %8d %9d %9d %9d" % tuple(["total"] + total))
    for src, what, n in bad:
        print("  %s: %s: %s" % (src, what, n))
    print("RESULT: %s" % ("DIFFERENT" if bad else "identical: same kernel symbols, same instructions, same resources"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
