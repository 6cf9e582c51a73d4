#!/usr/bin/env python3
"""Is the device code of two source trees the same?  For every csrc/*.hip: the gfx950 assembly of both trees with the build's own
flags (__graft_entry__.FLAGS + --cuda-device-only -S), compared line for line without the per-compilation __hip_cuid_* symbol.
A file that differs is compared once more function by function (labels carry the function's index in the file, which is dropped):
"same functions, other order" means the kernels are emitted in another order and nothing else differs.

    python tools/isa_diff.py PARENT_TREE [THIS_TREE]      # one line per file; exit status 1 unless every file is one of the two
    --rename 'PATTERN=REPLACEMENT'   a regex substitution (split at the last '=') applied to the whole of PARENT_TREE's assembly before
                                     comparing, for a change that renames symbols, such as one that drops a template parameter
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import FLAGS, HIPCC  # noqa: E402


def asm(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "a.s")
        subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        return [l for l in open(out).read().splitlines() if "__hip_cuid_" not in l]


def functions(lines):
    """{symbol: text} of the functions (from a function's .section line to the next one's), of what follows the last one and of the
    per-kernel entries of the metadata"""
    text = re.sub(r"BB\d+_|\.L(?:func_begin|func_end|tmp)\d+", lambda m: re.sub(r"\d+", "", m.group(0)), "\n".join(lines))
    code, _, meta = text.partition("\n\t.amdgpu_metadata\n")
    code, _, trailer = code.partition("\n\t.section\t.AMDGPU.gpr_maximums")
    head, *funcs = re.split(r"\n(?=(?:\t\.text|\t\.section\t\.text[^\n]*)\n(?:\t\.(?:protected|globl|weak|hidden|p2align)[^\n]*\n)*\t\.type\t\S+,@function)", code)
    out = {re.search(r"\.type\s+(\S+),@function", f).group(1): f for f in funcs}
    mhead, *entries = re.split(r"\n(?=  - \.)", meta)
    out.update({"meta " + re.search(r"\.symbol:\s+(\S+)", e).group(1): e for e in entries[:-1]})
    out.update({"head": head, "trailer": trailer, "meta head": mhead, "meta tail": entries[-1] if entries else ""})
    return out


def compare(name, a_tree, b_tree, rename=None):
    a, b = (asm(os.path.join(t, "delta-prox_amd", "csrc", name)) for t in (a_tree, b_tree))
    if rename:
        a = re.sub(rename[0], rename[1], "\n".join(a)).split("\n")
    kernels = lambda ls: sorted(l.split()[1] for l in ls if l.strip().startswith(".amdhsa_kernel "))
    ka, kb = kernels(a), kernels(b)
    if a == b:
        verdict = "equal"
    elif ka == kb and functions(a) == functions(b):
        verdict = "same functions, other order"
    else:
        verdict = "DIFFERENT"
    return f"{name}: {verdict}; {len(ka)} -> {len(kb)} __global__ symbols, {'same set' if ka == kb else 'SETS DIFFER'}"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("this", nargs="?", default=ROOT)
    ap.add_argument("--rename", type=lambda v: v.rpartition("=")[::2])
    args = ap.parse_args()
    parent, this = args.parent, args.this
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(this, "delta-prox_amd", "csrc", "*.hip")))
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda n: compare(n, parent, this, args.rename), names))
    print("\n".join(res))
    sys.exit(any("DIFFER" in r for r in res))
