#!/usr/bin/env python3
"""Compare two 'hipcc -S --cuda-device-only' listings of one source file per
function, by name: the functions' instruction text (with its .amdhsa_kernel
descriptor) and the kernels' amdhsa metadata.  The order of the functions in
a listing follows instantiation order and the local labels carry the
function's index or a count over the file (.LBB<i>_<n>, .Lpost_getpc<n>), so
both are left out of the comparison.
usage: listing_diff.py <before.s> <after.s>     (exit status 1: they differ)"""
import re
import sys


def functions(text):
    """name -> its text, labels renumbered"""
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\t\.size\t\1, ", text, re.M | re.S):
        body = re.sub(r"\b(L?BB|Lfunc_end|Lfunc_begin|L?JTI|Ltmp|Lpost_getpc)\d+", r"\1", m.group(2))
        out[m.group(1)] = re.sub(r"[ \t]+;", " ;", body)  # the comments' column follows the label's width
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        out[m.group(1)] += m.group(2)
    return out


def metadata(text):
    """kernel name -> its block of amdhsa.kernels"""
    blocks = re.split(r"\n  - \.", text.split("amdhsa.kernels:")[-1].split("amdhsa.target:")[0])
    out = {}
    for b in blocks:
        m = re.search(r"\.name:\s+(\S+)", b)
        if m:
            out[m.group(1)] = "\n".join(sorted(line.strip() for line in b.splitlines()))
    return out


def main():
    a, b = (open(p).read() for p in sys.argv[1:3])
    fa, fb, ma, mb = functions(a), functions(b), metadata(a), metadata(b)
    missing, added = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    text = sorted(n for n in set(fa) & set(fb) if fa[n] != fb[n])
    meta = sorted(n for n in set(ma) & set(mb) if ma[n] != mb[n])
    print(f"functions: {len(fa)} before, {len(fb)} after; kernels: {len(ma)} before, {len(mb)} after")
    print(f"missing after: {len(missing)}; added: {len(added)}; instruction text differs: {len(text)}; "
          f"metadata differs: {len(meta)}")
    for title, names in (("missing", missing), ("added", added), ("text", text), ("metadata", meta)):
        for n in names:
            print(f"  {title}: {n}")
    same = not (missing or added or text or meta) and set(ma) == set(mb)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
