#!/usr/bin/env python3
"""Compares two device-only assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    python tools/asm_kernel_diff.py parent/compat.s branch/compat.s

For every kernel of the second file: its instructions and its .amdhsa_ resource lines must be those of the kernel of the
same name in the first file, and the kernels both files hold must stand in the same relative order.  Kernels only the
first file holds are listed (a header split is meant to drop them).  Local labels carry the function's index in its file
(.LBB12_3), so the index is masked and comments are dropped before comparing.  Exit status 1 on any difference."""
import re
import sys


def kernels(path):
    """name -> (body lines, .amdhsa_ lines), in file order."""
    lines = open(path).read().splitlines()
    out, i = {}, 0
    # ... and comments (loop notes that name such labels) dropped
    mask = lambda l: re.sub(r"\.L(BB|post_getpc)\d+", r".L\1N", l.split(";")[0].rstrip())
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        end = lines.index("\t.amdhsa_kernel " + name, i)   # the kernel descriptor follows the kernel's last instruction
        desc = lines.index("\t.end_amdhsa_kernel", end)
        body = [mask(l) for l in lines[i + 1:end] if not l.startswith("\t.section")]
        hsa = [l.strip() for l in lines[end + 1:desc]]
        assert body and hsa and all(l.startswith(".amdhsa_") for l in hsa), name
        out[name] = (body, hsa)
        i = desc
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in b:
        if name not in a:
            print(f"NEW      {name}")
            bad += 1
        elif a[name] != b[name]:
            print(f"DIFFERS  {name}")
            bad += 1
    common = [n for n in a if n in b]
    if common != [n for n in b if n in a]:
        print("ORDER    the shared kernels stand in another order")
        bad += 1
    gone = [n for n in a if n not in b]
    for n in gone:
        print(f"dropped  {n}")
    print(f"{len(a)} kernels -> {len(b)}: {len(common)} compared, {len(gone)} dropped, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
