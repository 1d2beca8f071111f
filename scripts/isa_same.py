#!/usr/bin/env python3
"""Do two device-assembly files hold the same kernels?  For a refactor of the host side that must not change what is compiled.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only ss_hip.hip -o X.s      (build.py's guard_isa recipe), twice
    python scripts/isa_same.py parent.s new.s

Per kernel symbol (.amdhsa_kernel NAME) two texts are compared: the instruction text between `NAME:` and its `.Lfunc_end`, and
the kernel descriptor between `.amdhsa_kernel NAME` and `.end_amdhsa_kernel` (VGPR / SGPR / LDS / scratch / spill fields and all
the rest).  Only the compiler's function counter is normalised: it numbers functions in the order the host code first names them,
so `.LBB<f>_<n>` (and `BB<f>_<n>` in loop comments) becomes `BB_<n>`, and `.Lfunc_begin<f>` / `.Lfunc_end<f>` lose their number;
block numbers within a function keep theirs.
Exit status 0: same set of symbols, same text for each.  scripts/kernel_resources.py prints the resource table of one file."""
import re
import sys


def kernels(path):
    text = open(path).read()
    text = re.sub(r"\bL?BB\d+_(\d+)", r"BB_\1", text)           # (.LBB15_248 and, in loop comments, BB15_248)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        name, desc = m.group(1), m.group(2)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end:" % re.escape(name), text, re.M | re.S)
        # ... with the symbol's .set lines (num_vgpr, numbered_sgpr, private_seg_size ...) and the "; Kernel info:" comment block
        # behind the descriptor (ScratchSize, spill counts, Occupancy, LDS bytes)
        sets = "".join(re.findall(r"^\s*\.set %s\.[^\n]*\n" % re.escape(name), text, re.M))
        info = re.compile(r"; Kernel info:\n((?:;[^\n]*\n)*)").match(text, text.index("; Kernel info:", m.end()))
        out[name] = (body.group(1) if body else None, desc + sets + info.group(1))
    return out


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    bad = 0
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print("only in %s: %s" % (b if name in kb else a, name))
            bad += 1
        elif ka[name][0] is None or ka[name] != kb[name]:
            print("differs: %s (%s)" % (name, "instructions" if ka[name][0] != kb[name][0] else "descriptor"))
            bad += 1
    lines = sum(v[0].count("\n") for v in ka.values() if v[0])
    print("%d kernels in %s, %d in %s, %d instruction-text lines compared, %d differences" % (len(ka), a, len(kb), b, lines, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
