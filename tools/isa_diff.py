#!/usr/bin/env python3
"""Compare two gfx950 device-assembly files kernel by kernel (needs no GPU):

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S glf.hip -o new.s
    python tools/isa_diff.py old.s new.s [new2.s ...]

Several new files (a translation unit split in two) are compared as their union.  Per kernel: `same` or `differs` after stripping comments, whitespace and the function index of the .LBB<n>_ /
.Lfunc_end<n> labels; for a differing kernel whether the opcode histogram and the ordered s_waitcnt / s_barrier lines
are equal; and each file's resource figures (VGPRs, VGPR / SGPR spills, scratch B per lane, LDS B, occupancy).
Exit status 1 if any kernel differs or exists in one file only.
"""
import collections
import re
import shutil
import subprocess
import sys

FIELDS = (("vgpr_count", "VGPR"), ("vgpr_spill_count", "Vspill"), ("sgpr_spill_count", "Sspill"),
          ("private_segment_fixed_size", "scratch"), ("group_segment_fixed_size", "LDS"))


def parse(path):
    """{kernel symbol: (normalised body lines, resource figures)}"""
    text = open(path).read()
    kernels = {}
    for entry in re.split(r"\n  - (?=\.)", text[text.find("amdhsa.kernels:"):])[1:]:   # the metadata's kernel records
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        kernels[name] = ([], {key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1)) for key, _ in FIELDS})
    sym = done = None
    for line in text.split("\n"):
        if sym is None:
            m = re.match(r"(\S+):", line)
            sym = m.group(1) if m and m.group(1) in kernels else None
            if done and line.startswith("; Occupancy:"):   # follows the body; the metadata does not carry it
                kernels[done][1]["occ"], done = int(line.split(":")[1]), None
        elif re.match(r"\.Lfunc_end\d+:", line):
            sym, done = None, sym
        else:
            code = re.sub(r"\.(LBB|Lfunc_end)\d+", r".\1", line.split(";")[0]).split()
            if code:
                kernels[sym][0].append(" ".join(code))
    return kernels


def figures(res):
    return " ".join("%s %d" % (label, res[key]) for key, label in FIELDS + (("occ", "occ"),))


def main(old_path, *new_paths):
    old, new = parse(old_path), {}
    for path in new_paths:   # a file split in several: the old one against their union
        new.update(parse(path))
    names = sorted(set(old) | set(new))
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    shown = subprocess.run([filt] + names, capture_output=True, text=True).stdout.split("\n") if filt else names
    bad = 0
    for name, label in zip(names, shown):
        if name not in old or name not in new:
            print("%-8s %s" % ("old only" if name in old else "new only", label))
            bad += 1
            continue
        (a, ra), (b, rb) = old[name], new[name]
        print("%-8s %s\n         %s%s" % ("same" if a == b else "differs", label, figures(ra),
                                          "" if ra == rb else "  ->  " + figures(rb)))
        if a != b:
            bad += 1
            sync = [[l for l in body if l.startswith(("s_waitcnt", "s_barrier"))] for body in (a, b)]
            hist = [collections.Counter(l.split()[0] for l in body if not l.endswith(":")) for body in (a, b)]
            moved = sum((collections.Counter(a) - collections.Counter(b)).values())
            print("         instructions %d -> %d, %d lines without a twin; opcode histogram %s; "
                  "s_waitcnt / s_barrier sequence %s (%d lines)" %
                  (sum(hist[0].values()), sum(hist[1].values()), moved, "equal" if hist[0] == hist[1] else "DIFFERS",
                   "equal" if sync[0] == sync[1] else "DIFFERS", len(sync[1])))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
