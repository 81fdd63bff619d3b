#!/usr/bin/env python3
"""List the vmcnt waits the compiler put in front of an LDS read shortly behind LDS-DMA loads (needs no GPU):

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S glf_eig.hip -o eig.s
    python tools/dma_waits.py eig.s [kernel-name-substring]

The waitcnt pass orders an LDS read behind every LDS-DMA load of its own basic block that it cannot tell apart from the
read's buffer.  In a double-buffered K loop that is the other buffer's loads: the read then waits for the whole DMA it
was meant to run under (`s_waitcnt vmcnt(0)` in front of a tile's first `ds_read`).  Waits written in the source
(inline assembly) are not listed.  Prints one line per finding and exits with status 1 if there is any.
"""
import re
import sys

NEAR = 64   # instructions between the last DMA load and the wait


def main(path, want=""):
    found = 0
    kernel, since, inline = None, None, False
    lines = open(path).read().split("\n")
    for n, raw in enumerate(lines, 1):
        line = raw.split(";")[0].strip() if "#ASM" not in raw else raw.strip()
        m = re.match(r"(\S+):\s*$", line)
        if m and not m.group(1).startswith("."):
            kernel, since = m.group(1), None
        if "#ASMSTART" in raw:
            inline = True
        elif "#ASMEND" in raw:
            inline = False
        if not line or line.endswith(":") or line.startswith((".", ";")):
            continue
        if line.startswith("global_load_lds") or (line.startswith("buffer_load") and " lds" in line):
            since = 0
            continue
        if since is not None:
            since += 1
        if line.startswith("s_waitcnt") and "vmcnt" in line and not inline and since is not None and since <= NEAR:
            nxt = next((l.split(";")[0].strip() for l in lines[n:n + 8] if l.split(";")[0].strip()), "")
            if nxt.startswith("ds_read") and want in (kernel or ""):
                print("%s:%d: %s, %d instructions behind an LDS-DMA load, in front of %s" % (kernel, n, line, since, nxt))
                found += 1
    print("%d wait(s) between an LDS-DMA load and an LDS read" % found)
    return 1 if found else 0


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
