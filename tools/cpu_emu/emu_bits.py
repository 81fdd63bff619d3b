"""SHA-256 of what the emulated any-size engine computes, per case, for comparing two builds of it bit by bit:

    g++ -O1 -shared -fPIC -w -I tools/cpu_emu tools/cpu_emu/emu_spo.cpp -o /tmp/libemu_spo.so
    python tools/cpu_emu/emu_bits.py /tmp/libemu_spo.so > bits.txt

Cases: the runs of tests/test_spo_gen_host.py and the class and shape lists of tests/fft_cases.py (both directions).
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fft_cases as fc  # noqa: E402
import test_fft_engine_host as eng  # noqa: E402
import test_spo_gen_host as gen  # noqa: E402


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main(so):
    lib = ctypes.CDLL(so)
    lib.emu_fft_lines.restype = ctypes.c_int
    lib.emu_fft_lines.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_int)]
    for dims, ns, kw in gen.ND_CASES:
        nt, nout = kw.get("nt", 3), kw.get("nout", 1)
        merged, jacobi = kw.get("merged", False), kw.get("jacobi", False)
        psi, snap = gen.run_nd(lib, dims, ns, nt, nout, merged, gen.nd_inputs(dims, ns, nt, nout, jacobi))
        print("spo", dims, ns, kw, sha(psi, snap))
    for nx, nt, nout, B in [(50, 5, 2, 2), (97, 5, 2, 2), (200, 5, 2, 2), (127, 5, 2, 2), (2048, 3, 1, 1),
                            (6000, 3, 1, 1), (4106, 3, 1, 1), (5121, 3, 1, 1)]:
        _, _, _, psi, snap = gen.run_1d(lib, nx, nt, nout, B)
        print("spo1d", nx, sha(psi, snap))
    cases = [(n, 2, 3) for lengths in fc.CLASSES.values() for n in lengths] + fc.shape_cases()
    rng = np.random.default_rng(21)
    for n, o, i in cases:
        a = fc.noise(rng, (o, n, i))
        for inverse in (False, True):
            got, l2 = eng.emu_fft(lib, a, inverse)
            print("fft", (n, o, i), "inv" if inverse else "fwd", "l2", l2, sha(got))


if __name__ == "__main__":
    main(sys.argv[1])
