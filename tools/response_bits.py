"""Per case, the kernel paths noted and the SHA-256 of the outputs of everything that runs on response.hip's kernels
(the fixed-t2 ensemble, the waiting-time scan, the resolvent grid, the cube, the SOS propagator, and the TDSE and
superoperator batches on its split-K GEMM), on seeded inputs at the shapes of tests/test_response_edges_gpu.py, for
comparing two library builds bit by bit:

    QDYN_LIB=/path/to/libqdyn.so python tools/response_bits.py > bits.txt     (once per build, each in its own process)
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyqed_amd import _lib  # noqa: E402
from pyqed_amd import response as rsp  # noqa: E402

dev = torch.device("cuda", 0)
_lib.ensure_device(dev)
lib = _lib.load()
st = _lib.stream_ptr(dev)
KINDS = ("uu", "ua", "au", "aa")


def t(a, dtype=complex):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def report(name, *outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for o in outs:
        h.update(o.cpu().numpy().tobytes())
    print(name, "|", _lib.take_path(), "|", h.hexdigest(), flush=True)


def grid(n, kind, t0=3.7, dt=0.5):
    g = t0 + dt * np.arange(n)
    return g if kind == "u" else g + 1e-3 * np.sin(np.arange(n))


def cn(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def lams(rng, *s):
    return -rng.uniform(0.01, 0.2, s) + 1j * rng.uniform(-2, 2, s)


def ens(tag, M, nL, n3, n1, kinds=KINDS, prunes=(False, True), dt3=0.5):
    rng = np.random.default_rng([M, nL, n3, n1])
    inp = [t(x) for x in (lams(rng, M, nL), cn(rng, M, nL), cn(rng, M, nL, nL), cn(rng, M, nL))]
    for kind in kinds:
        for prune in prunes:
            _lib.take_path()
            out = rsp.response2d_ensemble(*inp, grid(n3, kind[0], 3.7, dt3), grid(n1, kind[1], 1.3, 0.4), prune=prune)
            report("%s M %d nL %d %dx%d %s prune %d" % (tag, M, nL, n3, n1, kind, prune), out)


def ens_rect(nx, nz, trans):
    M, n3, n1 = 5, 70, 45
    rng = np.random.default_rng([nx, nz, trans])
    ops = [t(x) for x in (cn(rng, M, nx), lams(rng, M, nx), cn(rng, M, nx, nz), cn(rng, M, nz), lams(rng, M, nz))]
    t1 = grid(n1, "u" if nx <= 16 else "a", 1.3, 0.4)
    t1d = t(t1, float)
    p1 = (None, t1[0], 0.4) if nx <= 16 else (t1d.data_ptr(), 0.0, 0.0)
    out = t(cn(rng, n1, n3) if trans else cn(rng, n3, n1))
    for acc in (0, 1):                      # written over the noise, then accumulated onto the result
        _lib.take_path()
        _lib.check(lib.qd_response2d_ensemble_rect(ops[0].data_ptr(), ops[1].data_ptr(), nx, ops[2].data_ptr(),
                                                   ops[3].data_ptr(), ops[4].data_ptr(), nz, M, None, 3.7, 0.5, n3,
                                                   p1[0], p1[1], p1[2], n1, trans, out.data_ptr(), acc, st),
                   "qd_response2d_ensemble_rect")
        report("rect (%d, %d) trans %d accumulate %d" % (nx, nz, trans, acc), out)


def scan(M, nL, n3, n1, t2):
    rng = np.random.default_rng([M, nL, n3, n1, len(t2)])
    inp = [lams(rng, M, nL), cn(rng, M, nL), cn(rng, M, nL, nL), cn(rng, M, nL, nL), cn(rng, M, nL)]
    t3, t1 = grid(n3, "u"), grid(n1, "u", 1.3, 0.4)
    tag = "M %d nL %d %dx%dx%d" % (M, nL, n3, len(t2), n1)
    _lib.take_path()
    report("t2scan " + tag, rsp.response2d_t2scan(*inp, t3, np.asarray(t2), t1, prune=False))
    sc = rsp.T2Scan(*inp, t3, t1, prune=False)
    out = sc.apply(np.asarray(t2))
    report("t2 operands + apply " + tag, sc.P, sc.Q, out)
    sc.apply(np.asarray(t2), out=out, accumulate=True)
    report("t2 apply accumulate " + tag, out)


def resolvent(n, nx, ny):
    rng = np.random.default_rng([n, nx, ny])
    lam = -rng.uniform(0.05, 2, n) + 1j * rng.uniform(-4, 4, n)
    args = [t(cn(rng, n)), t(cn(rng, n, n)), t(cn(rng, n)), t(lam)]
    wx, wy = t(-4 + 8 * np.arange(nx) / max(nx - 1, 1) + 0.013, float), t(-3 + 9 * np.arange(ny) / max(ny - 1, 1), float)
    out = torch.full((nx, ny), float("nan"), dtype=torch.complex128, device=dev)
    _lib.take_path()
    _lib.check(lib.qd_resolvent_grid2d(*(x.data_ptr() for x in args), n, wx.data_ptr(), nx, wy.data_ptr(), ny,
                                       out.data_ptr(), st), "qd_resolvent_grid2d")
    report("resolvent n %d %dx%d" % (n, nx, ny), out)
    s = torch.empty(nx, dtype=torch.complex128, device=dev)
    _lib.check(lib.qd_resolvent_sum(args[0].data_ptr(), args[3].data_ptr(), n, wx.data_ptr(), nx, s.data_ptr(), st),
               "qd_resolvent_sum")
    report("resolvent_sum n %d %d" % (n, nx), s)


def cube_and_propagator(nL=3):
    rng = np.random.default_rng(nL)
    lam = lams(rng, nL)
    _lib.take_path()
    report("cube nL %d" % nL, rsp.response_cube(lam, cn(rng, nL), cn(rng, nL, nL), cn(rng, nL, nL), cn(rng, nL),
                                                grid(17, "a"), [0.0, 1.3, 25.0], grid(33, "a", 1.3, 0.4)))
    report("sos_propagator nL %d" % nL, rsp.sos_propagator(lam, cn(rng, nL, nL), cn(rng, nL, nL), grid(40, "a")))


def tdse(N, B):
    from pyqed_amd.mol import tdse_rk4
    rng = np.random.default_rng([N, B])
    psi = cn(rng, B, N)
    psi = t(psi / np.linalg.norm(psi, axis=1, keepdims=True))
    _lib.take_path()
    snap, obs = tdse_rk4(t(cn(rng, N, N) / np.sqrt(N)), psi, 0.1, 5, save_every=2, e_ops=t(cn(rng, 2, N, N)))
    report("tdse N %d B %d" % (N, B), psi, snap, obs)


def superop(N2, B):
    from pyqed_amd.oqs import superop_rk4
    rng = np.random.default_rng([N2, B])
    v = t(cn(rng, B, N2))
    _lib.take_path()
    obs, snap = superop_rk4(t(cn(rng, N2, N2) / np.sqrt(N2)), v, 0.2, 5, t(cn(rng, 3, N2)), save_every=2)
    report("superop N2 %d B %d" % (N2, B), v, snap, obs)


# the cases of tests/test_response_edges_gpu.py, in its order
for n3, n1 in ((1, 129), (15, 16), (16, 257), (17, 1), (127, 17), (128, 15), (129, 128), (257, 127), (1, 1), (257, 257)):
    for M in (1, 3):
        ens("grid", M, 9, n3, n1)
for n1 in (1024, 1025):
    ens("table", 3, 9, 17, n1, ("uu",))
for nL in (1, 15, 16, 17):
    ens("nL", 3, nL, 33, 40, ("uu", "aa"))
for M, nL in ((1, 1), (3, 5), (2, 8), (17, 1), (7, 9), (5, 13)):
    ens("K", M, nL, 20, 33, ("uu", "aa"))
for M in (1023, 1024, 3073, 33000):
    ens("groups", M, 2, 40, 100, ("uu",), (False,))
for M, kind in ((2047, "uu"), (2048, "uu"), (2051, "uu"), (2048, "au"), (2051, "au")):
    ens("switch", M, 16, 256, 256, (kind,), (kind == "au",))    # the mixed kinds go through the rectangular entry
ens("guard", 4096, 16, 4096, 16, ("uu",), (False,), dt3=0.01)
ens("guard", 4096, 16, 4096, 16, ("au",), (True,), dt3=0.01)
ens("own X launch", 17, 16, 524161, 3, ("uu",), (False,), dt3=1e-4)
for nx, nz in ((4, 2), (2, 4), (16, 1), (1, 16), (17, 3)):
    for trans in (0, 1):
        ens_rect(nx, nz, trans)
for n3 in (63, 64, 65):
    for n1 in (40, 129):
        for t2 in ([25.0], [0.0, 25.0], [0.0, 1.3, 4.0, 7.5, 25.0]):
            scan(5, 9, n3, n1, t2)
for nL, M in ((16, 15), (16, 16), (16, 17), (9, 28), (9, 29), (3, 85), (3, 86)):
    scan(M, nL, 65, 40, [0.0, 25.0])
for n, nx, ny in ((1, 33, 20), (127, 33, 20), (128, 33, 20), (129, 33, 20), (40, 1, 130), (40, 130, 1), (40, 129, 257)):
    resolvent(n, nx, ny)
cube_and_propagator()
tdse(512, 64)        # the smallest tdse_gemm shape of tests/test_tdse_tails_gpu.py
superop(64, 48)      # the smallest superop_gemm shape of tests/test_superop_tails_gpu.py
