"""SPO / SPO2 / SPO3 with white-noise wavepackets.  The smooth-input tests propagate a Gaussian, whose spectrum is
about 0 over most bins: a transform fault that touches only high k changes nothing at their 1e-10.  White noise keeps
every bin alive (the point and kinetic operators are unit-modulus), and the bound sits at the rounding error of the
fp64 passes: nsteps (2 D + 1) tol(max dim) relative L2 (tests/fft_cases.py; a D-dimensional Strang step is D forward
and D inverse transforms and the point operators), against the oracle restatements run with the solver's own
operators.  Each test prints the worst err / bound it measured."""
import numpy as np
import pytest

import fft_cases as fc
from conftest import relerr, took
from spo_models import spo2_model_rect

pytestmark = pytest.mark.gpu
NT, NOUT, DT = 4, 2, 0.05


def white(shape, seed):
    psi = fc.noise(np.random.default_rng(seed), shape)
    return psi / np.linalg.norm(psi)


def bound(dims, nsteps=NT):
    return nsteps * (2 * len(dims) + 1) * fc.tol(max(dims))


def check(name, pairs, dims):
    """pairs: (computed, reference) states; each within the bound on its own (a NaN ratio fails fc.within)."""
    rs = [relerr(a, b) / bound(dims) for a, b in pairs]
    assert rs and fc.within(*rs), (name, rs)
    print(f"spo white noise {name}: worst err/bound {max(rs):.4f}")


# ---------------------------------------------------------------- SPO (1D)
def run_spo1d(n, paths):
    from oracle import spo as osp
    from pyqed_amd import SPO
    x = np.linspace(-8, 8, n)
    psi0 = white((3, n), 100 + n)
    sol = SPO(x, mass=1.0)
    sol.set_potential(lambda q: q ** 2 / 2)
    took("")
    r = sol.run(psi0, dt=0.01, nt=NT, nout=NOUT)
    got = took("")[1]
    for p in paths:
        assert p in got, (p, got)
    assert len(r.psilist) == NT // NOUT - 1
    pairs = []
    for b in range(3):
        pl, fin = osp.spo1d_run(x, x ** 2 / 2, psi0[b], 0.01, NT, NOUT)
        pairs += [(r.psi[b], fin)] + [(r.psilist[k][b], pl[k]) for k in range(len(pl))]
    check(f"SPO n={n}", pairs, (n,))


@pytest.mark.parametrize("n", [16, 32, 64, 128, 512, 1024])
def test_spo1d_pow2_kernel(n):
    run_spo1d(n, ("spo1d_pow2",))


@pytest.mark.parametrize("n,plan", [(61, "spo1d_mixed"), (509, "spo1d_bluestein"), (2557, "spo1d_bluestein"),
                                    (5121, "spo1d_direct"), (5125, "spo1d_fourstep")])
def test_spo1d_any_size_plans(n, plan):
    """61: one generic prime stage; 509 and 2557: chirp-z with M = 1024 and 5120; 5121 = 9 569 has no split into two
    mixed-radix factors, so the 1D run takes the direct DFT; 5125 = 41 125 has one (four-step, with the kinetic factor
    applied in the permuted k order)."""
    run_spo1d(n, ("spo_any", plan))


# ---------------------------------------------------------------- SPO2
def spo2_path(nx, ny, ns):
    """qd_spo2_run_ex's dispatch rule (spo_plan.hpp): the power-of-two kernels take 16 <= L <= 1024, ns <= 8 with
    ns (ny / 4) <= 256 and ns (nx / 4) <= 256 and both passes within the LDS."""
    p2 = lambda n: 16 <= n <= 1024 and n & (n - 1) == 0
    lds = max((ny + 2 * ns * ny) * 16, (nx + 4 * ns * nx) * 16)
    special = p2(nx) and p2(ny) and ns <= 8 and ns * (ny // 4) <= 256 and ns * (nx // 4) <= 256 and lds <= 160 * 1024
    return "spo2_pow2" if special else "spo_any"


def spo2_solver(nx, ny, ns, jacobi=False):
    from pyqed_amd import SPO2
    x, y, surfaces, couplings, _ = spo2_model_rect(nx, ny, ns)
    if jacobi:
        sol = SPO2(x, y, mass=[1.0, lambda q: 1.5 + 0.2 * q ** 2], nstates=ns, coords='jacobi')
    else:
        sol = SPO2(x, y, mass=[1.0, 1.3], nstates=ns)
    sol.set_DPES(surfaces, couplings)
    return sol


def run_spo2_strang(nx, ny, ns, path, jacobi=False):
    from oracle import spo as osp
    sol = spo2_solver(nx, ny, ns, jacobi)
    psi0 = white((nx, ny, ns), 200 + nx + ny)
    took("")
    r = sol.run(psi0, dt=DT, nt=NT, nout=NOUT)
    got = took("")[1]
    assert path in got and spo2_path(nx, ny, ns) == path, (path, got)
    keo = osp.keo_jacobi(sol.exp_Kx, sol.exp_Ky) if jacobi else osp.keo_linear(sol.exp_K)
    pl, fin = osp.spo2_strang_run(sol.exp_V_half, keo, psi0, NT, NOUT)
    assert len(r.psilist) == len(pl) == NT // NOUT + 1
    check(f"SPO2 {nx}x{ny}x{ns}{' jacobi' if jacobi else ''}",
          [(r.psi, fin)] + [(r.psilist[k], pl[k]) for k in range(1, len(pl))], (nx, ny))


@pytest.mark.parametrize("nx,ny,ns,path", [(16, 16, 2, "spo2_pow2"), (16, 1024, 1, "spo2_pow2"),
                                           (1024, 16, 1, "spo2_pow2"), (512, 32, 2, "spo2_pow2"),
                                           (32, 512, 2, "spo2_pow2"), (128, 16, 3, "spo2_pow2"),
                                           (256, 64, 3, "spo2_pow2"),
                                           (16, 1024, 2, "spo_any"), (512, 16, 3, "spo_any")])
def test_spo2_pow2_kernel_rectangular_and_boundary(nx, ny, ns, path):
    """Rectangular power-of-two grids on the specialised kernel up to its ns (n / 4) <= 256 limit, and the any-size
    engine just across it."""
    run_spo2_strang(nx, ny, ns, path)


@pytest.mark.parametrize("nx,ny,ns", [(67, 45, 3), (601, 12, 2), (12, 601, 1), (134, 61, 2)])
def test_spo2_any_size_grids(nx, ny, ns):
    run_spo2_strang(nx, ny, ns, "spo_any")


@pytest.mark.parametrize("nx,ny,ns", [(67, 45, 3), (601, 12, 2), (12, 601, 1), (134, 61, 2)])
def test_spo2_any_size_grids_merged(nx, ny, ns):
    """return_states=False: the merged V structure, NT + 1 kinetic steps."""
    from oracle import spo as osp
    sol = spo2_solver(nx, ny, ns)
    psi0 = white((nx, ny, ns), 300 + nx + ny)
    took("")
    r = sol.run(psi0, dt=DT, nt=NT, nout=NOUT, return_states=False)
    assert took("spo_any")[0]
    _, fin = osp.spo2_merged_run(sol.exp_V, sol.exp_V_half, osp.keo_linear(sol.exp_K), psi0, NT, NOUT)
    check(f"SPO2 merged {nx}x{ny}x{ns}", [(r.psi, fin)], (nx, ny))


def test_spo2_jacobi_any_size_grid():
    run_spo2_strang(97, 13, 2, "spo_any", jacobi=True)


# ---------------------------------------------------------------- SPO3
# (nx, ny, nz[, ns = 2]) and the paths the run must note.  Beyond the first two: for every pass family and tile width
# the SPO3 plans reach (the set in test_spo_plan_host.py), the smallest grid that takes it.
SPO3_CASES = [((16, 64, 32), "spo3_pow2"), ((7, 67, 5), "spo_any"),
              ((16, 64, 16, 1), "spo3_row_fast+spo3_mid64_c4+spo3_col_fast_c2"),
              ((16, 16, 16, 1), "spo3_row_fast+spo3_mid_fast_c4+spo3_col_fast_c2"),
              ((64, 16, 64, 2), "spo3_row64+spo3_mid_fast_c8+spo3_col64_c4"),
              ((64, 16, 128, 1), "spo3_row_fast+spo3_mid_fast_c8+spo3_col64_c8"),
              ((32, 16, 128, 2), "spo3_row_fast+spo3_mid_fast_c8+spo3_col_fast_c4"),
              ((16, 16, 256, 2), "spo3_row_q16+spo3_mid_fast_c8+spo3_col_fast_c4"),
              ((32, 16, 256, 1), "spo3_row_q16+spo3_mid_fast_c8+spo3_col_fast_c8"),
              ((32, 16, 64, 4), "spo3_row_lds+spo3_mid_fast_c8+spo3_col_lds_c2"),
              ((64, 16, 64, 4), "spo3_row_lds+spo3_mid_fast_c16+spo3_col_lds_c4"),
              ((16, 128, 16, 1), "spo3_row_fast+spo3_mid_lds_c4+spo3_col_fast_c2"),
              ((16, 256, 16, 1), "spo3_row_fast+spo3_mid_lds_c4+spo3_col_fast_c2"),
              ((16, 128, 64, 8), "spo3_row_lds+spo3_mid_lds_c8+spo3_col_lds_c2"),
              ((16, 64, 64, 8), "spo3_row_lds+spo3_mid64_c8+spo3_col_lds_c2"),
              ((16, 64, 128, 8), "spo3_row_lds+spo3_mid64_c16+spo3_col_lds_c2"),
              ((256, 16, 16, 2), "spo3_row_fast+spo3_mid_fast_c8+spo3_col_q16")]


@pytest.mark.parametrize("dims,path", SPO3_CASES)
def test_spo3_fft_passes(dims, path, monkeypatch):
    from oracle import spo as osp
    from pyqed_amd import SPO3
    dims, ns = dims[:3], (dims[3:] or (2,))[0]
    x, y, z = (np.linspace(-l, l, n) for l, n in zip((6.0, 5.0, 5.5), dims))
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    # ns displaced wells (ns = 2: centres -1 and 1), neighbours coupled
    surfaces = [0.5 * ((X - c) ** 2 + Y ** 2 + Z ** 2) for c in (np.linspace(-1, 1, ns) if ns > 1 else (0.0,))]
    sol = SPO3(x, y, z, masses=[1.0, 1.2, 0.9], nstates=ns)
    sol.set_DPES(surfaces, [[[a, a + 1], 0.2 * X] for a in range(ns - 1)])
    monkeypatch.setattr(SPO3, "kinetic_path", "fft")
    psi0 = white(dims + (ns,), 400 + sum(dims))
    took("")
    r = sol.run(psi0=psi0, dt=DT, nt=NT, nout=NOUT)
    got = took("")[1]
    for name in path.split("+"):
        assert name in got, (name, got)
    pl, fin = osp.spo3_run(sol.exp_V_half, sol.exp_K, psi0, NT, NOUT)
    assert len(r.psilist) == len(pl) == NT // NOUT
    check(f"SPO3 {dims} x {ns}", [(r.psi, fin)] + [(r.psilist[k], pl[k]) for k in range(len(pl))], dims)
