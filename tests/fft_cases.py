"""Lengths, shapes, tolerance and error measures shared by the white-noise FFT conformance tests: the GPU run
(test_fft_conformance_gpu.py), the solver run (test_spo_whitenoise_gpu.py) and the host emulation of the any-size
engine (test_fft_engine_host.py).

Tolerance: the rounding error of an fp64 FFT grows as u log2 n (Higham, Accuracy and Stability of Numerical
Algorithms, section 24.1), u = 2^-53.  tol(n) = 64 u (1 + log2 n) on the relative L2 error of one transform; the
constant covers Bluestein's three chained transforms of length up to 4 n and the sqrt(n) u statistical growth of the
direct sum up to n = 12288.  Per bin, |dX_k| <= 4 tol(n) ||x||_2 of the line: every white-noise bin has magnitude
about ||x||_2, so one bad bin cannot hide in the L2 norm."""
import numpy as np

U = 2.0 ** -53


def tol(n):
    return 64.0 * U * (1.0 + np.log2(n))


# one class per plan of the engine (pyqed_amd/csrc/fft_plan.hpp axis_plan / fourstep_split / fft_lines_plan, fft.hip)
TINY = [1, 2, 3, 4, 5, 7, 9, 15]
POW2 = [2 ** k for k in range(1, 14)]   # 16..1024: the fused Stockham kernel; 2048, 4096: LDS mixed radix; 8192: four-step
PRIMES_7_61 = [7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61]
PRIME_RADIX = PRIMES_7_61 + [2401, 4913, 3721, 3599, 5103]   # 7^4, 17^3, 61^2, 59 61, 3^6 7
MIXED_LIMIT = [5120, 5000, 3125, 2560]
BLUESTEIN = [67, 134, 213, 509, 1021, 2557]   # 509: M = 1024 = 2^(3j+1); 2557: M = next_smooth(5113) = 5120
DIRECT = [2579, 5158, 7919]                   # primes beyond the chirp-z plan, and 2 2579 with no plannable split
FOURSTEP = [5121, 5125, 6000, 6499, 5114, 10201, 12288]   # 9 569, 41 125, 75 80, 67 97, 2 2557, 101^2, 96 128
CLASSES = {"tiny": TINY, "pow2": POW2, "prime_radix": PRIME_RADIX, "mixed_limit": MIXED_LIMIT,
           "bluestein": BLUESTEIN, "direct": DIRECT, "fourstep": FOURSTEP}
DENSE = list(range(1, 321))
DENSE_SHAPE = (2, 3)                          # (outer, inner) of the dense sweep

SHAPE_LENGTHS = [12, 61, 67, 200, 1024]
# (outer, inner): single lines, column tiles, whole rows stacked G to a tile with an odd row count (601, 1025).  The
# engine narrows its column tiles until 256 of them exist, so only (90, 17) keeps the 8-column tile, with a partial
# last one (17 = 8 + 8 + 1); the smaller outer counts with inner > 1 run one column per tile
SHAPES = [(1, 1), (3, 8), (1, 17), (2, 9), (5, 64), (601, 1), (601, 2), (1025, 3), (90, 17)]
MAX_ELEMS = 400_000

STRUCT_LENGTHS = [61, 67, 128, 509, 2048, 2579, 5121, 6499]
EPILOGUE_LENGTHS = [5, 45, 128, 509, 5121]


def shape_cases():
    return [(n, o, i) for n in SHAPE_LENGTHS for (o, i) in SHAPES if n * o * i <= MAX_ELEMS]


def noise(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def reference(a, inverse, axis=1):
    """The raw transform qd_fft_axis computes with scale 1 and no shift: the unnormalised inverse is n ifft."""
    return np.fft.ifft(a, axis=axis) * a.shape[axis] if inverse else np.fft.fft(a, axis=axis)


def line_errors(got, ref, x, axis=1):
    """(relative L2 error of the call, worst per-bin error over ||x_line||_2 of its line)."""
    d = np.abs(got - ref)
    l2 = np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-300)
    xn = np.sqrt(np.sum(np.abs(x) ** 2, axis=axis, keepdims=True))
    return l2, float(np.max(d / np.maximum(xn, 1e-300)))


def ratios(got, ref, x, n, axis=1):
    """(L2 error / tol(n), per-bin error / (4 tol(n))): both must be <= 1."""
    l2, pb = line_errors(got, ref, x, axis)
    return l2 / tol(n), pb / (4.0 * tol(n))


def within(*rs):
    """Every ratio <= 1.  A NaN ratio (NaN or inf in the output) compares False and so fails, which max() over the
    ratios would not: max keeps whichever operand it saw first when the other is NaN."""
    return all(r <= 1.0 for r in rs)


def impulse_ref(n, j, inverse):
    """Transform of the unit impulse at j: w^(j k), w = exp(-+2 pi i / n), with j k mod n exact."""
    e = (j * np.arange(n, dtype=np.int64)) % n
    return np.exp((2j if inverse else -2j) * np.pi * e / n)


def tone(n, k0, inverse):
    """The input whose transform is n at bin k0 and 0 elsewhere: exp(+-2 pi i k0 m / n), k0 m mod n exact."""
    e = (k0 * np.arange(n, dtype=np.int64)) % n
    return np.exp((-2j if inverse else 2j) * np.pi * e / n)
