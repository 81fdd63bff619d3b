"""White-noise conformance of qd_fft_axis per plan class: the fused power-of-two Stockham kernel (fft.hip) and every
plan of the any-size engine (spo_gen.hip: mixed radix with generic prime stages, Bluestein, four-step, direct DFT),
forward and inverse, against numpy.fft.  White noise excites every bin, so a wrong twiddle, permutation or butterfly
output anywhere in the spectrum shows; the bounds (tests/fft_cases.py: tol(n) = 64 u (1 + log2 n) relative L2 per
call, 4 tol(n) ||x_line||_2 per bin) sit at the rounding error of an fp64 FFT, so a precision loss shows too.
Each test prints the worst err / tol it measured (DESIGN.md tabulates them)."""
import numpy as np
import pytest

import fft_cases as fc
from conftest import took

pytestmark = pytest.mark.gpu


def raw(a, inverse, axis=1):
    from pyqed_amd import fft as pf
    return pf._fft_axis(a, axis, inverse, 1.0, None, 0.0, shift=False)


def expected_path(n):
    return "fft_pow2" if n in (16, 32, 64, 128, 256, 512, 1024) else "fft_any"


def worst_ratio(cases, seed, check_path=False):
    """Forward and inverse of every (n, outer, inner), each asserted within the bounds as it is measured; returns the
    worst (L2 err / tol, per-bin err / (4 tol)) for the printed figure."""
    rng = np.random.default_rng(seed)
    worst = (0.0, 0.0, None)
    for n, o, i in cases:
        a = fc.noise(rng, (o, n, i))
        for inverse in (False, True):
            took("")
            got = raw(a, inverse)
            if check_path:
                paths = took("")[1]
                assert [p for p in paths if p.startswith("fft_")] == [expected_path(n)], (n, paths)
            r = fc.ratios(got, fc.reference(a, inverse), a, n)
            assert fc.within(*r), (n, o, i, "inverse" if inverse else "forward", r)
            if max(r) > max(worst[:2]):
                worst = (r[0], r[1], (n, o, i, "inverse" if inverse else "forward"))
    return worst


def report(name, worst):
    l2r, pbr, at = worst
    print(f"fft conformance {name}: worst err/tol L2 {l2r:.4f} per-bin {pbr:.4f} at {at}")
    assert at is not None and fc.within(l2r, pbr), (name, worst)


@pytest.mark.parametrize("cls", list(fc.CLASSES))
def test_white_noise_by_plan_class(cls):
    report(cls, worst_ratio([(n, 2, 3) for n in fc.CLASSES[cls]], seed=21, check_path=True))


def test_length_one_returns_the_input_bits():
    a = fc.noise(np.random.default_rng(22), (3, 1, 5))
    for inverse in (False, True):
        assert np.array_equal(raw(a, inverse).view(np.int64), a.view(np.int64))


@pytest.mark.parametrize("lo", [1, 81, 161, 241])
def test_white_noise_dense_sweep(lo):
    """Every length 1..320 at (2, n, 3), so that no small factorisation is skipped."""
    cases = [(n,) + fc.DENSE_SHAPE for n in fc.DENSE if lo <= n < lo + 80]
    report(f"dense {lo}..{lo + 79}", worst_ratio(cases, seed=23 + lo, check_path=True))


@pytest.mark.parametrize("n", fc.SHAPE_LENGTHS)
def test_white_noise_batch_and_inner_shapes(n):
    """Column tiles (8 columns with a partial last tile at (90, 17), one column where fewer than 256 tiles would be
    left), whole rows stacked G to a tile with an odd row count (outer 601, 1025), single lines."""
    report(f"shapes n={n}", worst_ratio([c for c in fc.shape_cases() if c[0] == n], seed=24 + n))


def test_white_noise_along_first_and_last_axis():
    """axis 0 (outer 1, inner = the rest) and axis -1 (inner 1) of a 3D array, as pyqed.fft passes them."""
    rng = np.random.default_rng(25)
    worst = (0.0, 0.0, None)
    for shape, axis in (((67, 5, 3), 0), ((4, 3, 128), -1), ((128, 7, 2), 0), ((3, 4, 45), 2)):
        a = fc.noise(rng, shape)
        n = shape[axis]
        for inverse in (False, True):
            got = raw(a, inverse, axis)
            r = fc.ratios(got, fc.reference(a, inverse, axis), a, n, axis)
            assert fc.within(*r), (shape, axis, inverse, r)
            if max(r) > max(worst[:2]):
                worst = (r[0], r[1], (shape, axis, inverse))
    report("axes", worst)


# ---------------------------------------------------------------- structure, independent of the noise
@pytest.mark.parametrize("n", fc.STRUCT_LENGTHS)
def test_impulse_gives_every_twiddle(n):
    """A unit impulse at j returns w^(j k) at every bin: each output is one twiddle product, none averaged away."""
    worst = 0.0
    for inverse in (False, True):
        for j in (n - 1, n // 2):
            a = np.zeros((1, n, 1), complex)
            a[0, j, 0] = 1.0
            got = raw(a, inverse)[0, :, 0]
            r = float(np.max(np.abs(got - fc.impulse_ref(n, j, inverse)))) / fc.tol(n)
            assert fc.within(r), (n, j, inverse, r)
            worst = max(worst, r)
    print(f"fft conformance impulse n={n}: worst per-bin err/tol {worst:.4f}")


@pytest.mark.parametrize("n", fc.STRUCT_LENGTHS)
def test_single_tone_lands_in_one_bin(n):
    worst = 0.0
    for inverse in (False, True):
        for k0 in (n - 1, n // 2):
            a = fc.tone(n, k0, inverse).reshape(1, n, 1)
            got = raw(a, inverse)[0, :, 0]
            ref = np.zeros(n, complex)
            ref[k0] = n
            r = float(np.max(np.abs(got - ref))) / (fc.tol(n) * n)
            assert fc.within(r), (n, k0, inverse, r)
            worst = max(worst, r)
    print(f"fft conformance tone n={n}: worst per-bin err/(tol n) {worst:.4f}")


@pytest.mark.parametrize("n", fc.STRUCT_LENGTHS)
def test_round_trip_and_determinism(n):
    """Forward then inverse returns n x within 2 tol(n); the same call twice returns the same bits."""
    a = fc.noise(np.random.default_rng(26 + n), (2, n, 3))
    f1 = raw(a, False)
    assert np.array_equal(f1.view(np.int64), raw(a, False).view(np.int64))
    back = raw(f1, True)
    assert np.array_equal(back.view(np.int64), raw(f1, True).view(np.int64))
    err = np.linalg.norm(back - n * a) / np.linalg.norm(n * a) / (2.0 * fc.tol(n))
    print(f"fft conformance round trip n={n}: err/(2 tol) {err:.4f}")
    assert fc.within(err)


# ---------------------------------------------------------------- fused shift / scale / phase epilogue
@pytest.mark.parametrize("n", fc.EPILOGUE_LENGTHS)
def test_shift_and_phase_epilogue(n):
    """pf.fft / pf.ifft with a non-zero x[0], odd and even n: fft_store (fused, the fft_pow2 lengths) and
    fft_post_kernel (every other length, with the four-step slot order at 5121) against
    fftshift(fft(a)) dx exp(-i w x0) and fftshift(ifft(a)) dx n exp(+i w x0)."""
    from pyqed_amd import fft as pf
    rng = np.random.default_rng(27 + n)
    a = fc.noise(rng, (2, n, 3))
    dx, x0 = 0.37, -1.3
    x = x0 + dx * np.arange(n)
    dx, x0 = x[1] - x[0], x[0]
    w = 2.0 * np.pi * np.fft.fftshift(np.fft.fftfreq(n, d=dx))
    ph = np.exp(-1j * w * x0)[None, :, None]
    worst = (0.0, 0.0)
    for fn, ref in ((pf.fft, np.fft.fftshift(np.fft.fft(a, axis=1), axes=1) * dx * ph),
                    (pf.ifft, np.fft.fftshift(np.fft.ifft(a, axis=1), axes=1) * dx * n * np.conj(ph))):
        got, freq = fn(a, x, axis=1)
        assert np.array_equal(freq, w)
        l2, pb = fc.line_errors(got, ref, a * dx)
        r = (l2 / fc.tol(n), pb / (4.0 * fc.tol(n)))
        assert fc.within(*r), (n, fn.__name__, r)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"fft conformance epilogue n={n}: worst err/tol L2 {worst[0]:.4f} per-bin {worst[1]:.4f}")


# ---------------------------------------------------------------- nothing outside the array is written
@pytest.mark.parametrize("n,outer,inner", [(67, 3, 17), (12, 601, 1), (128, 5, 3)])
def test_guard_bands_stay_untouched(n, outer, inner):
    """qd_fft_axis on the middle of a larger device buffer: the sentinels before and after keep their bits.  What writes
    the caller's buffer is guarded: at 128 the fused kernel, which transforms in place; at 67 and 12 only
    fft_post_kernel, since the any-size engine works on a scratch copy whose stores the sentinels cannot see."""
    import torch
    from pyqed_amd import _lib
    from pyqed_amd._util import default_device
    dev = default_device()
    _lib.ensure_device(dev)
    guard, tot = 4096, outer * n * inner
    a = fc.noise(np.random.default_rng(28 + n), (outer, n, inner))
    sentinel = complex(-7.25e300, 3.5e-300)
    host = np.full(guard + tot + guard, sentinel, complex)
    host[guard:guard + tot] = a.ravel()
    buf = torch.from_numpy(host.copy()).to(dev)
    for inverse in (False, True):
        buf.copy_(torch.from_numpy(host))
        with torch.cuda.device(dev):
            rc = _lib.load().qd_fft_axis(buf.data_ptr() + guard * 16, outer, n, inner, int(inverse), 0, 1.0, None, 0.0,
                                         _lib.stream_ptr(dev))
        _lib.check(rc, "qd_fft_axis")
        out = buf.cpu().numpy()
        want = np.full(guard, sentinel, complex).view(np.int64)
        assert np.array_equal(out[:guard].view(np.int64), want)
        assert np.array_equal(out[guard + tot:].view(np.int64), want)
        r = fc.ratios(out[guard:guard + tot].reshape(a.shape), fc.reference(a, inverse), a, n)
        assert fc.within(*r), (inverse, r)
