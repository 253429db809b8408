"""The SPEC of DESIGN.md §5 "Align and stack" without a GPU: its NumPy restatement (tests/_align_stack.py) against scipy -
the prefilter against spline_filter, the alignment against rotate(shift(...)) - and against the host functions of
processes/roi_modelling.py; the float32 figures the device tests take their bounds from; the exported symbols."""
import ctypes

import numpy as np
import pytest

from tests import _align_stack as AS


@pytest.mark.parametrize('n', AS.SIZES)
def test_float64_restatement_equals_scipy(n):
    from scipy.ndimage import spline_filter
    imgs = AS.make_blobs(len(AS.GEOMETRIES) + 1, n, seed=n)
    geos = AS.GEOMETRIES + (AS.INTEGER_SHIFT,)
    worst_filter = worst = 0.0
    for img, (s_y, s_x, angle) in zip(imgs.astype(np.float64), geos):
        want = spline_filter(img, 3, mode='mirror')
        worst_filter = max(worst_filter, np.abs(AS.prefilter(img) - want).max() / np.abs(want).max())
        ref = AS.scipy_align(img, s_y, s_x, angle)
        got = AS.align(img, s_y, s_x, angle)
        assert AS.coordinate_margin(n, s_y, s_x, angle) >= 1e-9
        assert np.array_equal(got == 0.0, ref == 0.0)          # the in-range decision, pixel for pixel
        assert (ref == 0.0).any() == (angle != 0.0)            # (a zero angle resamples the shift's zeros: rounding dust)
        worst = max(worst, np.abs(got - ref).max() / np.abs(ref).max())
    print(f'n={n}: prefilter {worst_filter:.2e}, rotate(shift()) {worst:.2e} of the peak')
    assert worst_filter <= 1e-12 and worst <= 1e-12


@pytest.mark.parametrize('n', AS.SIZES)
def test_float32_restatement_error_is_the_recorded_one(n):
    """The figure the device is held to four times of (AS.F32_ALIGN_ERROR): printed, and not exceeded."""
    imgs = AS.make_blobs(len(AS.GEOMETRIES), n, seed=n)
    worst = 0.0
    for img, (s_y, s_x, angle) in zip(imgs, AS.GEOMETRIES):
        ref = AS.scipy_align(img, s_y, s_x, angle)
        got = AS.align(img, s_y, s_x, angle, np.float32)
        assert got.dtype == np.float32 and np.array_equal(got == 0.0, ref == 0.0)
        worst = max(worst, np.abs(got - ref).max() / np.abs(ref).max())
    print(f'n={n}: float32 restatement against scipy {worst:.2e} of the peak (recorded {AS.F32_ALIGN_ERROR[n]:.1e})')
    assert worst <= AS.F32_ALIGN_ERROR[n]


def test_nan_spreads_as_in_scipy():
    img = AS.make_blobs(1, 17, seed=3)[0]
    img[5, 11] = np.nan
    for s_y, s_x, angle in AS.GEOMETRIES:
        ref = AS.scipy_align(img, s_y, s_x, angle)
        for dtype in (np.float64, np.float32):
            got = AS.align(img.astype(dtype), s_y, s_x, angle, dtype)
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == 0.0, ref == 0.0)
        assert np.isnan(ref).any()


@pytest.mark.parametrize('case', AS.STACK_CASES)
def test_stack_restatement_equals_the_host_function(case):
    from lightcurver_amd.processes.roi_modelling import sigma_clipped_weighted_stack
    E, n = case
    values, noise = AS.make_stack_case(3, E, n, AS.stack_seed(case))
    o64 = AS.stack_cubes(values, noise, dtype=np.float64)
    o32 = AS.stack_cubes(values, noise, dtype=np.float32)
    # the median: an exact order statistic, bit for bit numpy's on the float32 samples
    want = np.nanmedian(values, axis=1)
    assert o32['median'].dtype == np.float32
    assert np.array_equal(o32['median'].view(np.uint32), want.view(np.uint32))
    # the float64 form is the host's sigma_clipped_weighted_stack (up to the order of its sums)
    for c in range(3):
        host = sigma_clipped_weighted_stack(values[c], noise)
        assert np.array_equal(np.isnan(host), np.isnan(o64['stack'][c]))
        assert np.nanmax(np.abs(host - o64['stack'][c])) <= 1e-12 * np.nanmax(np.abs(host))
    # the oracle alone: few pixels on a rejection boundary, enough pixels that reject something
    near = o64['near']
    assert near.mean() <= AS.NEAR_CAP
    if E >= 64:
        assert (o64['n_rejected'] > 0).mean() >= 0.05
    ok = ~near
    assert np.array_equal(o32['n_rejected'][ok], o64['n_rejected'][ok])
    assert np.array_equal(np.isnan(o32['stack']), np.isnan(o64['stack']))
    err = np.nanmax(np.abs(o32['stack'][ok] - o64['stack'][ok])) / np.nanmax(np.abs(o64['stack']))
    print(f'E={E} n={n}: near a boundary {near.mean():.4f}, rejecting {(o64["n_rejected"] > 0).mean():.3f}, float32 stack '
          f'{err:.2e} (recorded {AS.F32_STACK_ERROR[case]:.1e})')
    assert err <= AS.F32_STACK_ERROR[case]
    # clip off: the plain weighted mean over the finite samples
    plain = AS.stack_cubes(values, noise, clip=False, dtype=np.float64)
    w = np.where(np.isfinite(values), 1.0 / noise.astype(np.float64)[None], 0.0)
    with np.errstate(invalid='ignore'):
        mean = (w * np.nan_to_num(values.astype(np.float64))).sum(axis=1) / w.sum(axis=1)
    assert not plain['n_rejected'].any()
    assert np.nanmax(np.abs(plain['stack'] - mean)) <= 1e-12 * np.nanmax(np.abs(mean))


@pytest.mark.parametrize('case,n_sigma', AS.N_SIGMA_CASES)
def test_stack_restatement_at_other_n_sigma(case, n_sigma):
    """The figure the device is held to four times of at an n_sigma other than 3 (AS.F32_STACK_ERROR_N_SIGMA,
    DESIGN.md): printed, and not exceeded.  The case is there to catch a kernel that ignores n_sigma, so the rejection
    counts must differ from those at n_sigma = 3, and few pixels may sit on a rejection boundary."""
    E, n = case
    values, noise, o64, o32, at3 = AS.n_sigma_wanted(case, n_sigma)
    near = o64['near']
    assert near.mean() <= AS.NEAR_CAP
    differ = (o64['n_rejected'] != at3['n_rejected']).mean()
    assert differ >= 0.05 and not np.array_equal(o64['stack'], at3['stack'], equal_nan=True)
    ok = ~near
    assert np.array_equal(o32['n_rejected'][ok], o64['n_rejected'][ok])
    assert np.array_equal(np.isnan(o32['stack']), np.isnan(o64['stack']))
    err = np.nanmax(np.abs(o32['stack'][ok] - o64['stack'][ok])) / np.nanmax(np.abs(o64['stack']))
    recorded = AS.F32_STACK_ERROR_N_SIGMA[case, n_sigma]
    print(f'E={E} n={n} n_sigma={n_sigma}: near a boundary {near.mean():.4f}, rejected epochs per pixel '
          f'{o64["n_rejected"].mean():.2f} ({at3["n_rejected"].mean():.2f} at 3; {differ:.2f} of the pixels differ), float32 '
          f'stack {err:.2e} (recorded {recorded:.1e})')
    assert err <= recorded
    # the sigma-clipped stack of the host function at this n_sigma, up to the order of its sums
    from lightcurver_amd.processes.roi_modelling import sigma_clipped_weighted_stack
    host = sigma_clipped_weighted_stack(values[0], noise, n_sigma=n_sigma)
    assert np.nanmax(np.abs(host - o64['stack'][0])) <= 1e-12 * np.nanmax(np.abs(host))


def test_n_sigma_cases_are_the_listed_ones():
    assert set(AS.F32_STACK_ERROR_N_SIGMA) == set(AS.N_SIGMA_CASES) and len(AS.N_SIGMA_CASES) == 10
    assert all(ns != 3.0 and tuple(case) in AS.STACK_CASES for case, ns in AS.N_SIGMA_CASES)
    # (3, 16) at n_sigma 1: the float64 restatement alone has more pixels on a boundary than the cap allows
    values, noise = AS.make_stack_case(3, 3, 16, AS.stack_seed((3, 16)))
    assert AS.stack_cubes(values, noise, n_sigma=1.0)['near'].mean() > AS.NEAR_CAP


def test_symbols_are_exported_and_the_size_query_needs_no_device():
    from lightcurver_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, 'lc_align_stack') and hasattr(handle, 'lc_align_stack_supported')
    lib = _lib.lib()
    assert [lib.lc_align_stack_supported(n) for n in (8, 33, 128)] == [1, 1, 1]
    assert [lib.lc_align_stack_supported(n) for n in (7, 129)] == [0, 0]
    assert ctypes.sizeof(_lib.StackCfg) == 8
