"""lc_align_stack on the device (DESIGN.md §5 "Align and stack"): the aligned cubes against scipy in float64, the stack stage
against the float64 restatement of tests/_align_stack.py, stack_data_diagnostic(on_device=True) against the host
function, the error codes.  Every bound is four times the float32 restatement's own error against the same oracle
(AS.F32_ALIGN_ERROR, AS.F32_STACK_ERROR: measured by tests/test_align_stack_cpu.py), the project's margin for
reassociation."""
import ctypes as C

import numpy as np
import pytest

from tests import _align_stack as AS

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('n', AS.SIZES)
def test_aligned_cubes_equal_scipy(ctx, n):
    from lightcurver_amd.processes.roi_modelling import align_stack_batch
    E, nc = len(AS.GEOMETRIES), 2
    cubes = np.stack([AS.make_blobs(E, n, seed=n), AS.make_blobs(E, n, seed=1000 + n)])
    shift_yx, angle = AS.geometry_arrays(E)
    got = align_stack_batch(cubes, None, shift_yx, angle, want=('aligned',), ctx=ctx)
    assert got['aligned'].dtype == np.float32 and got['aligned'].shape == cubes.shape
    worst = 0.0
    for c in range(nc):
        for e, (s_y, s_x, ang) in enumerate(AS.GEOMETRIES):
            assert AS.coordinate_margin(n, s_y, s_x, ang) >= 1e-9
            assert ang % 90.0 != 0.0 or ang == 0.0
            ref = AS.scipy_align(cubes[c, e], s_y, s_x, ang)
            dev = got['aligned'][c, e]
            assert np.array_equal(dev == 0.0, ref == 0.0), (c, e)      # the in-range decision, pixel for pixel
            worst = max(worst, np.abs(dev - ref).max() / np.abs(ref).max())
    print(f'n={n}: device against scipy {worst:.2e} of the peak (bound {4 * AS.F32_ALIGN_ERROR[n]:.1e}), kernel '
          f'{got["kernel_ms"]:.3f} ms')
    assert worst <= 4 * AS.F32_ALIGN_ERROR[n]


@pytest.mark.parametrize('n', (17, 64))
def test_integer_shift_moves_the_pixels(ctx, n):
    from lightcurver_amd.processes.roi_modelling import align_stack_batch
    s_y, s_x, ang = AS.INTEGER_SHIFT
    img = AS.make_blobs(1, n, seed=50 + n)
    got = align_stack_batch(img[None], None, [[s_y, s_x]], [ang], want=('aligned',), ctx=ctx)['aligned'][0, 0]
    ref = AS.scipy_align(img[0], s_y, s_x, ang)
    bound = 4 * AS.F32_ALIGN_ERROR[n] * np.abs(ref).max()
    assert np.abs(got - ref).max() <= bound
    moved = np.zeros((n, n))
    moved[2:, :n - 3] = img[0, :n - 2, 3:]                               # out(y, x) = in(y - 2, x + 3), 0 outside
    assert np.abs(got - moved).max() <= bound


@pytest.mark.parametrize('n', (17, 32))
def test_nan_positions_equal_scipy(ctx, n):
    from lightcurver_amd.processes.roi_modelling import align_stack_batch
    E = len(AS.GEOMETRIES)
    cube = AS.make_blobs(E, n, seed=7 * n)
    cube[1, 5, n - 6] = np.nan                                           # one pixel of one epoch
    shift_yx, angle = AS.geometry_arrays(E)
    got = align_stack_batch(cube[None], None, shift_yx, angle, want=('aligned',), ctx=ctx)['aligned'][0]
    for e, (s_y, s_x, ang) in enumerate(AS.GEOMETRIES):
        ref = AS.scipy_align(cube[e], s_y, s_x, ang)
        assert np.array_equal(np.isnan(got[e]), np.isnan(ref)), e
        assert np.isnan(ref).any() == (e == 1)
        assert np.array_equal(got[e] == 0.0, ref == 0.0)


@pytest.mark.parametrize('case', AS.STACK_CASES)
def test_stack_stage_equals_the_restatement(ctx, case):
    from lightcurver_amd.processes.roi_modelling import align_stack_batch, median_stack_batch
    E, n = case
    values, noise = AS.make_stack_case(3, E, n, AS.stack_seed(case))
    o64 = AS.stack_cubes(values, noise, dtype=np.float64)
    o32 = AS.stack_cubes(values, noise, dtype=np.float32)
    got = align_stack_batch(values, noise, want=('stack', 'median', 'n_rejected'), ctx=ctx)
    assert got['median'].dtype == np.float32 and got['n_rejected'].dtype == np.int32
    assert np.array_equal(_bits(got['median']), _bits(o32['median']))
    assert np.array_equal(_bits(median_stack_batch(values, ctx=ctx)), _bits(o32['median']))
    near = o64['near']
    assert near.mean() <= AS.NEAR_CAP
    if E >= 64:
        assert (o64['n_rejected'] > 0).mean() >= 0.05
    ok = ~near
    assert np.array_equal(got['n_rejected'][ok], o64['n_rejected'][ok])
    assert np.array_equal(np.isnan(got['stack'][ok]), np.isnan(o64['stack'][ok]))
    err = np.nanmax(np.abs(got['stack'][ok] - o64['stack'][ok])) / np.nanmax(np.abs(o64['stack']))
    print(f'E={E} n={n}: device stack against float64 {err:.2e} (bound {4 * AS.F32_STACK_ERROR[case]:.1e}), left out '
          f'{near.sum()} pixels, kernel {got["kernel_ms"]:.3f} ms')
    assert err <= 4 * AS.F32_STACK_ERROR[case]
    # clip = 0: the plain weighted mean
    plain = align_stack_batch(values, noise, clip=False, want=('stack', 'n_rejected'), ctx=ctx)
    p64 = AS.stack_cubes(values, noise, clip=False, dtype=np.float64)
    assert not plain['n_rejected'].any()
    assert np.array_equal(np.isnan(plain['stack']), np.isnan(p64['stack']))
    assert np.nanmax(np.abs(plain['stack'] - p64['stack'])) <= 4 * AS.F32_STACK_ERROR[case] * np.nanmax(np.abs(p64['stack']))


@pytest.mark.parametrize('case,n_sigma', AS.N_SIGMA_CASES)
def test_stack_stage_at_other_n_sigma(ctx, case, n_sigma):
    """The assertions of test_stack_stage_equals_the_restatement at an n_sigma other than 3, where the rejection counts
    differ from those at 3 (tests/test_align_stack_cpu.py asserts that), against four times the figure measured for this
    (case, n_sigma)."""
    from lightcurver_amd.processes.roi_modelling import align_stack_batch
    E, n = case
    values, noise, o64, o32, at3 = AS.n_sigma_wanted(case, n_sigma)
    got = align_stack_batch(values, noise, n_sigma=n_sigma, want=('stack', 'median', 'n_rejected'), ctx=ctx)
    assert np.array_equal(_bits(got['median']), _bits(o32['median']))
    near = o64['near']
    assert near.mean() <= AS.NEAR_CAP
    ok = ~near
    bound = 4 * AS.F32_STACK_ERROR_N_SIGMA[case, n_sigma]
    err = np.nanmax(np.abs(got['stack'][ok] - o64['stack'][ok])) / np.nanmax(np.abs(o64['stack']))
    print(f'E={E} n={n} n_sigma={n_sigma}: device stack against float64 {err:.2e} (bound {bound:.1e}), rejected epochs per '
          f'pixel {got["n_rejected"].mean():.2f} (restatement {o64["n_rejected"].mean():.2f}, at 3 '
          f'{at3["n_rejected"].mean():.2f}), left out {near.sum()} pixels')
    assert got['n_rejected'].dtype == np.int32 and np.array_equal(got['n_rejected'][ok], o64['n_rejected'][ok])
    assert np.array_equal(np.isnan(got['stack'][ok]), np.isnan(o64['stack'][ok]))
    assert err <= bound


def test_stack_data_diagnostic_on_device_equals_the_host(ctx):
    from lightcurver_amd.processes import roi_modelling as RM
    from lightcurver_amd.starred.deconvolution.deconvolution import setup_model
    from lightcurver_amd.synthetic import make_roi_dataset
    E, M, n, ss = 12, 2, 32, 2
    rng = np.random.default_rng(11)
    angles = rng.uniform(-0.5, 0.5, E)
    angles[0] = 0.0
    angles[1::2] += 180.0
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=21, alpha=angles)
    t = ds['truth']
    data, noise = ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64)
    model, k, _, _, _ = setup_model(data, noise ** 2, ds['psf'], t['c_x'], t['c_y'], ss, list(t['a']), ctx=ctx)
    for name in ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha'):
        k['kwargs_analytic'][name] = np.array(t[name], dtype=np.float64)
    for name in ('h', 'mean'):
        k['kwargs_background'][name] = np.array(t[name], dtype=np.float64)
    host = RM.stack_data_diagnostic(data, noise, k, model)
    dev = RM.stack_data_diagnostic(data, noise, k, model, on_device=True, ctx=ctx)
    assert set(dev) == set(host) == {'stack', 'stack_no_ps', 'stack_no_background'}
    # the same three cubes through both paths, for the rejection counts
    only_ps, no_ps = RM.deepcopy(k), RM.deepcopy(k)
    only_ps['kwargs_background']['h'] = np.array(k['kwargs_background']['h']) * 0.0
    no_ps['kwargs_analytic']['a'] = np.array(k['kwargs_analytic']['a']) * 0.0
    cubes = {'stack': data, 'stack_no_ps': data - model.model(only_ps), 'stack_no_background': data - model.model(no_ps)}
    batch = RM.align_data_interpolation_batch(np.stack(list(cubes.values())), k, ctx=ctx)
    shift_yx, angle = RM._alignment_of(k)
    counts = RM.align_stack_batch(np.stack(list(cubes.values())), noise, shift_yx, angle, want=('n_rejected',), ctx=ctx)
    for i, (key, cube) in enumerate(cubes.items()):
        aligned = RM.align_data_interpolation(cube, k)
        peak = np.abs(aligned).max()
        assert batch[i].shape == aligned.shape
        assert np.abs(batch[i] - aligned).max() <= 4 * AS.F32_ALIGN_ERROR[n] * peak
        o = AS.stack(aligned, noise, dtype=np.float64)
        same = counts['n_rejected'][i] == o['n_rejected']
        assert (~same).mean() <= 0.01
        assert dev[key].shape == host[key].shape == (n, n)
        assert np.array_equal(np.isnan(dev[key][same]), np.isnan(host[key][same]))
        err = np.nanmax(np.abs(dev[key][same] - host[key][same])) / peak
        print(f'{key}: device against host {err:.2e} of the aligned peak, rejection counts differ at {(~same).sum()} pixels')
        assert err <= 4 * AS.F32_ALIGN_ERROR[n]


def test_error_codes(ctx):
    from lightcurver_amd import _lib
    lib = _lib.lib()

    def call(n, E, shift=0.25, n_sigma=3.0):
        v = np.ones((1, max(E, 1), n, n), np.float32)
        s = np.ones((max(E, 1), n, n), np.float32)
        sh = np.full((max(E, 1), 2), shift, np.float64)
        ang = np.zeros(max(E, 1), np.float64)
        out = np.zeros((1, n, n), np.float32)
        cfg = _lib.StackCfg(n_sigma, 1)
        return lib.lc_align_stack(ctx.h, 1, E, n, _lib.ptr(v), _lib.ptr(s), sh.ctypes.data_as(_lib.dp),
                                  ang.ctypes.data_as(_lib.dp), C.byref(cfg), None, _lib.ptr(out), None, None, None)
    assert call(16, 2) == 0
    assert call(7, 2) == -3 and call(129, 2) == -3          # LC_ERR_UNSUPPORTED
    assert call(16, 0) == -1                                # LC_ERR_INVALID
    assert call(16, 2, shift=np.nan) == -1
    assert call(16, 2, n_sigma=0.0) == -1 and call(16, 2, n_sigma=np.inf) == -1
    with pytest.raises(_lib.LcError):
        from lightcurver_amd.processes.roi_modelling import median_stack_batch
        median_stack_batch(np.ones((1, 2, 7, 7), np.float32), ctx=ctx)
