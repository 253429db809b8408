"""The restatement of the co-addition SPEC (tests/_coadd.py; DESIGN.md §5 "Co-addition of frames") against scipy and
against what the SPEC promises of it, the host code of processes/coaddition.py, the float32 figure the device tests take
their bound from, and the guard of their sigma_clip comparison.  No device."""
import ctypes

import numpy as np
import pytest

from tests import _coadd as CO


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- order 1 against scipy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', range(len(CO.GRIDS)))
def test_order_1_equals_scipy_where_every_tap_is_inside(grid):
    shape, origin = CO.GRIDS[grid]
    frames = CO.frames()
    for g, geometry in enumerate(CO.GEOMETRIES):
        A = CO.affine_of(geometry)
        img = frames[g]                                        # g = 1 is the frame with the NaN pixel
        got = CO.warp(img, A, shape, origin, order=1, dtype=np.float64)
        ref = CO.scipy_warp_order1(img, A, shape, origin)
        inside = got['inside']
        assert inside.sum() > 0.5 * min(inside.size, img.size) and np.isnan(got['sample'][~inside]).all()
        assert np.array_equal(np.isnan(got['sample'][inside]), np.isnan(ref[inside])), g
        assert np.isnan(got['sample'][inside]).any() == (g == CO.NAN_FRAME)
        err = np.nanmax(np.abs(got['sample'][inside] - ref[inside])) / np.nanmax(np.abs(ref[inside]))
        assert err <= 1e-12, (g, err)
    assert not CO.warp(frames[0], CO.affine_of(CO.GEOMETRIES[0]), *CO.GRIDS[1], order=1)['inside'].all()


# ---- order 3 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,tol', ((np.float64, 4e-16), (np.float32, 3e-7)))
def test_cubic_weights_sum_to_one(dtype, tol):
    t = np.linspace(0.0, 1.0, 4097)[:-1].astype(dtype)
    w = CO.cubic_weights(t, dtype)
    assert all(x.dtype == dtype for x in w)
    assert np.abs(sum(x.astype(np.float64) for x in w) - 1.0).max() <= tol
    at0 = [float(x[0]) for x in w]
    assert at0 == [0.0, 1.0, 0.0, 0.0]                          # t = 0: the sample itself (-0.0 == 0.0)


@pytest.mark.parametrize('order', (1, 3))
def test_integer_shift_is_a_bit_exact_copy(order):
    img = CO.frames()[0]
    h, w = img.shape
    A = CO.affine_of((3.0, -2.0, 0.0, 1.0))
    got = CO.warp(img, A, (h, w), order=order, dtype=np.float32)
    before, after = (1, 2) if order == 3 else (0, 1)
    moved = np.full((h, w), np.nan, np.float32)
    # out(y, x) = in(y - 2, x + 3) where the taps around it are inside
    for y in range(h):
        for x in range(w):
            yy, xx = y - 2, x + 3
            if before <= yy <= h - 1 - after and before <= xx <= w - 1 - after:
                moved[y, x] = img[yy, xx]
    assert got['sample'].dtype == np.float32
    assert np.array_equal(np.isnan(got['sample']), np.isnan(moved))
    ok = ~np.isnan(moved)
    assert np.array_equal(_bits(got['sample'][ok]), _bits(moved[ok]))


def test_order_3_reproduces_a_quadratic_under_a_similarity():
    h, w = 60, 70
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    quad = lambda x, y: 3.0 + 0.7 * x - 0.4 * y + 0.02 * x * x - 0.015 * x * y + 0.01 * y * y
    img = quad(x, y)
    A = CO.affine_of((0.37, -1.62, 12.0, 1.015), (h, w))
    got = CO.warp(img, A, (h, w), order=3, dtype=np.float64)
    xs, ys = A[0, 0] * x + A[0, 1] * y + A[0, 2], A[1, 0] * x + A[1, 1] * y + A[1, 2]
    want = quad(xs, ys) * 1.015 ** 2
    inside = got['inside']
    assert inside.sum() > 0.6 * h * w
    assert np.abs(got['sample'][inside] - want[inside]).max() <= 1e-12 * np.abs(img).max()


@pytest.mark.parametrize('order', (1, 3))
def test_a_constant_image_at_scale_s_gives_c_s_squared(order):
    c, s = 7.25, 1.015
    img = np.full((40, 48), c)
    got = CO.warp(img, CO.affine_of((0.3, 0.4, 33.0, s)), (40, 48), order=order, dtype=np.float64)
    assert np.abs(got['sample'][got['inside']] - c * s * s).max() <= 1e-13 * c
    got = CO.warp(img, CO.affine_of((0.3, 0.4, 33.0, s)), (40, 48), order=order, flux_scale=0.5, dtype=np.float64)
    assert np.abs(got['sample'][got['inside']] - 0.5 * c * s * s).max() <= 1e-13 * c


# ---- combine -----------------------------------------------------------------------------------------------------------
def _samples(n, seed, shape=(9, 11)):
    rng = np.random.default_rng(seed)
    v = rng.normal(10.0, 2.0, (n,) + shape)
    v[rng.random(v.shape) < 0.2] = np.nan
    v[:, 0, 0] = np.nan                                          # a pixel without any sample
    v[:n // 2 * 2, 0, 1] = rng.normal(10.0, 2.0, n // 2 * 2)     # an even count ...
    v[n // 2 * 2:, 0, 1] = np.nan
    return v, rng.uniform(0.0, 2.0, n)


@pytest.mark.parametrize('n', (1, 2, 5, 6, 13))
def test_combine_mean_and_median(n):
    v, w = _samples(n, 40 + n)
    fin = np.isfinite(v)
    mean = CO.combine(v, w, 'mean')
    with np.errstate(invalid='ignore', divide='ignore'):
        want = np.nansum(v * w[:, None, None], axis=0) / (fin * w[:, None, None]).sum(axis=0)
    assert np.array_equal(np.isnan(mean['image']), np.isnan(want))
    assert np.nanmax(np.abs(mean['image'] - want)) <= 1e-13 * 20
    assert np.allclose(mean['weight'], (fin * w[:, None, None]).sum(axis=0), rtol=1e-14, atol=0)
    assert np.array_equal(mean['count'], fin.sum(axis=0)) and not mean['n_rejected'].any()
    med = CO.combine(v, w, 'median')
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        want = np.nanmedian(v, axis=0)
    assert np.array_equal(np.isnan(med['image']), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.abs(med['image'][ok] - want[ok]).max() <= 1e-14 * 20
    assert np.array_equal(med['count'], fin.sum(axis=0)) and not med['n_rejected'].any()
    assert np.array_equal(med['weight'], mean['weight'])
    for out in (mean, med, CO.combine(v, w, 'sigma_clip')):
        assert np.isnan(out['image'][0, 0]) and out['weight'][0, 0] == 0 and out['count'][0, 0] == 0 \
            and out['n_rejected'][0, 0] == 0


def test_sigma_clip_on_a_case_worked_by_hand():
    """Eleven samples of 10 and one of 100: mean 17.5, population deviation sqrt(618.75) = 24.87, median 10; at 3 sigma the
    threshold is 74.6 < 90, so the outlier goes and the weighted mean of the rest is 10.  At 4 sigma (99.5 > 90) it stays.
    The distance is taken from the median and the deviation about the mean, so one outlier among m - 1 equal samples lies
    m / sqrt(m - 1) deviations out, the most there can be: a clip at 3 sigma rejects nothing below 8 samples (7 / sqrt(6) =
    2.86, 8 / sqrt(7) = 3.02).  About the mean the largest z-score would be (m - 1) / sqrt(m), which passes 3 at 11."""
    v = np.full((12, 1), 10.0)
    v[7] = 100.0
    w = np.linspace(0.5, 1.6, 12)
    for dtype in (np.float64, np.float32):
        out = CO.combine(v, w, 'sigma_clip', 3.0, dtype)
        assert out['image'].dtype == dtype
        assert abs(out['image'][0] - 10.0) <= 1e-6 and out['n_rejected'][0] == 1 and out['count'][0] == 11
        assert abs(out['weight'][0] - (w.sum() - w[7])) <= 1e-6 * w.sum()
        assert abs(out['margin'][0] - (90.0 - 3.0 * np.sqrt(618.75))) <= 1e-4
        out = CO.combine(v, w, 'sigma_clip', 4.0, dtype)
        assert out['n_rejected'][0] == 0 and out['count'][0] == 12
        assert abs(out['image'][0] - (w * v[:, 0]).sum() / w.sum()) <= 1e-5
    for m in range(1, 13):
        x = np.zeros((m, 1))
        x[0] = 1e6
        assert CO.combine(x, np.ones(m), 'sigma_clip', 3.0)['n_rejected'][0] == (1 if m >= 8 else 0), m


# ---- depth -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', (1, 3))
def test_depth_of_the_weighted_mean(order):
    """Pure noise of known sigma_k, w_k = 1 / sigma_k^2: the co-add's rms is at most 1.1 / sqrt(sum w).  Interpolation
    weights have sum w^2 <= 1, so interpolation only lowers the rms; the 10 % is the sampling margin at >= 5000 pixels."""
    rng = np.random.default_rng(9)
    h = w = 84
    sigma = np.array([1.0, 1.5, 0.8, 2.0, 1.2, 1.0])
    frames = (rng.standard_normal((len(sigma), h, w)) * sigma[:, None, None]).astype(np.float32)
    shifts = ((0.0, 0.0), (0.31, -0.77), (1.5, 0.5), (-0.2, 0.43), (2.25, -1.1), (-1.6, -0.35))
    affines = [CO.affine_of((sx, sy, 0.0, 1.0), (h, w)) for sx, sy in shifts]
    wk = 1.0 / sigma ** 2
    out = CO.coadd(frames, np.arange(len(sigma)), affines, (h, w), weights=wk, order=order, mode='mean', dtype=np.float32)
    full = out['count'] == len(sigma)
    assert full.sum() >= 5000
    rms = float(np.sqrt(np.mean(out['image'][full].astype(np.float64) ** 2)))
    print(f'order {order}: rms {rms:.4f} over {full.sum()} pixels, 1 / sqrt(sum w) = {1 / np.sqrt(wk.sum()):.4f}')
    assert rms <= 1.1 / np.sqrt(wk.sum())
    assert np.allclose(out['weight'][full], wk.sum(), rtol=1e-6)


# ---- host code ---------------------------------------------------------------------------------------------------------
def test_relative_flux_scales_on_made_up_tables():
    from lightcurver_amd.processes.coaddition import relative_flux_scales
    dt = np.dtype([('x', '<f8'), ('y', '<f8'), ('flux', '<f8')])

    def table(fluxes):
        t = np.zeros(len(fluxes), dt)
        t['flux'] = fluxes
        return t

    # tables in raster order; pairs number the rows brightest first, as table_positions sorts them
    ref = table([5.0, 100.0, 20.0, 50.0])                       # brightest first: 100, 50, 20, 5
    twice = table([40.0, 10.0, 200.0, 100.0, 3.0])              # 200, 100, 40, 10, 3
    odd = table([30.0, 1000.0, 75.0])                           # 1000, 75, 30: 10 x, 1.5 x, 1.5 x the reference's
    results = [dict(success=True, pairs=np.array([[0, 0], [1, 1], [2, 2], [3, 3]])),
               dict(success=True, pairs=np.array([[0, 0], [1, 1], [2, 2], [3, 3]])),
               dict(success=True, pairs=np.array([[0, 0], [1, 1], [2, 2]])),
               dict(success=False, pairs=np.zeros((0, 2), np.int64)),
               dict(success=True, pairs=np.zeros((0, 2), np.int64))]
    got = relative_flux_scales([ref, twice, odd, ref, ref], results, reference=0)
    assert got[0] == 1.0 and got[1] == 0.5 and got[2] == 1.0 / 1.5 and np.isnan(got[3]) and np.isnan(got[4])
    # the reference as a table of its own, a dict of characterize_frames, and pairs that are not the identity
    results = [dict(success=True, pairs=np.array([[3, 0], [0, 2]]))]                  # 5 <-> 200, 100 <-> 40
    got = relative_flux_scales([dict(sources_table=twice)], results, reference=ref)
    assert got[0] == 1.0 / np.median([200.0 / 5.0, 40.0 / 100.0])


def test_coadd_frames_skips_what_failed_without_a_device():
    from lightcurver_amd.processes.coaddition import coadd_frames

    class Recorder:
        def coadd(self, frame_index, transforms, **kw):
            return dict(frame_index=list(frame_index), transforms=transforms, kw=kw)

    results = [dict(success=True, transform='t0'), dict(success=False, transform=None), dict(success=True, transform='t2'),
               dict(success=True, transform='t3')]
    out = coadd_frames(Recorder(), results, order=1)
    assert out['frame_index'] == [0, 2, 3] and out['transforms'] == ['t0', 't2', 't3'] and out['frames'].tolist() == [0, 2, 3]
    assert out['kw'] == dict(flux_scale=None, weights=None, order=1)
    out = coadd_frames(Recorder(), results, frames=[3, 1, 0], flux_scale=[1.0, np.nan, 2.0, np.nan], weights=[4.0, 5.0, 6.0, 7.0])
    assert out['frame_index'] == [0] and out['kw']['flux_scale'].tolist() == [1.0] and out['kw']['weights'].tolist() == [4.0]
    with pytest.raises(ValueError, match='no registered frame'):
        coadd_frames(Recorder(), results, frames=[1])


def test_symbol_and_settings_structure():
    from lightcurver_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, 'lc_frames_coadd')
    res, args = _lib.SIGNATURES['lc_frames_coadd']
    assert res is ctypes.c_int and len(args) == 16
    assert [n for n, _ in _lib.CoaddCfg._fields_] == ['order', 'combine', 'n_sigma', 'scratch_rows']
    assert ctypes.sizeof(_lib.CoaddCfg) == 16
    assert _lib.COADD_COMBINE == {'mean': 0, 'median': 1, 'sigma_clip': 2}
    # a null set is refused without a device
    assert _lib.lib().lc_frames_coadd(None, 1, None, None, None, None, 4, 4, 0, 0, None, None, None, None, None, None) == -1


# ---- the figures the device tests rest on --------------------------------------------------------------------------------
def test_float32_warp_error_is_within_the_recorded_ratio():
    """c of the device's bound B = c 2^-24 |s| sum_taps |v|: the float32 restatement against the float64 one on the
    geometries, grids and orders of the device tests; the worst ratio r is recorded (CO.F32_WARP_RATIO) and the
    device is held to the next power of two >= 4 r."""
    frames = CO.frames()
    worst = {}
    for order in (1, 3):
        r = 0.0
        for shape, origin in CO.GRIDS:
            for g, geometry in enumerate(CO.GEOMETRIES):
                for scale in (1.0, 0.8371, 1.1934):
                    A = CO.affine_of(geometry)
                    lo = CO.warp(frames[g], A, shape, origin, order, scale, np.float32)
                    hi = CO.warp(frames[g], A, shape, origin, order, scale, np.float64)
                    assert lo['sample'].dtype == np.float32 and np.array_equal(lo['inside'], hi['inside'])
                    ok = hi['inside'] & np.isfinite(hi['sample'])
                    assert np.array_equal(np.isnan(lo['sample']), np.isnan(hi['sample']))
                    unit = CO.EPS * abs(float(hi['s'])) * hi['tapabs'][ok]
                    r = max(r, float((np.abs(lo['sample'][ok].astype(np.float64) - hi['sample'][ok]) / unit).max()))
        worst[order] = r
    print('worst |float32 - float64| of a sample in units of 2^-24 |s| sum_taps |v|:', worst)
    assert max(worst.values()) <= CO.F32_WARP_RATIO
    assert CO.C_BOUND == CO.next_power_of_two(4 * CO.F32_WARP_RATIO)


@pytest.mark.parametrize('n', CO.COUNTS)
def test_guard_of_the_sigma_clip_comparison(n):
    """On the device tests' own inputs: the pixels whose decision margin | |v - med| - n_sigma dev | is below twice the
    tolerance are left out of the device comparison, and are at most 1 % of every case."""
    for grid in range(len(CO.GRIDS)):
        for order in (1, 3):
            ref = CO.wanted(n, grid, order, 'sigma_clip')
            share = CO.guarded(ref).mean()
            print(f'n={n} grid={grid} order={order}: {CO.guarded(ref).sum()} guarded pixels ({100 * share:.2f} %), rejected '
                  f'samples per pixel {ref["n_rejected"].mean():.2f}')
            assert share <= CO.NEAR_CAP
            if n >= 5:
                assert ref['n_rejected'].any()
            assert np.isfinite(ref['image']).any() and (grid == 0 or (ref['count'] == 0).any())


@pytest.mark.parametrize('n', CO.LARGE_COUNTS)
def test_guard_of_the_comparison_at_large_frame_counts(n):
    shape, origin = CO.GRIDS[1]
    index, affines, g, w = CO.case_inputs(n)
    ref = CO.coadd(CO.frames(), index, affines, shape, origin, g, w, 3, 'sigma_clip', CO.LARGE_N_SIGMA, np.float64)
    assert CO.guarded(ref).mean() <= CO.NEAR_CAP and (ref['n_rejected'] > 0).mean() > 0.1
