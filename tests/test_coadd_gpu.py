"""lc_frames_coadd on the device (DESIGN.md §5 "Co-addition of frames"; FrameSet.coadd) against the float64 restatement
of tests/_coadd.py at small shapes where it can go wrong: h != w, a grid with uncovered pixels, six geometries, 1 to 67
frames, a NaN pixel, a frame outside the grid, a frame listed twice, a zero weight, both orders, the three combines, a raw
and an imported set.  A warped sample is held to B = c 2^-24 |s| sum_taps |v| with c = CO.C_BOUND (the next power of two
>= 4 times the float32 restatement's own worst ratio, measured by tests/test_coadd_cpu.py); a combined pixel to
max_k B_k + (m + 2) 2^-24 max_k |v_k| (CO.pixel_bound).  Validity, counts and rejections are compared exactly."""
import ctypes as C

import numpy as np
import pytest

from tests import _coadd as CO

pytestmark = pytest.mark.gpu

_ip = C.POINTER(C.c_int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def fs(ctx):
    from lightcurver_amd.frames import FrameSet
    with FrameSet(CO.frames(), ctx) as s:
        yield s


# ---- one frame: the mean co-add is the warp itself ------------------------------------------------------------------------
@pytest.mark.parametrize('order', (1, 3))
@pytest.mark.parametrize('grid', range(len(CO.GRIDS)))
def test_warp_of_one_frame(fs, grid, order):
    shape, origin = CO.GRIDS[grid]
    frames = CO.frames()
    for g, geometry in enumerate(CO.GEOMETRIES):
        A = CO.affine_of(geometry)
        for scale in (None, 0.8371):
            got = fs.coadd([g], [A], shape, origin, flux_scale=scale, order=order, combine='mean')
            ref = CO.warp(frames[g], A, shape, origin, order, 1.0 if scale is None else np.float32(scale), np.float64)
            assert got['image'].dtype == np.float32 and got['image'].shape == shape
            assert np.array_equal(np.isnan(got['image']), np.isnan(ref['sample'])), (g, scale)
            ok = np.isfinite(ref['sample'])
            assert ok.any() and (grid == 0 or not ref['inside'].all())
            bound = CO.sample_bound(ref['tapabs'], float(ref['s']))
            ratio = (np.abs(got['image'][ok] - ref['sample'][ok]) / bound[ok]).max() * CO.C_BOUND
            assert np.all(np.abs(got['image'][ok] - ref['sample'][ok]) <= bound[ok]), (g, scale, ratio)
            assert np.array_equal(got['count'], ok.astype(np.int32)) and not got['n_rejected'].any()
            assert np.array_equal(got['weight'], ok.astype(np.float32))
            low = CO.warp(frames[g], A, shape, origin, order, 1.0 if scale is None else np.float32(scale), np.float32)
            same = np.array_equal(_bits(got['image'][ok]), _bits(low['sample'][ok]))
            print(f'grid {grid} order {order} geometry {g} scale {scale}: worst error {ratio:.3f} x 2^-24 |s| sum|v| (bound '
                  f'{CO.C_BOUND:g}), bits of the float32 restatement: {same}')
            if order == 1:                                       # scipy itself, where every tap is inside
                sci = CO.scipy_warp_order1(frames[g], A, shape, origin) * (1.0 if scale is None else float(np.float32(scale)))
                assert np.all(np.abs(got['image'][ok] - sci[ok]) <= bound[ok]), (g, scale)
        if g == 1:                                               # an integer shift copies the pixels, bit for bit
            plain = fs.coadd([g], [A], shape, origin, order=order, combine='mean')['image']
            ys, xs = np.nonzero(np.isfinite(plain))
            assert np.array_equal(_bits(plain[ys, xs]), _bits(frames[g][ys + origin[1] - 2, xs + origin[0] + 3]))


# ---- the parity cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', CO.COMBINES)
@pytest.mark.parametrize('order', (1, 3))
@pytest.mark.parametrize('grid', range(len(CO.GRIDS)))
@pytest.mark.parametrize('n', CO.COUNTS)
def test_coadd_equals_the_restatement(fs, n, grid, order, mode):
    shape, origin = CO.GRIDS[grid]
    index, affines, g, w = CO.case_inputs(n)
    ref = CO.wanted(n, grid, order, mode)
    call = lambda rows: fs.coadd(index, affines, shape, origin, flux_scale=g, weights=w, order=order, combine=mode,
                                 n_sigma=CO.N_SIGMA, scratch_rows=rows)
    got = call(0)
    ok = ~CO.guarded(ref) if mode == 'sigma_clip' else np.ones(shape, bool)
    assert ok.mean() >= 1.0 - CO.NEAR_CAP
    assert got['count'].dtype == np.int32 and got['n_rejected'].dtype == np.int32
    assert np.array_equal(got['count'][ok], ref['count'][ok])
    assert np.array_equal(got['n_rejected'][ok], ref['n_rejected'][ok])
    assert np.array_equal(np.isnan(got['image'][ok]), np.isnan(ref['image'][ok]))
    nothing = (~np.isfinite(ref['samples'])).all(axis=0)
    assert nothing.sum() > 300 or grid == 0                     # the second grid reaches beyond every frame
    assert np.isnan(got['image'][nothing]).all() and not got['weight'][nothing].any() \
        and not got['count'][nothing].any() and not got['n_rejected'][nothing].any()
    fin = ok & np.isfinite(ref['image'])
    bound = CO.pixel_bound(ref)
    err = np.abs(got['image'][fin] - ref['image'][fin])
    m = np.isfinite(ref['samples']).sum(axis=0)
    print(f'n={n} grid={grid} order={order} {mode}: worst error / bound {(err / bound[fin]).max():.3f}, left out '
          f'{(~ok).sum()} pixels, rejected per pixel {got["n_rejected"].mean():.2f}, kernel {got["kernel_ms"]:.3f} ms')
    assert np.all(err <= bound[fin])
    assert np.all(np.abs(got['weight'][ok] - ref['weight'][ok]) <= (m[ok] + 2) * CO.EPS * ref['weight'][ok])
    # the strip height changes nothing, bit for bit
    for rows in (1, 7, shape[0]):
        other = call(rows)
        for key in ('image', 'weight', 'count', 'n_rejected'):
            assert np.array_equal(_bits(other[key]), _bits(got[key])), (rows, key)


@pytest.mark.parametrize('n', CO.LARGE_COUNTS)
def test_frame_counts_on_either_side_of_what_the_lds_holds(fs, n):
    """Up to 640 frames the combine keeps a wave's samples in LDS, beyond it reads the scratch: the last count of the one
    form and the first of the other, same arithmetic, same bounds."""
    shape, origin = CO.GRIDS[1]
    index, affines, g, w = CO.case_inputs(n)
    ref = CO.coadd(CO.frames(), index, affines, shape, origin, g, w, 3, 'sigma_clip', CO.LARGE_N_SIGMA, np.float64)
    got = fs.coadd(index, affines, shape, origin, flux_scale=g, weights=w, order=3, combine='sigma_clip',
                   n_sigma=CO.LARGE_N_SIGMA)
    ok = ~CO.guarded(ref)
    assert ok.mean() >= 1.0 - CO.NEAR_CAP and ref['n_rejected'].any()
    assert np.array_equal(got['count'][ok], ref['count'][ok]) and np.array_equal(got['n_rejected'][ok], ref['n_rejected'][ok])
    assert np.array_equal(np.isnan(got['image'][ok]), np.isnan(ref['image'][ok]))
    fin = ok & np.isfinite(ref['image'])
    err = np.abs(got['image'][fin] - ref['image'][fin])
    print(f'n={n}: worst error / bound {(err / CO.pixel_bound(ref)[fin]).max():.3f}, left out {(~ok).sum()} pixels, kernel '
          f'{got["kernel_ms"]:.3f} ms')
    assert np.all(err <= CO.pixel_bound(ref)[fin])
    med = fs.coadd(index, affines, shape, origin, flux_scale=g, weights=w, order=3, combine='median')
    med64 = CO.combine(ref['samples'], w, 'median')
    fin = np.isfinite(med64['image'])
    assert np.array_equal(np.isnan(med['image']), ~fin) and np.array_equal(med['count'], med64['count'])
    assert np.all(np.abs(med['image'][fin] - med64['image'][fin]) <= CO.pixel_bound(ref)[fin])
    other = fs.coadd(index, affines, shape, origin, flux_scale=g, weights=w, order=3, combine='sigma_clip',
                     n_sigma=CO.LARGE_N_SIGMA, scratch_rows=7)
    for key in ('image', 'weight', 'count', 'n_rejected'):
        assert np.array_equal(_bits(other[key]), _bits(got[key])), key


def test_a_frame_contributes_the_same_whatever_shares_the_call(fs):
    """With the weight 1 for one slot and 0 for the others the weighted mean is that slot's sample, bit for bit (1 v + 0
    = v; the pedestal keeps every sample away from -0), wherever it has one."""
    n = 67
    index, affines, g, _ = CO.case_inputs(n)
    shape, origin = CO.GRIDS[1]
    for order in (1, 3):
        for slot in (0, 3, 29, 66):
            alone = fs.coadd(index[slot:slot + 1], affines[slot:slot + 1], shape, origin, flux_scale=g[slot:slot + 1],
                             order=order, combine='mean')
            w = np.zeros(n, np.float32)
            w[slot] = 1.0
            shared = fs.coadd(index, affines, shape, origin, flux_scale=g, weights=w, order=order, combine='mean')
            there = np.isfinite(alone['image'])
            assert there.any() and not (alone['image'][there] == 0).any()
            assert np.array_equal(_bits(shared['image'][there]), _bits(alone['image'][there])), (order, slot)
            assert np.isnan(shared['image'][~there]).all()
            assert np.array_equal(shared['weight'], there.astype(np.float32))
            assert (shared['count'] >= alone['count']).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(fs, ctx):
    from lightcurver_amd import _lib
    lib = _lib.lib()
    H, W = 6, 5
    A = np.array([[1.0, 0.0, 2.0, 0.0, 1.0, 3.0]] * 2)
    base = dict(f=fs.h, n=2, frame=np.array([0, 1], np.int32), affine=A, scale=np.ones(2, np.float32),
                weight=np.ones(2, np.float32), H=H, W=W, cfg=_lib.CoaddCfg(3, 2, 3.0, 0))

    def call(outputs=True, **kw):
        a = {**base, **kw}
        out = [np.full((a['H'] if 0 < a['H'] < 100 else H, a['W'] if 0 < a['W'] < 100 else W), 7, t)
               for t in (np.float32, np.float32, np.int32, np.int32)]
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        rc = lib.lc_frames_coadd(a['f'], a['n'], ptr(a['frame'], _ip), ptr(a['affine'], _lib.dp), ptr(a['scale'], _lib.fp),
                                 ptr(a['weight'], _lib.fp), a['H'], a['W'], 0, 0, None if a['cfg'] is None else C.byref(a['cfg']),
                                 ptr(out[0], _lib.fp), ptr(out[1], _lib.fp) if outputs else None,
                                 ptr(out[2], _ip) if outputs else None, ptr(out[3], _ip) if outputs else None, None)
        return rc, out

    def bad_affine(i, v):
        B = A.copy()
        B[1, i] = v
        return B

    refused = dict(
        n_zero=dict(n=0), n_negative=dict(n=-1), frame_low=dict(frame=np.array([0, -1], np.int32)),
        frame_high=dict(frame=np.array([CO.K_SET, 0], np.int32)), affine_nan=dict(affine=bad_affine(2, np.nan)),
        affine_inf=dict(affine=bad_affine(0, np.inf)), det_zero=dict(affine=np.array([[1.0, 2.0, 0.0, 2.0, 4.0, 0.0]] * 2)),
        scale_nan=dict(scale=np.array([1.0, np.nan], np.float32)), scale_inf=dict(scale=np.array([np.inf, 1.0], np.float32)),
        weight_negative=dict(weight=np.array([1.0, -0.5], np.float32)), weight_nan=dict(weight=np.array([np.nan, 1.0], np.float32)),
        weight_inf=dict(weight=np.array([1.0, np.inf], np.float32)), H_zero=dict(H=0), W_zero=dict(W=0), H_negative=dict(H=-3),
        too_large=dict(H=65536, W=32768), order_2=dict(cfg=_lib.CoaddCfg(2, 2, 3.0, 0)), order_0=dict(cfg=_lib.CoaddCfg(0, 2, 3.0, 0)),
        combine_3=dict(cfg=_lib.CoaddCfg(3, 3, 3.0, 0)), combine_negative=dict(cfg=_lib.CoaddCfg(3, -1, 3.0, 0)),
        n_sigma_zero=dict(cfg=_lib.CoaddCfg(3, 2, 0.0, 0)), n_sigma_negative=dict(cfg=_lib.CoaddCfg(3, 0, -1.0, 0)),
        n_sigma_nan=dict(cfg=_lib.CoaddCfg(3, 1, float('nan'), 0)), n_sigma_inf=dict(cfg=_lib.CoaddCfg(3, 2, float('inf'), 0)),
        rows_negative=dict(cfg=_lib.CoaddCfg(3, 2, 3.0, -1)), no_cfg=dict(cfg=None), no_frame=dict(frame=None),
        no_affine=dict(affine=None))
    before = fs.planes()
    for name, kw in refused.items():
        rc, out = call(**kw)
        assert rc == -1, name                                                     # LC_ERR_INVALID
        assert all((o == 7).all() for o in out), name
        assert lib.lc_last_error(ctx.h), name
    assert call(f=None)[0] == -1
    # the set is as usable as before; null optional outputs, scales and weights work
    rc, full = call()
    assert rc == 0 and not any((o == 7).all() for o in full[:1])
    rc, bare = call(outputs=False, scale=None, weight=None)
    assert rc == 0 and np.array_equal(_bits(bare[0]), _bits(full[0])) and all((o == 7).all() for o in bare[1:])
    assert np.array_equal(_bits(fs.planes()), _bits(before))
    # FrameSet.coadd refuses what it can name
    with pytest.raises(ValueError, match='combine'):
        fs.coadd([0], [np.eye(3)], combine='sum')
    with pytest.raises(ValueError, match='transforms'):
        fs.coadd([0, 1], [np.eye(3)])
    with pytest.raises(ValueError, match='frame index'):
        fs.coadd([CO.K_SET], [np.eye(3)])
    with pytest.raises(_lib.LcError):
        fs.coadd([0], [np.eye(3)], order=2)


def test_transform_forms_are_the_same_call(fs):
    from lightcurver_amd.astroalign import SimilarityTransform
    A = CO.affine_of(CO.GEOMETRIES[4])
    full = np.vstack([A, [0.0, 0.0, 1.0]])
    a = fs.coadd([2, 5], [A, A], order=3, combine='median')
    b = fs.coadd([2, 5], [full, SimilarityTransform(full)], order=3, combine='median')
    c = fs.coadd(np.array([2, 5]), np.stack([A, A]), order=3, combine='median')
    for key in ('image', 'weight', 'count', 'n_rejected'):
        assert np.array_equal(_bits(a[key]), _bits(b[key])) and np.array_equal(_bits(a[key]), _bits(c[key]))
    assert a['image'].shape == CO.FRAME_SHAPE


# ---- what the co-add is for ----------------------------------------------------------------------------------------------------
def test_a_cosmic_ray_hit_is_rejected(ctx):
    """A single-pixel hit of 50 sigma in one of 12 frames: gone from the median co-add and from the sigma_clip co-add at
    n_sigma = 2.5, where exactly that sample is rejected (it lies about 12 / sqrt(11) = 3.6 deviations from the median),
    present in the mean co-add (50 / 12 = 4.2 sigma above the pedestal; the noise of a mean of 12 is 0.29)."""
    from lightcurver_amd.frames import FrameSet
    rng = np.random.default_rng(21)
    n, h, w, pedestal = 12, 32, 36, 100.0
    frames = (pedestal + rng.standard_normal((n, h, w))).astype(np.float32)
    shifts = [(k % 4 - 1, k % 3 - 1) for k in range(n)]                         # integer: the hit stays one output pixel
    hit_frame, (hy, hx) = 7, (15, 20)
    sx, sy = shifts[hit_frame]
    frames[hit_frame, hy + sy, hx + sx] = pedestal + 50.0
    affines = [np.array([[1.0, 0.0, sx], [0.0, 1.0, sy]]) for sx, sy in shifts]
    with FrameSet(frames, ctx) as s:
        out = {mode: s.coadd(np.arange(n), affines, combine=mode, n_sigma=2.5) for mode in CO.COMBINES}
    for mode in CO.COMBINES:
        assert out[mode]['count'][hy, hx] + out[mode]['n_rejected'][hy, hx] == n
    print({mode: float(out[mode]['image'][hy, hx]) - pedestal for mode in CO.COMBINES})
    assert abs(out['median']['image'][hy, hx] - pedestal) < 1.5
    assert abs(out['sigma_clip']['image'][hy, hx] - pedestal) < 1.5
    assert out['sigma_clip']['n_rejected'][hy, hx] == 1 and out['sigma_clip']['count'][hy, hx] == n - 1
    assert out['mean']['image'][hy, hx] - pedestal > 3.0 and out['mean']['n_rejected'][hy, hx] == 0
    assert out['median']['n_rejected'][hy, hx] == 0


# ---- an imported set ---------------------------------------------------------------------------------------------------------
def test_imported_set_and_its_default_weights(ctx):
    """On the sky-subtracted planes of an imported set, against the restatement run on those planes; weights=None is then
    1 / (s rms)^2 with the recorded globalrms; the planes are left as they were."""
    from lightcurver_amd.frames import FrameSet
    from tests import _frames_scene as S
    sc = S.scene()
    take = np.array([0, 1, 2, 3, 5], np.int32)
    T = sc['truth']['transforms'][take]
    g = np.array([1.0, 1.3, 0.8, 1.1, 1.6], np.float32)
    with FrameSet(sc['frames'][:6], ctx) as s:
        assert not s.imported
        raw = s.coadd(take, T, combine='mean', order=1)                          # a raw set: weights default to 1
        assert np.array_equal(raw['weight'], raw['count'].astype(np.float32))
        imported = s.import_frames(sc['exptimes'][:6].astype(np.float32))
        assert s.imported
        planes = s.planes()
        rms = np.asarray(imported['globalrms'], np.float64)[take]
        det = np.abs(T[:, 0, 0] * T[:, 1, 1] - T[:, 0, 1] * T[:, 1, 0])
        weights = (1.0 / (g.astype(np.float64) * det * rms) ** 2).astype(np.float32)
        for order, mode in ((3, 'sigma_clip'), (1, 'median'), (3, 'mean')):
            got = s.coadd(take, T, flux_scale=g, order=order, combine=mode, n_sigma=1.2)
            explicit = s.coadd(take, T, flux_scale=g, weights=weights, order=order, combine=mode, n_sigma=1.2)
            for key in ('image', 'weight', 'count', 'n_rejected'):
                assert np.array_equal(_bits(got[key]), _bits(explicit[key])), (mode, key)
            ref = CO.coadd(planes, take, T, S.SHAPE, (0, 0), g, weights, order, mode, 1.2, np.float64)
            ok = ~CO.guarded(ref) if mode == 'sigma_clip' else np.ones(S.SHAPE, bool)
            assert ok.mean() >= 1.0 - CO.NEAR_CAP
            assert np.array_equal(got['count'][ok], ref['count'][ok]) and np.array_equal(got['n_rejected'][ok], ref['n_rejected'][ok])
            assert np.array_equal(np.isnan(got['image'][ok]), np.isnan(ref['image'][ok]))
            fin = ok & np.isfinite(ref['image'])
            assert fin.mean() > 0.9 and (mode != 'sigma_clip' or got['n_rejected'].any())
            assert np.all(np.abs(got['image'][fin] - ref['image'][fin]) <= CO.pixel_bound(ref)[fin])
        assert np.array_equal(_bits(s.planes()), _bits(planes))
