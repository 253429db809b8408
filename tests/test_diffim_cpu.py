"""The restatement of the difference-imaging SPEC (tests/_diffim.py; DESIGN.md §5 "Difference imaging") against closed
forms, and the parts of the feature that need no device: prototypes and the argument checks of the Python layer."""
import ctypes as C

import numpy as np
import pytest

from tests import _diffim as DI


def test_restatement_recovers_a_known_kernel():
    """Noise-free T = R (*) K_true + plane: both float64 solutions return the kernel, its sum and the plane."""
    s = DI.known_kernel_scene()
    out = DI.subtract(s['T'], s['R'], r=2, bg_degree=1, clip_iters=0)
    assert out['status'][0] == 0 and out['n_used'][0] == (48 - 4) * (40 - 4)
    f = out['fits'][0]
    gap = np.abs(f['x'] - f['x_lstsq']).max()
    err = np.abs(out['kernel'][0] - s['K']).max()
    print(f'kernel error {err:.3e}, Cholesky against lstsq {gap:.3e}, scale {out["scale"][0]:.9f}, plane {out["bg"][0, :3]}, '
          f'max |D| {np.nanmax(np.abs(out["diff64"])):.3e}')
    # T is rounded to float32 (2^-24 of up to 2000 counts per pixel), which the fit averages over ~2000 pixels
    assert err < 1e-5 and np.abs(f['x_lstsq'][:25].reshape(5, 5) - s['K']).max() < 1e-5
    assert abs(out['scale'][0] - 0.8) < 1e-5
    assert np.allclose(out['bg'][0], [3.0, 1.5, -0.7, 0, 0, 0], atol=1e-3)
    assert np.nanmax(np.abs(out['diff64'])) < 2000 * 2.0 ** -23
    assert np.isnan(out['diff64'][:2]).all() and np.isnan(out['diff64'][:, -2:]).all() and np.isfinite(out['diff64'][2:-2, 2:-2]).all()


def test_model_is_scipys_convolution():
    from scipy import signal
    s = DI.known_kernel_scene()
    R = s['R'].astype(np.float64)
    rng = np.random.default_rng(3)
    K = rng.standard_normal((5, 5))
    want = signal.convolve2d(R, K, mode='same')
    assert np.allclose(DI.convolve_same(R, K), want, rtol=0, atol=1e-9)
    x = np.concatenate([K.reshape(-1), [0.0]])
    D, _ = DI.difference(np.zeros_like(s['R']), s['R'], 2, 0, (0, 48, 0, 40), x, np.float64)
    assert np.allclose(-D[2:-2, 2:-2], want[2:-2, 2:-2], rtol=0, atol=1e-9)
    rows, cols = np.nonzero(DI.footprint_finite(s['R'], 2))
    A = DI.design(s['R'], 2, 0, (0, 48, 0, 40), rows, cols)
    assert np.allclose(A @ x, want[rows, cols], rtol=0, atol=1e-9)


def test_fit_set_obeys_every_exclusion_rule():
    s = DI.known_kernel_scene()
    T, R = s['T'].copy(), s['R'].copy()
    H, W = T.shape
    r = 2
    full = DI.base_set(T, R, r)
    assert full.sum() == (H - 2 * r) * (W - 2 * r) and not full[:r].any() and not full[:, W - r:].any()
    R[20, 17] = np.nan
    gone = full & ~DI.base_set(T, R, r)
    assert gone.sum() == (2 * r + 1) ** 2 and gone[18:23, 15:20].all()
    T[30, 30] = np.inf
    var = np.ones((H, W), np.float32)
    var[10, 10], var[11, 10], var[12, 10] = 0.0, np.nan, -1.0
    mask = np.zeros((H, W), np.uint8)
    mask[40, 5] = 7
    now = DI.base_set(T, R, r, var, mask)
    assert (full & ~now).sum() == 25 + 1 + 3 + 1
    out = DI.subtract(T, R, r=r, clip_iters=0, var=var, mask=mask)
    assert out['n_used'][0] == now.sum()
    # D is computed at masked pixels and where the variance is bad, not where T or the footprint is not finite
    assert np.isfinite(out['diff64'][40, 5]) and np.isfinite(out['diff64'][10, 10])
    assert np.isnan(out['diff64'][30, 30]) and np.isnan(out['diff64'][18:23, 15:20]).all()
    assert np.array_equal(np.isnan(out['diff64']), np.isnan(out['diff32']))


@pytest.mark.parametrize('name', ['var_clip', 'sigma_clip', 'rms_clip'])
def test_a_clipping_round_removes_exactly_the_injected_outliers(name):
    c, want = DI.case(name), DI.wanted(name)
    for k, out in enumerate(want):
        first = DI.subtract(c['T'][k], c['R'], var=None if c['var'] is None else c['var'][k],
                            mask=None if c['mask'] is None else c['mask'][k],
                            sigma=None if c['sigma'] is None else c['sigma'][k], **{**c['settings'], 'clip_iters': 0})
        clipped = first['used'] & ~out['used']
        n_out = 1 if name == 'rms_clip' else 3
        print(name, k, 'clipped', clipped.sum(), 'margins (round, region, worst kept, least clipped):', out['margins'])
        assert 1 <= clipped.sum() <= n_out and first['n_used'][0] - out['n_used'][0] == clipped.sum()
        assert np.all(np.abs(out['diff64'][clipped]) > 50.0)          # the outliers stay in D
        assert len(out['margins']) == 2 and out['status'][0] == 0


def test_status_rules():
    out = DI.wanted('regions_fail')[0]
    P = 49 + 6
    print('status', out['status'], 'n_used', out['n_used'])
    assert out['status'][0] == DI.STATUS_FEW and out['n_used'][0] < 2 * P
    assert out['status'][5] == DI.STATUS_PIVOT
    assert (out['status'][1:5] == 0).all()
    regs = DI.regions_of((40, 48), (2, 3))
    for g in (0, 5):
        i0, i1, j0, j1 = regs[g]
        assert np.isnan(out['diff64'][i0:i1, j0:j1]).all() and np.isnan(out['kernel'][g]).all() and np.isnan(out['chi2'][g])
    assert np.isfinite(out['diff64'][3:20, 16:32]).all()


def test_float32_order_against_float64():
    """The float32 restatement of D against the float64 one over every case: the worst ratio to 2^-24 (sum |K_m| |R| +
    |bg| + |T|), and the bound's factor C_BOUND: the next power of two >= 4 x it."""
    worst = 0.0
    for name in DI.CASES:
        for out in DI.wanted(name):
            ok = np.isfinite(out['diff64'])
            assert np.array_equal(ok, np.isfinite(out['diff32']))
            ratio = np.abs(out['diff32'][ok] - out['diff64'][ok]) / (2.0 ** -24 * out['magnitude'][ok])
            worst = max(worst, float(ratio.max()))
    c = 2.0 ** np.ceil(np.log2(4.0 * worst))
    print(f'worst float32 / float64 ratio {worst:.3f} x 2^-24 magnitude; next power of two >= 4 x it: {c:g}')
    assert c == DI.C_BOUND


def test_gram_of_the_restatement_is_within_the_summation_bound():
    out = DI.wanted('plain')[0]
    f = out['fits'][0]
    U, b, Ua, ba = DI.gram(f['A'], f['w'], f['t'])
    assert np.all(np.abs(f['U'] - U) <= (f['n'] + 4) * 2.0 ** -53 * Ua)
    assert np.all(np.abs(f['b'] - b) <= (f['n'] + 4) * 2.0 ** -53 * ba)


def test_prototypes_are_declared():
    from lightcurver_amd import _lib
    for name in ('lc_diffim_supported', 'lc_diffim_frames', 'lc_frames_subtract_reference'):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['lc_diffim_frames'][1]) == 12
    assert len(_lib.SIGNATURES['lc_frames_subtract_reference'][1]) == 16
    assert C.sizeof(_lib.DiffimCfg) == 24 and C.sizeof(_lib.DiffimOut) == 10 * C.sizeof(C.c_void_p)
    header = open(__import__('os').path.join(__import__('os').path.dirname(_lib._HERE), 'include', 'lcmi.h')).read()
    for name in ('lc_diffim_supported', 'lc_diffim_frames', 'lc_frames_subtract_reference', 'lc_diffim_cfg', 'lc_diffim_out'):
        assert name in header


def test_python_checks_come_before_the_library(monkeypatch):
    from lightcurver_amd import _lib
    from lightcurver_amd.processes import difference_imaging as di

    def no_library(*args, **kw):
        raise AssertionError('the library was touched')

    monkeypatch.setattr(_lib, 'lib', no_library)
    monkeypatch.setattr(_lib, 'default_context', no_library)
    img, ref = np.zeros((2, 20, 24), np.float32), np.zeros((20, 24), np.float32)
    for kw, match in ((dict(r=0), 'r must'), (dict(r=8), 'r must'), (dict(bg_degree=3), 'bg_degree'),
                      (dict(regions=(0, 1)), 'regions'), (dict(regions=(9, 8)), 'regions'), (dict(regions=3), 'regions'),
                      (dict(clip_iters=-1), 'clip_iters'), (dict(n_sigma=0.0), 'n_sigma'), (dict(n_sigma=np.nan), 'n_sigma'),
                      (dict(sigma=[1.0, -1.0]), 'sigma'), (dict(sigma=np.inf), 'sigma'), (dict(download=('image',)), 'download'),
                      (dict(download=()), 'download'), (dict(variance=np.ones((20, 24))), 'variance'),
                      (dict(mask=np.zeros((2, 20, 23))), 'mask'), (dict(r=7, regions=(1, 1)), 'images of')):
        with pytest.raises(ValueError, match=match):
            di.match_and_subtract(img[:, :14, :14] if kw.get('r') == 7 else img, ref[:14, :14] if kw.get('r') == 7 else ref, **kw)
    with pytest.raises(ValueError, match='reference'):
        di.match_and_subtract(img, ref[:-1])
    with pytest.raises(ValueError, match='expected'):
        di.match_and_subtract(np.zeros(5), ref)
    with pytest.raises(ValueError, match='no registered frame'):
        di.difference_frames(None, [dict(success=False)], ref)
    two = [dict(success=True, transform=np.eye(3)), dict(success=False)]
    with pytest.raises(ValueError, match='sigma must be'):
        di.difference_frames(None, two, ref, sigma=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match='mask must be'):
        di.difference_frames(None, two, ref, mask=np.zeros((1, 20, 24)))
    with pytest.raises(ValueError, match='scales per frame'):
        di.difference_light_curves(img, np.ones((2, 4)), [[3.0, 3.0]], 2.0)


def test_physics_scene_passes_with_the_restatement_alone():
    """What tests/test_diffim_gpu.py asks of the device on the physics scene, with the restatement: the aperture sums of
    D / scale give delta at the variable and 0 at the constant stars within 5 sigma sqrt(pi r^2) / scale, and the pixel
    hit is clipped from the fit and present in D."""
    p, s = DI.PHYS, DI.physics_scene()
    for k in range(p['n_frames']):
        out = DI.subtract(s['T'][k], s['R'], r=p['r'], bg_degree=1, clip_iters=2, n_sigma=4.0, sigma=p['sigma'])
        scale = out['scale'][0]
        tol = 5.0 * p['sigma'] * np.sqrt(np.pi * p['aperture'] ** 2) / scale
        flux = np.array([DI.aperture_sum_subsampled(out['diff64'], x, y, p['aperture']) / scale for x, y in s['xy']])
        want = np.zeros(len(flux))
        want[p['variable']] = p['delta']
        print(k, 'scale', scale, 'tolerance', tol, 'flux - wanted', np.round(flux - want, 1))
        assert abs(scale - 0.7) < 0.01 and np.all(np.abs(flux - want) < tol)
        assert not out['used'][p['hit_at']] and out['diff64'][p['hit_at']] > 40.0 * p['sigma']
