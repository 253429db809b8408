"""The PSF fit at subsampling 1 above the 16 x 16 fixture size: the kernels of n = 32 (one-wave layout, 8 pixels per thread
kept in registers) and n = 64 (block-synchronised layout, pixel state in global memory: DESIGN.md section 5) against the float64
oracle, with the checks and the bounds tests/test_psf_gpu.py and tests/test_psf_geometry_gpu.py apply at subsampling 2; and
``build_psf`` through the facade at 32 (native), 24 (embedded in 32) and with the field-distortion fit.

Bounds: 2e-5 on model / loss / noise maps, 5e-5 on star and grid gradients, 1e-4 on the Moffat gradient and on the loss
history of a trajectory; moved pixels as explained in tests/test_psf_gpu.py."""
import os

import numpy as np
import pytest

from oracle import model as om, optim as oo
from lightcurver_amd.synthetic import make_psf_dataset
from tests import helpers as H
from tests import _psf_geometry as G
from tests import _distortion as D

pytestmark = pytest.mark.gpu

CASES = [(32, 1, 8), (32, 1, 3), (64, 1, 3)]   # 8 fills a group of stars, 3 leaves it ragged


def _batch(ds, plist, ss, ctx):
    from lightcurver_amd.psf_batch import PsfBatch
    b = PsfBatch(ds['data'], H.weights_from(ds), ss, ctx)
    b.set_moffat(H.moffat_array(plist))
    b.set_stars(H.stars_array(plist))
    b.set_grid(np.stack([p['B'].numpy() for p in plist]))
    return b


def _setup(n, ss, F, S, seed, ctx, jitter=0.3):
    ds = make_psf_dataset(F=F, S=S, n=n, ss=ss, seed=seed)
    rng = np.random.default_rng(seed + 1)
    plist = [H.psf_initial_params(ds, f, ss, rng, jitter) for f in range(F)]
    return ds, plist, _batch(ds, plist, ss, ctx)


def _oracle_weights(ds, plist, ss):
    return [om.propagate_noise_psf(plist[f], *H.psf_oracle_inputs(ds, f, ss)[1:], ss) for f in range(len(plist))]


def _check_eval(ds, plist, b, n, ss, tag, lam_scales=1.3, lam_hf=0.7, ring=False):
    """tests/test_psf_gpu.py::test_eval_matches_oracle's figures, printed before they are judged; ring: also dL/dB on its
    outer 8 pixels against the largest element there and the model per star (tests/test_psf_geometry_gpu.py)."""
    N = n * ss
    J = om.n_scales(N)
    Ws = _oracle_weights(ds, plist, ss)
    b.set_regularization(np.stack([w[:J].numpy() for w in Ws]), lam_scales=lam_scales, lam_hf=lam_hf)
    out = b.evaluate(model=True)
    free = ['fwhm_x', 'fwhm_y', 'phi', 'beta', 'a', 'x0', 'y0', 'sky', 'B']
    for f in range(len(plist)):
        data, sig2, mask = H.psf_oracle_inputs(ds, f, ss)
        fn = lambda q: om.psf_loss(q, data, sig2, mask, ss, W=Ws[f], lam_scales=lam_scales, lam_hf=lam_hf)
        L, g = oo.value_and_grad(fn, plist[f], free)
        model = om.psf_model(plist[f], ss, n).numpy()
        gs = np.stack([g['a'].numpy(), g['x0'].numpy(), g['y0'].numpy(), g['sky'].numpy()], axis=-1)
        gB = g['B'].numpy().reshape(N, N)
        gm = np.array([float(g[k]) for k in ['fwhm_x', 'fwhm_y', 'phi', 'beta']])
        fig = dict(model=H.rel_err(out['model'][f], model), loss=abs(out['loss'][f] - L) / abs(L),
                   stars=max(H.rel_err(out['grad_stars'][f][:, q], gs[:, q]) for q in range(4)),
                   grid=H.rel_err(out['grad_grid'][f], gB), moffat=H.rel_err(out['grad_moffat'][f], gm),
                   ring=G.ring_err(out['grad_grid'][f], gB), model_per_star=G.per_star_model_err(out['model'][f], model).max())
        print(tag, 'frame', f, {k: '%.2e' % v for k, v in fig.items()})
        assert fig['model'] < 2e-5 and fig['loss'] < 2e-5
        assert fig['stars'] < 5e-5 and fig['grid'] < 5e-5
        assert fig['moffat'] < 1e-4
        if ring:
            assert fig['ring'] < 5e-5 and fig['model_per_star'] < 2e-5


@pytest.mark.parametrize('n,ss,S', CASES)
def test_eval_matches_oracle(ctx, n, ss, S):
    ds, plist, b = _setup(n, ss, 2, S, 11 + n + ss, ctx)
    _check_eval(ds, plist, b, n, ss, f'eval n={n} ss={ss} S={S}')
    b.close()


@pytest.mark.parametrize('n,ss,S', CASES)
def test_noise_propagation_matches_oracle(ctx, n, ss, S):
    """Device tables, the host form (LCMI_NOISE_HOST=1) and a frame with a zero-weight padding star."""
    from lightcurver_amd.psf_batch import PsfBatch
    F = 2
    ds, plist, b = _setup(n, ss, F, S, 21 + n, ctx)
    b.propagate_noise()
    W = b.get_weights()
    J = om.n_scales(n * ss)
    Wo = np.stack([w[:J].numpy() for w in _oracle_weights(ds, plist, ss)])
    for f in range(F):
        print(f'noise n={n} S={S} frame {f}: {H.rel_err(W[f], Wo[f]):.2e}')
        assert H.rel_err(W[f], Wo[f]) < 2e-5
    os.environ['LCMI_NOISE_HOST'] = '1'
    try:
        b.propagate_noise()
    finally:
        os.environ.pop('LCMI_NOISE_HOST', None)
    assert H.rel_err(W, b.get_weights()) < 2e-5
    b.close()
    w = H.weights_from(ds)
    stars = H.stars_array(plist)
    b2 = PsfBatch(np.concatenate([ds['data'], np.zeros_like(ds['data'][:, :1])], axis=1),
                  np.concatenate([w, np.zeros_like(w[:, :1])], axis=1), ss, ctx)
    b2.set_moffat(H.moffat_array(plist))
    b2.set_stars(np.concatenate([stars, np.zeros_like(stars[:, :1])], axis=1))
    b2.propagate_noise()
    assert H.rel_err(b2.get_weights(), W) < 1e-6
    b2.close()


@pytest.mark.parametrize('n,ss,S', [(32, 1, 8), (64, 1, 3)])
def test_adabelief_trajectory_matches_oracle(ctx, n, ss, S):
    F, T = 2, 25
    ds, plist, b = _setup(n, ss, F, S, 5 + n, ctx, jitter=0.1)
    J = om.n_scales(n * ss)
    Ws = _oracle_weights(ds, plist, ss)
    b.set_regularization(np.stack([w[:J].numpy() for w in Ws]), lam_scales=1.0, lam_hf=1.0)
    b.run_adabelief(T, init_learning_rate=1e-4, schedule_learning_rate=True)
    hist, stars, grid = b.loss_history(), b.get_stars(), b.get_grid()
    b.close()
    assert hist.shape == (F, T + 1)
    for f in range(F):
        data, sig2, mask = H.psf_oracle_inputs(ds, f, ss)
        fn = lambda q: om.psf_loss(q, data, sig2, mask, ss, W=Ws[f], lam_scales=1.0, lam_hf=1.0)
        pf, lh, l0 = oo.adabelief(fn, plist[f], ['B', 'a', 'x0', 'y0'], 1e-4, T, schedule=True)
        ref = np.array([l0] + lh)
        dB = np.abs(grid[f].ravel() - pf['B'].numpy())
        fig = dict(hist=np.abs(hist[f] - ref).max() / np.abs(ref).max(), dBmax=dB.max(), dBmed=np.median(dB),
                   moved=(dB > 1e-6).mean(), a=H.rel_err(stars[f][:, 0], pf['a'].numpy()),
                   x0=np.abs(stars[f][:, 1] - pf['x0'].numpy()).max())
        print(f'trajectory n={n} frame {f}', {k: '%.2e' % v for k, v in fig.items()})
        assert fig['hist'] < 1e-4
        assert fig['dBmax'] < 0.02 * T * 1e-4 and fig['dBmed'] < 1e-7 and fig['moved'] < 0.01
        assert fig['a'] < 1e-5 and fig['x0'] < 2e-5


@pytest.mark.parametrize('n', [32, 64])
def test_eval_next_to_the_offset_limit_matches_oracle(ctx, n):
    """Stars at +-(n/4 - 0.01) data pixels (corners, edges and the tie pairs of tests/_psf_geometry.py, clipped): the window
    bases, aprons (n = 32) and clamped reads (n = 64) at the largest offsets the fit can reach.  The global bounds, and dL/dB
    on its border ring and the model per star as tests/test_psf_geometry_gpu.py judges them."""
    ss, S, F = 1, 8, 2
    lim = n / 4.0
    xy = np.clip(G.offsets_for(n, ss, S, F), -(lim - 0.01), lim - 0.01)
    ds = G.draw_dataset(n, ss, G.displaced(xy, 431 + n), 430 + n)
    plist = G.params_at(ds, xy, 432 + n)
    b = _batch(ds, plist, ss, ctx)
    _check_eval(ds, plist, b, n, ss, f'limit n={n}', ring=True)
    b.close()


# ---- build_psf ---------------------------------------------------------------------------------------------------------------
KW = dict(n_iter_analytic=20, n_iter_adabelief=50, guess_method_star_position='center')


def _check_result(r, S, n, ss):
    N = n * ss
    for key in ('full_psf', 'adabelief_extra_fields', 'narrow_psf', 'chi2', 'residuals', 'kwargs_psf'):
        assert key in r
    assert len(r['adabelief_extra_fields']['loss_history']) == 50
    assert np.all(np.isfinite(r['adabelief_extra_fields']['loss_history']))
    assert r['residuals'].shape == (S, n, n) and r['narrow_psf'].shape == (N, N) and r['full_psf'].shape == (N, N)
    assert abs(r['narrow_psf'].sum() - 1) < 1e-5 and abs(r['full_psf'].sum() - 1) < 1e-5
    assert np.isfinite(r['chi2'])
    km = r['kwargs_psf']['kwargs_moffat']
    assert np.isfinite(float(np.asarray(0.5 * (km['fwhm_x'] + km['fwhm_y'])).item()))
    assert np.asarray(r['kwargs_psf']['kwargs_background']['background']).shape == (N * N,)
    assert isinstance(r['kwargs_psf']['kwargs_distortion'], dict)


def test_build_psf_at_32(ctx):
    from lightcurver_amd.starred.procedures.psf_routines import build_psf, _fit_size
    n, ss, S = 32, 1, 5
    assert _fit_size(n, ss) == n
    ds = make_psf_dataset(F=1, S=S, n=n, ss=ss, seed=61)
    r = build_psf(ds['data'][0].astype(np.float64), ds['noisemap'][0].astype(np.float64), ss,
                  masks=ds['masks'][0].astype(np.float64), guess_fwhm_pixels=float(ds['fwhm_guess'][0]), **KW)
    _check_result(r, S, n, ss)
    lh = r['adabelief_extra_fields']['loss_history']
    assert lh[-1] < lh[0]


def test_build_psf_at_24_is_the_fit_at_32_of_the_padded_problem(ctx):
    """n = 24 has no kernel at subsampling 1: embedded in 32, bit for bit the n = 32 fit of the centrally padded stamps
    (no weight on the ring), cut back and renormalised."""
    from lightcurver_amd.starred.procedures.psf_routines import build_psf_batch, _fit_size
    ss, F, S, n, m = 1, 2, 4, 24, 32
    assert _fit_size(n, ss) == m
    pad = (m - n) // 2
    ds = make_psf_dataset(F=F, S=S, n=n, ss=ss, seed=5)
    kw = dict(KW, guess_fwhm_pixels=ds['fwhm_guess'])
    res = build_psf_batch(list(ds['data']), list(ds['noisemap']), ss, masks=list(ds['masks']), **kw)
    big = lambda a, fill: np.pad(np.asarray(a, np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad)), constant_values=fill)
    ref = build_psf_batch(list(big(ds['data'], 0.0)), list(big(ds['noisemap'], 1.0)), ss, masks=list(big(ds['masks'], 0.0)), **kw)
    P, N = pad * ss, n * ss
    for f in range(F):
        _check_result(res[f], S, n, ss)
        cut = ref[f]['narrow_psf'][P:P + N, P:P + N]
        assert np.array_equal(res[f]['narrow_psf'], cut / cut.sum())
        assert np.array_equal(res[f]['residuals'], ref[f]['residuals'][:, pad:pad + n, pad:pad + n])
        assert res[f]['chi2'] == ref[f]['chi2']
        assert np.array_equal(res[f]['kwargs_psf']['kwargs_gaussian']['x0'], ref[f]['kwargs_psf']['kwargs_gaussian']['x0'])
        assert res[f]['adabelief_extra_fields']['loss_history'] == ref[f]['adabelief_extra_fields']['loss_history']


def test_build_psf_with_field_distortion_at_32(ctx):
    """field_distortion=True at n = 32, ss = 1 runs, returns the coefficient layout of the reference, and the PSF resamples
    at a stamp position.  Coefficients and positions: a corner case of the matrix set of tests/_distortion.py, scaled to a
    tenth (a field distortion a fit meets)."""
    from lightcurver_amd.starred.procedures.psf_routines import build_psf
    from lightcurver_amd.starred.psf.psf import apply_distortion
    S, n, ss = 8, 32, 1
    N = n * ss
    name, coef, pos = D.CORNERS[0]
    true, xy = 0.1 * coef, pos[:S]
    rng = np.random.default_rng(79)
    p = dict(fwhm_x=om.T(3.2), fwhm_y=om.T(3.0), phi=om.T(0.3), beta=om.T(3.0), B=om.T(np.zeros(N * N)),
             a=om.T(rng.uniform(2e5, 6e5, S)), x0=om.T(rng.uniform(-0.4, 0.4, S)), y0=om.T(rng.uniform(-0.4, 0.4, S)),
             sky=om.T(np.zeros(S)), dist=om.T(true))
    clean = om.psf_model_distorted(p, xy, ss, n).numpy()
    noise = np.sqrt(5.0 ** 2 + np.abs(clean))
    data = clean + noise * rng.standard_normal(clean.shape)
    r = build_psf(image=data, noisemap=noise, subsampling_factor=ss, masks=np.ones_like(data), guess_fwhm_pixels=3.5,
                  field_distortion=True, stamp_coordinates=xy, **KW)
    _check_result(r, S, n, ss)
    kd = r['kwargs_psf']['kwargs_distortion']
    assert set(kd) == {'dilation_x', 'dilation_y', 'shear'} and all(np.asarray(v).shape == (3,) for v in kd.values())
    assert all(np.all(np.isfinite(np.asarray(v))) for v in kd.values())
    star_psf = apply_distortion(r['narrow_psf'], kd, xy[:1], ctx=ctx)
    assert star_psf.shape == (N, N) and abs(star_psf.sum() - 1.0) < 1e-5 and np.all(np.isfinite(star_psf))
