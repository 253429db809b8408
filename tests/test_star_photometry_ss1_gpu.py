"""Star photometry and the ROI fit through the facade at subsampling 1 above 16 x 16: the batch without a background at n = 24
(bit for bit every star's own fit), the route with a per-star background (the one-star function itself: no batch at these
sizes), the marginal flux errors, the reference's own fixture of tests/test_starred_calls/test_starred_calls.py at twice its
size, the two-stage ROI fit with its diagnostics, and the STARRED-shaped objects (setup_model / Loss / Optimizer,
propagate_noise, FisherCovariance, get_flux_covariance) at n = 32."""
import warnings
from copy import deepcopy

import numpy as np
import pytest

from lightcurver_amd.synthetic import make_narrow_psf, make_roi_dataset

pytestmark = pytest.mark.gpu

KEYS = {'scale', 'kwargs_final', 'fluxes', 'fluxes_uncertainties', 'chi2', 'chi2_per_frame', 'loss_curve', 'residuals',
        'deconvolved_image', 'starlet_background'}


def _stacks(E_list, n, ss, seed, uniform=False):
    stars = [make_roi_dataset(E=E, M=1, n=n, ss=ss, seed=seed + g, with_background=False) for g, E in enumerate(E_list)]
    return [(ds['data'].astype(np.float64) * ds['scale'] + 3.0 * uniform, ds['noisemap'].astype(np.float64) * ds['scale'], ds['psf'])
            for ds in stars]


def _assert_same_star(o, r, keys=KEYS):
    assert set(o) == set(r) == set(keys)
    for key in set(keys) - {'scale', 'kwargs_final', 'chi2', 'loss_curve'}:
        assert np.array_equal(np.asarray(o[key]), np.asarray(r[key])), key
    assert o['chi2'] == r['chi2'] and list(o['loss_curve']) == list(r['loss_curve']) and o['scale'] == r['scale']
    for grp in ('kwargs_analytic', 'kwargs_background'):
        for k, v in r['kwargs_final'][grp].items():
            assert np.array_equal(np.asarray(o['kwargs_final'][grp][k]), np.asarray(v)), (grp, k)


@pytest.mark.parametrize('uniform,starlet', [(False, False), (True, False), (False, True), (True, True)])
def test_every_star_of_a_batch_equals_its_own_fit(ctx, uniform, starlet):
    """Three stars with 3 / 5 / 4 epochs at n = 24: without a background one batched device fit, bit for bit each star's own
    one-star fit; with starlet_global_background=True the stars go through the one-star function one after the other (the
    sizes with a per-star-background batch are unchanged), so the results are equal because they are the same call."""
    from lightcurver_amd.joint import background_batch_supported, joint_fit_size
    from lightcurver_amd.processes.star_photometry import do_many_stars_forward_modelling, do_one_star_forward_modelling
    E_list, n, ss, T = [3, 5, 4], 24, 1, 50
    assert joint_fit_size(n, ss) == n and not background_batch_supported(n, ss)
    kw = dict(n_iter=T, uniform_background_per_epoch=uniform, starlet_global_background=starlet)
    ref = [do_one_star_forward_modelling(d, nm, p, ss, **kw) for d, nm, p in _stacks(E_list, n, ss, 520, uniform)]
    out = do_many_stars_forward_modelling(_stacks(E_list, n, ss, 520, uniform), ss, **kw)
    assert len(out) == len(ref)
    for o, r, E in zip(out, ref, E_list):
        _assert_same_star(o, r)
        assert len(o['loss_curve']) == T and np.all(np.isfinite(o['loss_curve'])) and o['loss_curve'][-1] < o['loss_curve'][0]
        assert o['residuals'].shape == (E, n, n) and o['deconvolved_image'].shape == (n * ss, n * ss)
        assert np.all(np.isfinite(o['fluxes'])) and np.all(o['fluxes_uncertainties'] > 0)
        if uniform:
            assert np.any(np.asarray(o['kwargs_final']['kwargs_background']['mean']) != 0.0)


def test_marginal_flux_errors(ctx):
    from lightcurver_amd.processes.star_photometry import do_many_stars_forward_modelling
    E_list, n, ss = [3, 5, 4], 24, 1
    plain = do_many_stars_forward_modelling(_stacks(E_list, n, ss, 540), ss, n_iter=50)
    out = do_many_stars_forward_modelling(_stacks(E_list, n, ss, 540), ss, n_iter=50, marginalize_shifts=True)
    for o, r, E in zip(out, plain, E_list):
        m = o.pop('fluxes_uncertainties_marginal')
        _assert_same_star(o, r)
        assert m.shape == (E,) and np.all(np.isfinite(m))
        assert np.all(m >= o['fluxes_uncertainties'] * (1 - 1e-6))


def test_reference_fixture_at_twice_its_size():
    """The fixture of the reference's test of its STARRED calls (gauss = exp(-0.1 r^2), 5 stamps, subsampling 1, 50
    iterations; seeded here) on 32 x 32 stamps, and the assertions of that test."""
    from lightcurver_amd.processes.star_photometry import do_one_star_forward_modelling
    from lightcurver_amd.starred.procedures.psf_routines import build_psf
    rng = np.random.default_rng(0)
    x, y = np.meshgrid(np.arange(-16, 16), np.arange(-16, 16))
    gauss = np.exp(-0.1 * (x ** 2 + y ** 2))
    data = 0.1 * rng.random((5, 32, 32)) + np.repeat(gauss[None, :, :], repeats=5, axis=0)
    noisemap = 0.1 * np.ones((5, 32, 32))
    psf = np.repeat(gauss[None, :, :], repeats=5, axis=0)
    n_iter = 50
    shape = data.shape
    res = build_psf(data.copy(), noisemap.copy(), subsampling_factor=1, n_iter_analytic=5, n_iter_adabelief=10,
                    masks=np.ones_like(data), guess_method_star_position='center')
    assert isinstance(res, dict)
    for key in ('full_psf', 'adabelief_extra_fields', 'narrow_psf', 'chi2', 'residuals'):
        assert key in res
    assert 'loss_history' in res['adabelief_extra_fields'] and len(res['adabelief_extra_fields']['loss_history']) == 10
    assert res['narrow_psf'].shape == (32, 32) and res['residuals'].shape == shape
    result = do_one_star_forward_modelling(data, noisemap, psf, 1, n_iter)
    assert isinstance(result, dict)
    for key in ('scale', 'kwargs_final', 'fluxes', 'fluxes_uncertainties', 'chi2', 'chi2_per_frame', 'loss_curve', 'residuals'):
        assert key in result
    assert isinstance(result['scale'], float) and result['scale'] > 0
    assert isinstance(result['kwargs_final'], dict)
    assert isinstance(result['fluxes'], np.ndarray) and isinstance(result['fluxes_uncertainties'], np.ndarray)
    assert result['fluxes'].ndim == 1 and result['fluxes_uncertainties'].ndim == 1
    assert result['fluxes'].size == result['fluxes_uncertainties'].size == shape[0]
    assert isinstance(result['chi2'], float) and result['chi2'] >= 0
    assert isinstance(result['chi2_per_frame'], np.ndarray) and result['chi2_per_frame'].ndim == 1
    assert len(result['chi2_per_frame']) == shape[0]
    assert len(result['loss_curve']) == n_iter
    assert result['residuals'].shape == shape


def test_model_roi_cutouts_and_the_stack_diagnostic(ctx):
    """E = 6, M = 2, n = 32, 30 + 50 iterations: the reference's shapes, a reduced chi2 that is finite and below the one
    the fit starts from, and the three diagnostic stacks (host and device form)."""
    from lightcurver_amd.joint import JointFit
    from lightcurver_amd.processes.roi_modelling import model_roi_cutouts, stack_data_diagnostic
    E, M, n, ss = 6, 2, 32, 1
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=77)
    t = ds['truth']
    off = (n - 1) / 2.0
    xs, ys = np.asarray(t['c_x']) + off, np.asarray(t['c_y']) + off
    out = model_roi_cutouts(ds['data'] * ds['scale'], ds['noisemap'] * ds['scale'], ds['psf'], ss, xs, ys,
                            roi_deconv_translations_iters=30, roi_deconv_all_iters=50)
    assert type(out['model']._fit) is JointFit
    k = out['kwargs_final']
    assert len(out['loss_history']) == 50 and np.all(np.isfinite(out['loss_history']))
    assert 1 <= len(out['loss_history_stage1']) <= 31 and np.all(np.isfinite(out['loss_history_stage1']))
    assert np.asarray(k['kwargs_background']['h']).size == (n * ss) ** 2
    assert np.asarray(k['kwargs_analytic']['a']).shape == (E * M,) and np.asarray(k['kwargs_analytic']['dx']).shape == (E,)
    assert out['x_pixels'].shape == (M,) and out['y_pixels'].shape == (M,)
    chi2 = lambda kw: float(np.mean(((out['data'] - np.asarray(out['model'].model(kw))) / out['noisemap']) ** 2))
    start = deepcopy(k)                      # what setup_model hands to stage 1
    start['kwargs_analytic']['a'] = np.array(E * list(out['initial_a']))
    start['kwargs_analytic']['c_x'] = xs - off
    start['kwargs_analytic']['c_y'] = ys - off
    start['kwargs_analytic']['dx'] = np.zeros(E)
    start['kwargs_analytic']['dy'] = np.zeros(E)
    start['kwargs_background']['h'] = np.zeros((n * ss) ** 2)
    start['kwargs_background']['mean'] = np.zeros(E)
    c_end, c_start = chi2(k), chi2(start)
    print('reduced chi2: start', c_start, 'final', c_end)
    assert np.asarray(out['model'].model(k)).shape == (E, n, n)
    assert np.isfinite(c_end) and c_end < c_start
    host = stack_data_diagnostic(out['data'], out['noisemap'], k, out['model'])
    dev = stack_data_diagnostic(out['data'], out['noisemap'], k, out['model'], on_device=True, ctx=ctx)
    for st in (host, dev):
        assert set(st) == {'stack', 'stack_no_ps', 'stack_no_background'}
        assert all(v.shape == (n, n) and np.all(np.isfinite(v)) for v in st.values())
        assert st['stack_no_ps'].sum() < st['stack'].sum()


def test_starred_objects_at_32(ctx):
    """setup_model / ParametersDeconv / Loss / Optimizer, propagate_noise, FisherCovariance, get_flux_covariance with the
    positions and with the shifts free."""
    from lightcurver_amd.starred.deconvolution.deconvolution import setup_model
    from lightcurver_amd.starred.deconvolution.loss import Loss, Prior
    from lightcurver_amd.starred.deconvolution.parameters import ParametersDeconv
    from lightcurver_amd.starred.optim.inference_base import FisherCovariance
    from lightcurver_amd.starred.optim.optimization import Optimizer
    from lightcurver_amd.starred.utils.noise_utils import propagate_noise
    from lightcurver_amd.utilities.starred_utilities import get_flux_covariance, get_flux_uncertainties
    E, M, n, ss = 4, 2, 32, 1
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=12)
    data, noise, s = ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64), ds['psf']
    t = ds['truth']
    model, k_init, k_up, k_down, _ = setup_model(data, noise ** 2, s, t['c_x'], t['c_y'], ss, list(0.9 * np.asarray(t['a'])), ctx=ctx)
    W = propagate_noise(model, noise, k_init, wavelet_type_list=['starlet'], method='SLIT', num_samples=200, seed=1,
                        likelihood_type='chi2', verbose=False, upsampling_factor=ss)[0]
    assert W.shape[1:] == (n * ss, n * ss) and np.all(np.isfinite(W)) and W.min() > 0
    fixed = deepcopy(k_init)
    for grp, name in (('kwargs_background', 'h'), ('kwargs_analytic', 'a'), ('kwargs_analytic', 'dx'), ('kwargs_analytic', 'dy')):
        del fixed[grp][name]
    pars = ParametersDeconv(kwargs_init=k_init, kwargs_fixed=fixed, kwargs_up=k_up, kwargs_down=k_down)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        loss = Loss(data, model, pars, noise ** 2, regularization_terms='l1_starlet', regularization_strength_scales=1.0,
                    regularization_strength_hf=1.0, regularization_strength_positivity=100.0, W=W)
    optim = Optimizer(loss, pars, method='adabelief')
    optim.minimize(max_iterations=40, init_learning_rate=1e-3, schedule_learning_rate=True, restart_from_init=False,
                   stop_at_loss_increase=False, progress_bar=False, return_param_history=False)
    lh = np.asarray(optim.loss_history)
    assert lh.shape == (40,) and np.all(np.isfinite(lh)) and lh[-1] < lh[0]
    k = pars.best_fit_values(as_kwargs=True)
    assert np.asarray(model.model(k)).shape == data.shape
    scene, bg = model.getDeconvolved(k, 0)
    assert scene.shape == (n * ss, n * ss) and bg.shape == (n * ss, n * ss)
    # the Fisher information of the fluxes at the fitted point (everything else held: the free sets it is built for)
    frozen = deepcopy(k)
    frozen['kwargs_analytic'].pop('a')
    pars_a = ParametersDeconv(kwargs_init=k, kwargs_fixed=frozen, kwargs_up=k_up, kwargs_down=k_down)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        loss_a = Loss(data, model, pars_a, noise ** 2, regularization_terms='l1_starlet')
    optim_a = Optimizer(loss_a, pars_a, method='l-bfgs-b')
    full = FisherCovariance(pars_a, optim_a, diagonal_only=False)
    diag = FisherCovariance(pars_a, optim_a, diagonal_only=True)
    s_full = np.asarray(full.get_kwargs_sigma()['kwargs_analytic']['a'])
    s_diag = np.asarray(diag.get_kwargs_sigma()['kwargs_analytic']['a'])
    assert s_full.shape == s_diag.shape == (E * M,) and np.all(s_diag > 0) and np.all(s_full >= s_diag * (1 - 1e-6))
    su = get_flux_uncertainties(deepcopy(k), k_up, k_down, data, noise, model, refine_iterations=3)
    prior = Prior(prior_analytic=[['c_x', np.asarray(t['c_x']), np.full(M, 0.05)], ['c_y', np.asarray(t['c_y']), np.full(M, 0.05)]])
    sig = {}
    for name, kw in (('fluxes', {}), ('positions', dict(free_positions=True)), ('shifts', dict(free_shifts=True)),
                     ('both', dict(free_positions=True, free_shifts=True, prior=prior))):
        cov = get_flux_covariance(deepcopy(k), k_up, k_down, data, noise, model, refine_iterations=3, **kw)
        assert cov.shape == (E, M, M) and np.all(np.isfinite(cov)), name
        sig[name] = np.sqrt(np.stack([np.diag(c) for c in cov]).ravel())
    assert np.all(sig['fluxes'] >= su * (1 - 1e-5))
    assert np.all(sig['positions'] >= sig['fluxes'] * (1 - 1e-5)) and np.all(sig['shifts'] >= sig['fluxes'] * (1 - 1e-5))


def test_place_psf_at_32(ctx):
    """joint.place_psf at subsampling 1 on the N = 32 grid: 24-wide stamps land centrally, 40-wide ones are cut to their
    window (with the warning), against the tests' own statement of the rule; and the fit made from the stamps is the fit made
    from the placed stack."""
    from lightcurver_amd.joint import JointFit, place_psf
    from tests import _psf_place as PP
    E, M, n, ss = 3, 1, 32, 1
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=51)
    sig2 = ds['noisemap'].astype(np.float64) ** 2
    for P in (24, 40):
        rng = np.random.default_rng(60 + P)
        stamps = np.stack([make_narrow_psf(rng, P, ss)[0] for _ in range(E)]).astype(np.float32)
        want = PP.place(stamps, n * ss)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)
            got = place_psf(stamps, n * ss)
            ja, jb = JointFit(ds['data'], sig2, stamps, ss, M, ctx), JointFit(ds['data'], sig2, want, ss, M, ctx)
        assert np.array_equal(np.asarray(got, np.float32), want)
        assert ja.psf_side == P and jb.psf_side == n * ss
        p = {k: np.asarray(v, np.float64) for k, v in ds['truth'].items()}
        ja.set_params(**p)
        jb.set_params(**p)
        ma, mb = ja.model(), jb.model()
        ja.close()
        jb.close()
        assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
