"""Batched star photometry with a background grid per star (lc_joint_create_groups_background): the reference's
do_one_star_forward_modelling with starlet_global_background=True - its own default (lightcurver/processes/star_photometry.py:
23-24) - once per reference star (:257-326) as ONE device object.  Each star of the batch must end bit for bit where its own
one-star fit with h free ends: the same epoch kernel per epoch (reading its star's h and positions), the same regulariser,
reduction and update per star."""
import time

import numpy as np
import pytest

from lightcurver_amd.synthetic import make_roi_dataset
from tests import helpers as H

pytestmark = pytest.mark.gpu

LAM = dict(lam_scales=3.0, lam_hf=3.0)


def _stars(E_list, n, seed, ss=2):
    return [make_roi_dataset(E=E, M=1, n=n, ss=ss, seed=seed + g, with_background=True) for g, E in enumerate(E_list)]


def _start(ds, rng):
    E = ds['data'].shape[0]
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    p['a'] = p['a'] * rng.uniform(0.8, 1.2, E)
    p['c_x'] = p['c_x'] + rng.normal(0, 0.2, 1)
    p['c_y'] = p['c_y'] + rng.normal(0, 0.2, 1)
    p['h'] = np.zeros_like(p['h'])
    return p


def _batch(stars, ctx, ss=2):
    from lightcurver_amd.joint import StarPhotometryBatch
    return StarPhotometryBatch([(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf']) for ds in stars], ss, 1, ctx,
                               background=True)


@pytest.mark.parametrize('n,E_list,free', [(16, [5, 1, 7, 3], ('a', 'c_x', 'c_y', 'dx', 'dy', 'h')),
                                           (24, [4, 6, 1], ('a', 'c_x', 'c_y', 'dx', 'dy', 'h', 'mean')),
                                           (32, [3, 5], ('a', 'c_x', 'c_y', 'dx', 'dy', 'h', 'mean'))])
def test_every_star_equals_its_own_background_fit(ctx, n, E_list, free):
    from lightcurver_amd.joint import JointFit
    G, T = len(E_list), 40
    stars = _stars(E_list, n, 600 + n)
    rng = np.random.default_rng(11)
    starts = [_start(ds, rng) for ds in stars]
    cfg = dict(init_learning_rate=1e-3, schedule_learning_rate=True)
    single, Ws = [], []
    for ds, p in zip(stars, starts):
        j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], 2, 1, ctx)
        W = j.propagate_noise()
        Ws.append(W)
        j.set_params(**p)
        j.set_loss(W=W, **LAM)
        j.set_free(list(free))
        j.run_adabelief(T, **cfg)
        E = ds['data'].shape[0]
        single.append((j.get_params(), j.loss_history(), j.model(), j.fisher_flux_sigma(), j.deconvolved(E - 1)))
        j.close()
    b = _batch(stars, ctx)
    W = b.propagate_noise()
    assert W.shape == (G, b.J + 1, b.N, b.N)
    for g in range(G):
        assert np.array_equal(W[g], Ws[g]), g
    cat = {k: np.concatenate([p[k] for p in starts]) for k in ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha', 'h', 'mean')}
    assert cat['h'].size == b.sizes['h'] == G * b.N * b.N
    b.set_params(**cat)
    b.set_loss(W=W, **LAM)
    b.set_free(list(free))
    b.run_adabelief(T // 2, **cfg)
    b.run_adabelief(T - T // 2, **cfg)            # a second call continues the first
    got, hist, (model, chi2_e), sig = b.get_params(), b.loss_history(), b.model(), b.fisher_flux_sigma()
    assert hist.shape == (G, T + 1) and b.iterations_done == T
    for g in range(G):
        ps, hs, (ms, cs), ss_, (scene, bgr) = single[g]
        for k in ('a', 'c_x', 'c_y', 'dx', 'dy', 'mean', 'h'):
            assert np.array_equal(b.split(got[k], k)[g], ps[k]), (g, k)
        assert np.array_equal(hist[g], hs), g
        e0, e1 = b.starts[g], b.starts[g + 1]
        assert np.array_equal(model[e0:e1], ms) and np.array_equal(chi2_e[e0:e1], cs), g
        assert np.array_equal(sig[e0:e1], ss_), g
        s2, b2 = b.deconvolved(e1 - 1)
        assert np.array_equal(s2, scene) and np.array_equal(b2, bgr), g
        assert np.any(ps['h'] != 0.0) and hs[-1] < hs[0]
    b.close()


@pytest.mark.parametrize('n,ss', [(16, 2), (16, 1)])
def test_noise_propagation_per_star(ctx, n, ss):
    from lightcurver_amd.joint import JointFit
    stars = _stars([4, 1, 6], n, 700, ss)
    b = _batch(stars, ctx, ss)
    W = b.propagate_noise()
    b.close()
    for g, ds in enumerate(stars):
        j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], ss, 1, ctx)
        assert np.array_equal(W[g], j.propagate_noise()), g
        j.close()


@pytest.mark.parametrize('uniform', [False, True])
@pytest.mark.parametrize('n', [16, 24, 20])
def test_step_function_runs_batched(ctx, monkeypatch, n, uniform):
    """do_many_stars_forward_modelling(starlet_global_background=True): all ten keys bit for bit those of the one-star function -
    and computed WITHOUT it (the one-star function is made to raise: the loop over stars cannot be reached)."""
    from lightcurver_amd.processes import star_photometry as sp
    E_list, T = [5, 1, 4], 30
    stars = _stars(E_list, n, 800 + n)

    def stacks():
        return [(ds['data'].astype(np.float64) * ds['scale'] + 3.0 * uniform, ds['noisemap'].astype(np.float64) * ds['scale'], ds['psf'])
                for ds in stars]
    ref = [sp.do_one_star_forward_modelling(d, nm, p, 2, n_iter=T, uniform_background_per_epoch=uniform, starlet_global_background=True)
           for d, nm, p in stacks()]

    def no_loop(*a, **k):
        raise AssertionError('the loop over stars was reached')
    monkeypatch.setattr(sp, 'do_one_star_forward_modelling', no_loop)
    out = sp.do_many_stars_forward_modelling(stacks(), 2, n_iter=T, uniform_background_per_epoch=uniform, starlet_global_background=True)
    assert len(out) == len(ref)
    for o, r in zip(out, ref):
        assert set(o) == set(r)
        for key in ('fluxes', 'fluxes_uncertainties', 'chi2_per_frame', 'residuals', 'deconvolved_image', 'starlet_background'):
            assert np.array_equal(np.asarray(o[key]), np.asarray(r[key])), key
        assert o['chi2'] == r['chi2'] and list(o['loss_curve']) == list(r['loss_curve']) and o['scale'] == r['scale']
        for grp in ('kwargs_analytic', 'kwargs_background'):
            for k, v in r['kwargs_final'][grp].items():
                assert np.array_equal(np.asarray(o['kwargs_final'][grp][k]), np.asarray(v)), (grp, k)
        assert np.any(np.asarray(o['starlet_background']) != 0.0)


def test_refusals_and_the_loop_beyond_scope(ctx):
    from lightcurver_amd import _lib
    from lightcurver_amd.joint import StarPhotometryBatch
    from lightcurver_amd.processes.star_photometry import do_many_stars_forward_modelling, do_one_star_forward_modelling
    stars = _stars([3, 2], 16, 900)
    b = _batch(stars, ctx)
    G, NN = 2, b.N * b.N
    with pytest.raises(_lib.LcError):
        b.set_loss(lam_pts_source=0.1, **LAM)
    with pytest.raises(_lib.LcError):
        b.loss_grad(('a',))
    with pytest.raises(_lib.LcError):
        b.step_local()
    with pytest.raises(_lib.LcError):
        b.run_lbfgs(2)
    with pytest.raises(_lib.LcError):
        b.param_history_begin(4)
    with pytest.raises(_lib.LcError):
        b.set_params(h=np.zeros(NN))                 # one star's worth
    with pytest.raises(ValueError):
        b.set_loss(W=np.ones((G, 3, b.N, b.N)), **LAM)    # too few scales
    with pytest.raises(ValueError):
        b.set_loss(W=np.ones((b.J + 1, b.N, b.N)), **LAM)  # the one-star layout
    b.set_free(['a', 'dx'])                          # h fixed: no background loop to run
    with pytest.raises(_lib.LcError):
        b.run_adabelief(2)
    b.close()
    for n_out in (40, 64):                           # n = 40: no single-workgroup update; n = 64: the cluster form's size
        s_out = _stars([2], n_out, 901)
        with pytest.raises(_lib.LcError, match='single-workgroup update only'):
            StarPhotometryBatch([(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf']) for ds in s_out], 2, 1, ctx,
                                background=True)
    # ... so the step function loops there, with the one-star numbers
    s40 = _stars([2, 3], 40, 902)
    def stacks():
        return [(ds['data'].astype(np.float64) * ds['scale'], ds['noisemap'].astype(np.float64) * ds['scale'], ds['psf']) for ds in s40]
    ref = [do_one_star_forward_modelling(d, nm, p, 2, n_iter=6) for d, nm, p in stacks()]
    out = do_many_stars_forward_modelling(stacks(), 2, n_iter=6, starlet_global_background=True)
    for o, r in zip(out, ref):
        assert np.array_equal(o['fluxes'], r['fluxes']) and np.array_equal(o['starlet_background'], r['starlet_background'])
        assert list(o['loss_curve']) == list(r['loss_curve'])


def test_thirty_stars_with_backgrounds_against_the_loop(ctx):
    """30 stars x 100 epochs x 24^2 (the reference's default stamp_size_stars), 2000 iterations, starlet background on: the
    batched step function against the loop over the one-star function - same numbers per star; the ratio of the times goes
    to tests/test_zz_perf_star_background_gpu.py."""
    from lightcurver_amd.processes.star_photometry import do_many_stars_forward_modelling, do_one_star_forward_modelling
    G, E, n, T = 30, 100, 24, 2000
    base = make_roi_dataset(E=E, M=1, n=n, ss=2, seed=79, with_background=True)
    rng = np.random.default_rng(6)
    stacks = []
    for g in range(G):
        f = rng.uniform(0.3, 3.0)
        d = (base['data'].astype(np.float64) * f + 0.01 * rng.standard_normal(base['data'].shape)) * base['scale']
        nm = base['noisemap'].astype(np.float64) * np.sqrt(f) * base['scale']
        stacks.append((d, nm, base['psf']))
    loop_in = [(d.copy(), nm.copy(), p) for d, nm, p in stacks]
    do_one_star_forward_modelling(loop_in[0][0].copy(), loop_in[0][1].copy(), loop_in[0][2], 2, n_iter=5)   # warm-up
    do_many_stars_forward_modelling([(d.copy(), nm.copy(), p) for d, nm, p in stacks[:2]], 2, n_iter=5, starlet_global_background=True)
    ctx.synchronize()
    t0 = time.perf_counter()
    ref = [do_one_star_forward_modelling(d, nm, p, 2, n_iter=T) for d, nm, p in loop_in]
    t_loop = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = do_many_stars_forward_modelling(stacks, 2, n_iter=T, starlet_global_background=True)
    t_batch = time.perf_counter() - t0
    print(f'30 stars x 100 epochs x 24^2 x {T} iterations, starlet background: loop {t_loop:.2f} s, batch {t_batch:.2f} s, '
          f'ratio {t_loop / t_batch:.1f}')
    for g in range(G):
        assert np.array_equal(out[g]['fluxes'], ref[g]['fluxes']), g
        assert np.array_equal(out[g]['starlet_background'], ref[g]['starlet_background']), g
        assert np.array_equal(out[g]['kwargs_final']['kwargs_analytic']['c_x'], ref[g]['kwargs_final']['kwargs_analytic']['c_x'])
        assert out[g]['loss_curve'] == list(ref[g]['loss_curve']) and len(out[g]['loss_curve']) == T
        assert np.array_equal(out[g]['fluxes_uncertainties'], ref[g]['fluxes_uncertainties'])
        assert out[g]['chi2'] == ref[g]['chi2'] and np.array_equal(out[g]['residuals'], ref[g]['residuals'])
    H.PERF['star_bg_batch_over_loop'] = t_loop / t_batch
