"""Fisher information with the source positions free (lc_joint_fisher_positions, JointFit.fisher_positions): theta = (a, c_x,
c_y[, mean]), everything else fixed.  The oracle is the forward-mode Jacobian of the float64 oracle.model.deconv_model with
respect to (a, c_x, c_y, mean) and J^T W J; information and covariance are compared in normalised form (F / sqrt(d d^T),
d = diag F_oracle), so that flux and pixel units do not hide each other.  Then the new template path against the FFT
pipeline's flux covariance, the device solve against its host restatement, blended pairs, the prior, the degenerate cases,
chunking and determinism, an embedded size, the refusals and the facade."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import model as om
from lightcurver_amd.synthetic import make_roi_dataset
from lightcurver_amd.starred.optim.inference_base import arrowhead_covariance, dense_from_arrowhead
from tests import helpers as H

pytestmark = pytest.mark.gpu

ALPHAS = [0.0, 120.0, 180.0]
SHIFTS = [(0.0, 0.0), (1.3, -0.7), (-2.1, 1.6)]   # data pixels
# Normalised information: the project's bound for the flux blocks is 3e-5; measured on MI355X the largest deviation from the
# float64 oracle over all sizes below is 3.53e-7 (n = 24, 64), so the bound is tightened to four times that.
F_BOUND = 1.4e-6


def _problem(n, ss, M, seed, background, E=3, mask_frac=0.05):
    """Dataset at the rotations / shifts above, float32-rounded parameters, a few masked pixels per epoch (sigma2 = inf
    for the device, weight 0 for the oracle)."""
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=seed, alpha=ALPHAS[:E], with_background=background,
                          dx=[s[0] for s in SHIFTS[:E]], dy=[s[1] for s in SHIFTS[:E]])
    rng = np.random.default_rng(seed + 1)
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    p['a'] = p['a'] * rng.uniform(0.9, 1.1, p['a'].shape)
    if not background:
        p['h'] = np.zeros_like(p['h'])
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    sig2 = ds['noisemap'].astype(np.float64) ** 2
    sig2[rng.random(sig2.shape) < mask_frac] = np.inf
    return ds, p, sig2


def _joint(ctx, ds, sig2, p, ss, M, prior=None):
    from lightcurver_amd.joint import JointFit
    j = JointFit(ds['data'], sig2, ds['psf'], ss, M, ctx)
    j.set_params(**p)
    j.set_free(['a'])
    if prior is not None:
        j.set_loss(prior=prior)
    return j


def _prior(p, sigma_p):
    M = p['c_x'].size
    return {'c_x_mean': p['c_x'], 'c_x_sigma': np.full(M, sigma_p), 'c_y_mean': p['c_y'], 'c_y_sigma': np.full(M, sigma_p)}


def _oracle_fisher(ds, p, sig2, ss):
    """J^T W J of the float64 oracle in the order a (E M), c_x, c_y, mean (E); forward-mode Jacobian."""
    E, n, _ = ds['data'].shape
    po = {k: om.T(v) for k, v in p.items()}
    psf = om.T(ds['psf'])
    names = ('a', 'c_x', 'c_y', 'mean')
    fn = lambda a, cx, cy, m: om.deconv_model({**po, 'a': a, 'c_x': cx, 'c_y': cy, 'mean': m}, psf, ss, n)
    J = torch.autograd.functional.jacobian(fn, tuple(po[k] for k in names), vectorize=True, strategy='forward-mode')
    J = np.concatenate([j.reshape(E * n * n, -1).numpy() for j in J], axis=1)
    s2 = sig2.astype(np.float32).astype(np.float64)  # (the device holds sigma2 in float32)
    w = np.where(np.isfinite(s2), 1.0 / np.where(np.isfinite(s2), s2, 1.0), 0.0).reshape(-1)
    return J.T @ (w[:, None] * J)


SIZES = [(16, 1, 2), (16, 2, 3), (24, 2, 4), (32, 2, 2), (40, 2, 3), (64, 2, 8), (128, 2, 2)]


@functools.lru_cache(maxsize=None)
def _case(n, ss, M, background=True):
    """One problem per size and its oracle information (all four blocks free), computed once and never modified."""
    E = 2 if n == 128 else 3
    ds, p, sig2 = _problem(n, ss, M, 900 + n + ss + M, background, E=E)
    Fo = _oracle_fisher(ds, p, sig2, ss)
    Fo.setflags(write=False)
    return ds, p, sig2, Fo


def _select(Fo, E, M, positions, mean, sigma_p=None):
    """The oracle's information of the free set (order a, c_x, c_y, mean), prior added."""
    keep = list(range(E * M)) + (list(range(E * M, E * M + 2 * M)) if positions else []) \
        + (list(range(E * M + 2 * M, E * M + 2 * M + E)) if mean else [])
    F = np.array(Fo[np.ix_(keep, keep)])
    if sigma_p is not None:
        for k in range(E * M, E * M + 2 * M):
            F[k, k] += 1.0 / sigma_p ** 2
    return F


def _dense(res, M, covariance):
    k = 'C' if covariance else 'F'
    S = res[k + '_shared']
    return dense_from_arrowhead(res[k + '_local'], res[k + '_cross'] if S.size else None, S if S.size else None, M,
                                covariance=covariance)


def _sigma_dense(res, E, M):
    """The device's sigmas in the dense order."""
    return np.concatenate([res['sigma_a'], res['sigma_c'], res['sigma_mean']]).astype(np.float64)


def _check_against_oracle(res, Fo, E, M, label):
    """Information within F_BOUND, covariance and sigma within 3e-6 cond + 1e-6, all in normalised form; returns the
    measured figures."""
    d = np.sqrt(np.diag(Fo))
    nrm = np.outer(d, d)
    Fn = Fo / nrm
    err_F = float(np.abs(_dense(res, M, False) / nrm - Fn).max())
    cond = float(np.linalg.cond(Fn))
    Cn = np.linalg.inv(Fn)
    err_C = H.rel_err(_dense(res, M, True) * nrm, Cn)
    err_s = float(np.max(np.abs(_sigma_dense(res, E, M) * d / np.sqrt(np.diag(Cn)) - 1.0)))
    print(f'{label}: max|dF~| = {err_F:.3g}, cond = {cond:.3g}, rel_err C~ = {err_C:.3g}, sigma = {err_s:.3g}')
    assert err_F < F_BOUND, (label, err_F)
    assert err_C < 3e-6 * cond + 1e-6, (label, cond, err_C)
    assert err_s < 3e-6 * cond + 1e-6, (label, cond, err_s)
    return err_F, cond, err_C


@pytest.mark.parametrize('n,ss,M', SIZES)
@pytest.mark.parametrize('mean', [False, True], ids=['a+c', 'a+c+mean'])
def test_native_sizes_match_the_oracle_jacobian(ctx, n, ss, M, mean):
    ds, p, sig2, Fo = _case(n, ss, M)
    E = ds['data'].shape[0]
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        res = j.fisher_positions(positions=True, mean=mean)
    finally:
        j.close()
    Lp = M + (1 if mean else 0)
    assert res['F_local'].shape == res['C_local'].shape == (E, Lp, Lp)
    assert res['F_cross'].shape == res['C_cross'].shape == (E, Lp, 2 * M)
    assert res['F_shared'].shape == res['C_shared'].shape == (2 * M, 2 * M)
    assert res['sigma_a'].shape == (E * M,) and res['sigma_c'].shape == (2 * M,)
    assert res['sigma_mean'].shape == ((E,) if mean else (0,))
    _check_against_oracle(res, _select(Fo, E, M, True, mean), E, M, f'n={n} ss={ss} M={M} mean={mean}')


def test_prior_enters_the_shared_block(ctx):
    n, ss, M = 24, 2, 4
    ds, p, sig2, Fo = _case(n, ss, M)
    E = ds['data'].shape[0]
    j = _joint(ctx, ds, sig2, p, ss, M, prior=_prior(p, 0.05))
    try:
        res = j.fisher_positions()          # prior=None: used, because one is set
        off = j.fisher_positions(prior=False)
    finally:
        j.close()
    _check_against_oracle(res, _select(Fo, E, M, True, False, 0.05), E, M, 'prior 0.05')
    _check_against_oracle(off, _select(Fo, E, M, True, False), E, M, 'prior off')


@pytest.mark.parametrize('n,ss,M', SIZES)
@pytest.mark.parametrize('background', [True, False], ids=['fft', 'ps'])
def test_template_path_equals_the_fft_pipeline(ctx, n, ss, M, background):
    """positions=False is the flux covariance through the new template kernel: against fisher_flux_covariance() (FFT pipeline
    with h, point-source kernel without)."""
    E = 2 if n == 128 else 3
    ds, p, sig2 = _problem(n, ss, M, 900 + n + ss + M, background, E=E)
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        F, Cv, sig = j.fisher_flux_covariance()
        res = j.fisher_positions(positions=False)
    finally:
        j.close()
    assert res['F_shared'].size == res['F_cross'].size == res['sigma_c'].size == 0
    for e in range(E):
        err = H.rel_err(res['F_local'][e], F[e])
        cond = np.linalg.cond(F[e].astype(np.float64))
        err_c = H.rel_err(res['C_local'][e], Cv[e])
        print(f'n={n} e={e}: F {err:.3g}, cond {cond:.3g}, C {err_c:.3g}')
        assert err < 3e-5, (e, err)
        assert err_c < 3e-6 * cond + 1e-6, (e, cond, err_c)
    assert np.allclose(res['sigma_a'], sig, rtol=3e-6 * cond + 1e-6)


@pytest.mark.parametrize('n,ss,M,mean', [(16, 2, 3, True), (24, 2, 4, False), (64, 2, 8, True)])
def test_device_solve_is_the_host_restatement(ctx, n, ss, M, mean):
    ds, p, sig2, _ = _case(n, ss, M)
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        res = j.fisher_positions(mean=mean)
    finally:
        j.close()
    ref = arrowhead_covariance(res['F_local'], res['F_cross'], res['F_shared'])
    Fd = _dense(res, M, False)
    d = np.sqrt(np.diag(Fd))
    cond = np.linalg.cond(Fd / np.outer(d, d))
    tol = 3e-6 * cond + 1e-6
    for k in ('C_local', 'C_cross', 'C_shared'):
        assert H.rel_err(res[k], ref[k]) < tol, (k, H.rel_err(res[k], ref[k]), tol)
    assert np.allclose(res['sigma_a'], ref['sigma_local'][:, :M].ravel(), rtol=tol)
    assert np.allclose(res['sigma_c'], ref['sigma_shared'], rtol=tol)
    if mean:
        assert np.allclose(res['sigma_mean'], ref['sigma_local'][:, M], rtol=tol)


def _pair(ctx, n, sep, seed=31):
    """Two sources `sep` data pixels apart along x, h zero, no mask."""
    ds, p, sig2 = _problem(n, 2, 2, seed, False, E=2, mask_frac=0.0)
    p['c_x'] = np.array([-sep / 2.0, sep / 2.0])
    p['c_y'] = np.array([0.3, 0.3])
    return _joint(ctx, ds, sig2, p, 2, 2)


@pytest.mark.parametrize('sep', [2.0, 6.0])
def test_blended_and_separated_pair(ctx, sep):
    j = _pair(ctx, 32, sep)
    try:
        free = j.fisher_positions()['sigma_a']
        fixed = j.fisher_flux_covariance()[2]
    finally:
        j.close()
    ratio = free / fixed
    print(f'sep {sep}: sigma(a) positions free / fixed = {ratio}')
    assert np.all(free >= fixed * (1 - 1e-6))
    if sep == 2.0:
        assert np.all(ratio > 2.0), ratio        # oracle: 4.2 - 5.1
    else:
        assert np.all((ratio >= 1 - 1e-6) & (ratio <= 1.1)), ratio   # oracle: <= 1.04


def test_tight_prior_pins_the_positions(ctx):
    n, ss, M = 24, 2, 4
    ds, p, sig2, _ = _case(n, ss, M)
    sp = 1e-4
    j = _joint(ctx, ds, sig2, p, ss, M, prior=_prior(p, sp))
    try:
        res = j.fisher_positions(prior=True)
        flux = j.fisher_positions(positions=False)
    finally:
        j.close()
    assert np.all(res['sigma_c'] <= sp) and np.all(res['sigma_c'] > sp * (1 - 1e-3)), res['sigma_c']
    assert H.rel_err(res['C_local'], flux['C_local']) < 1e-3


def test_source_outside_the_stamp(ctx):
    n, M, E = 24, 3, 3
    ds, p, sig2 = _problem(n, 2, M, 77, True, E=E)
    p['c_x'][2], p['c_y'][2] = 1000.0, -1000.0
    sp = 0.05
    j = _joint(ctx, ds, sig2, p, 2, M)
    try:
        res = j.fisher_positions(mean=True)
        j.set_loss(prior=_prior(p, sp))
        pri = j.fisher_positions(mean=True)
    finally:
        j.close()
    p2 = dict(p, a=p['a'].reshape(E, M)[:, :2].ravel(), c_x=p['c_x'][:2], c_y=p['c_y'][:2])
    j2 = _joint(ctx, ds, sig2, p2, 2, 2)
    try:
        two = j2.fisher_positions(mean=True)
    finally:
        j2.close()
    loc, sh = [0, 1, 3], [0, 1, 3, 4]      # the two sources (and the mean) in the three-source layout
    assert np.all(np.isinf(res['sigma_a'].reshape(E, M)[:, 2])) and np.all(np.isinf(res['sigma_c'][[2, 5]]))
    for k in ('F_local', 'C_local'):
        assert np.all(res[k][:, 2, :] == 0) and np.all(res[k][:, :, 2] == 0), k
    for k in ('F_cross', 'C_cross'):
        assert np.all(res[k][:, 2, :] == 0) and np.all(res[k][:, :, [2, 5]] == 0), k
    for k in ('F_shared', 'C_shared'):
        assert np.all(res[k][[2, 5], :] == 0) and np.all(res[k][:, [2, 5]] == 0), k
    assert np.allclose(res['C_local'][:, loc][:, :, loc], two['C_local'], rtol=1e-5, atol=0)
    assert np.allclose(res['C_cross'][:, loc][:, :, sh], two['C_cross'], rtol=1e-5, atol=1e-5 * np.abs(two['C_cross']).max())
    assert np.allclose(res['C_shared'][sh][:, sh], two['C_shared'], rtol=1e-5, atol=1e-5 * np.abs(two['C_shared']).max())
    assert np.allclose(res['sigma_a'].reshape(E, M)[:, :2], two['sigma_a'].reshape(E, 2), rtol=1e-5)
    assert np.allclose(res['sigma_c'][sh], two['sigma_c'], rtol=1e-5)
    assert np.allclose(res['sigma_mean'], two['sigma_mean'], rtol=1e-5)
    # with a prior the position of the absent source is known to the prior's width, its flux still not at all
    assert np.allclose(pri['sigma_c'][[2, 5]], sp, rtol=1e-6)
    assert np.all(np.isinf(pri['sigma_a'].reshape(E, M)[:, 2]))


def test_two_sources_at_one_position(ctx):
    n, M = 24, 2
    ds, p, sig2 = _problem(n, 2, M, 91, True, E=3)
    p['c_x'][1], p['c_y'][1] = p['c_x'][0], p['c_y'][0]
    j = _joint(ctx, ds, sig2, p, 2, M)
    try:
        res = j.fisher_positions()
    finally:
        j.close()
    for k, v in res.items():
        if k.startswith('F_'):
            assert np.all(np.isfinite(v)), k
        else:
            assert np.all(np.isnan(v)), k
    assert np.all(res['F_local'][:, 0, 0] > 0)


def test_chunks_and_determinism(ctx):
    """150 epochs at n = 64, M = 8: the slab takes 128 epochs, so two chunks."""
    from lightcurver_amd import _lib
    from lightcurver_amd.joint import JointFit
    E, n, ss, M = 150, 64, 2, 8
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=5151, with_background=True)
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    sig2 = ds['noisemap'].astype(np.float64) ** 2

    def make(lo, hi):
        q = dict(p, a=p['a'][lo * M:hi * M], dx=p['dx'][lo:hi], dy=p['dy'][lo:hi], alpha=p['alpha'][lo:hi],
                 mean=p['mean'][lo:hi])
        j = JointFit(ds['data'][lo:hi], sig2[lo:hi], ds['psf'][lo:hi], ss, M, ctx)
        j.set_params(**q)
        return j

    j = make(0, E)
    try:
        res = j.fisher_positions(mean=True)
        again = j.fisher_positions(mean=True)
        # NULL outputs in any combination
        lib, names = _lib.lib(), _lib.FISHER_POSITIONS_FIELDS
        for given in ([], ['sigma_c'], ['F_local', 'C_cross'], ['C_shared', 'sigma_a', 'sigma_mean']):
            bufs = {k: np.full_like(res[k], -7.0) for k in given}
            out = _lib.FisherPositionsOut(*[_lib.ptr(bufs.get(k)) for k in names])
            assert lib.lc_joint_fisher_positions(j.h, 3, ctypes.byref(out)) == 0, given
            for k in given:
                assert np.array_equal(bufs[k], res[k]), k
    finally:
        j.close()
    for k in res:
        assert np.array_equal(res[k], again[k], equal_nan=True), k
    assert np.all(np.isfinite(res['sigma_a'])) and np.all(np.isfinite(res['sigma_c']))
    parts = []
    for lo, hi in ((0, 70), (70, E)):
        jp = make(lo, hi)
        try:
            parts.append(jp.fisher_positions(mean=True))
        finally:
            jp.close()
    for k in ('F_local', 'F_cross'):
        assert np.array_equal(res[k], np.concatenate([q[k] for q in parts])), k
    total = parts[0]['F_shared'].astype(np.float64) + parts[1]['F_shared'].astype(np.float64)
    assert H.rel_err(res['F_shared'], total) < 1e-6


def _pad(x, p, fill=0.0):
    x = np.asarray(x)
    out = np.full((x.shape[0], x.shape[1] + 2 * p, x.shape[2] + 2 * p), fill, np.float64)
    out[:, p:-p, p:-p] = x
    return out


def test_embedded_size(ctx):
    from lightcurver_amd.joint import EmbeddedJointFit, JointFit, joint_fit_size
    n, ss, M, E = 20, 2, 2, 3
    ds, p, sig2 = _problem(n, ss, M, 320, True, E=E)
    n_fit = joint_fit_size(n, ss)
    assert n_fit > n
    j = EmbeddedJointFit(ds['data'], sig2, ds['psf'], ss, M, ctx, n_fit)
    try:
        j.set_params(**p)
        res = j.fisher_positions(mean=True)
        big = JointFit(_pad(ds['data'], j.pad), _pad(sig2, j.pad, EmbeddedJointFit.RING_VARIANCE), j._psf_fit, ss, M, ctx)
        try:
            big.set_params(**dict(p, h=j._pad_h(p['h'])))
            ref = big.fisher_positions(mean=True)
        finally:
            big.close()
    finally:
        j.close()
    for k in res:
        assert np.array_equal(res[k], ref[k]), k
    _check_against_oracle(res, _oracle_fisher(ds, p, sig2, ss), E, M, 'embedded n=20')


def test_refusals_leave_the_object_usable(ctx):
    from lightcurver_amd import _lib
    from lightcurver_amd.joint import StarPhotometryBatch
    n, ss, M = 16, 2, 3
    ds, p, sig2, _ = _case(n, ss, M)
    E = ds['data'].shape[0]
    b = StarPhotometryBatch([(ds['data'], sig2, ds['psf'])], ss, M, ctx)
    try:
        with pytest.raises(NotImplementedError):
            b.fisher_positions()
        buf = np.full(E * M, -7.0, np.float32)
        out = _lib.FisherPositionsOut(sigma_a=_lib.ptr(buf))
        assert _lib.lib().lc_joint_fisher_positions(b.h, 1, ctypes.byref(out)) == -3   # LC_ERR_UNSUPPORTED
        assert np.all(buf == -7.0)
    finally:
        b.close()
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        with pytest.raises(_lib.LcError):
            j.fisher_positions(prior=True)            # no prior set
        buf = np.full(2 * M, -7.0, np.float32)
        out = _lib.FisherPositionsOut(sigma_c=_lib.ptr(buf))
        assert _lib.lib().lc_joint_fisher_positions(j.h, 2, ctypes.byref(out)) == -1   # shared output, positions fixed
        assert np.all(buf == -7.0)
        res = j.fisher_positions()
        assert np.all(np.isfinite(res['sigma_a'])) and np.all(np.isfinite(res['sigma_c']))
    finally:
        j.close()


def test_facade(ctx):
    """FisherCovariance(free = a, c_x, c_y) through setup_model / ParametersDeconv / Loss(prior) / Optimizer, the
    lightcurver-level helpers and the ROI fit with marginalize_positions."""
    import warnings
    from copy import deepcopy
    from lightcurver_amd.starred.deconvolution.deconvolution import setup_model
    from lightcurver_amd.starred.deconvolution.loss import Loss, Prior
    from lightcurver_amd.starred.deconvolution.parameters import ParametersDeconv
    from lightcurver_amd.starred.optim.inference_base import FisherCovariance
    from lightcurver_amd.starred.optim.optimization import Optimizer
    from lightcurver_amd.utilities.starred_utilities import (get_flux_covariance, get_flux_uncertainties,
                                                             get_position_covariance)
    E, M = 5, 3
    ds = make_roi_dataset(E=E, M=M, n=16, ss=2, seed=12)
    data, noise, s = ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64), ds['psf']
    t = ds['truth']
    model, k_init, k_up, k_down, k_fixed = setup_model(data, noise ** 2, s, t['c_x'], t['c_y'], 2, list(t['a']))

    def fisher(free, prior=None, diagonal_only=False):
        frozen = deepcopy(k_init)
        for k in free:
            frozen['kwargs_analytic' if k != 'mean' else 'kwargs_background'].pop(k)
        pars = ParametersDeconv(kwargs_init=k_init, kwargs_fixed=frozen, kwargs_up=k_up, kwargs_down=k_down)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            loss = Loss(data, model, pars, noise ** 2, regularization_terms='l1_starlet', prior=prior)
        return FisherCovariance(pars, Optimizer(loss, pars, method='l-bfgs-b'), diagonal_only=diagonal_only), loss, pars

    flux, loss, pars = fisher(['a'])
    fit = loss.configure()
    fit.set_params(**pars._current)
    F0, C0, s0 = fit.fisher_flux_covariance()
    assert np.array_equal(flux.flux_covariance_blocks, C0)            # free == ['a']: the arrays of before
    assert np.array_equal(np.asarray(flux.get_kwargs_sigma()['kwargs_analytic']['a']), s0)

    full, _, _ = fisher(['a', 'c_x', 'c_y'])
    sig = full.get_kwargs_sigma()['kwargs_analytic']
    sa, sx, sy = (np.asarray(sig[k]) for k in ('a', 'c_x', 'c_y'))
    assert sa.shape == (E * M,) and sx.shape == sy.shape == (M,)
    assert np.all(np.isfinite(sa)) and np.all(sx > 0) and np.all(sy > 0) and np.all(np.isfinite(sx + sy))
    assert np.all(sa >= s0 * (1 - 1e-6))
    P = E * M + 2 * M
    Fm, Cm = full.fisher_matrix, full.covariance_matrix
    assert Fm.shape == Cm.shape == (P, P)
    d = np.sqrt(np.diag(Fm))
    cond = np.linalg.cond(Fm / np.outer(d, d))
    assert H.rel_err(Cm * np.outer(d, d), np.linalg.inv(Fm / np.outer(d, d))) < 3e-6 * cond + 1e-6
    assert full.position_covariance.shape == (2 * M, 2 * M)
    assert full.flux_covariance_blocks.shape == (E, M, M)
    assert np.allclose(np.sqrt(np.diag(full.position_covariance)), np.concatenate([sx, sy]), rtol=1e-6)
    diag, _, _ = fisher(['a', 'c_x', 'c_y'], diagonal_only=True)
    sd = diag.get_kwargs_sigma()['kwargs_analytic']
    assert np.allclose(np.asarray(sd['c_x']), 1.0 / np.sqrt(np.diag(Fm)[E * M:E * M + M]), rtol=1e-6)
    assert np.all(np.asarray(sd['a']) <= sa * (1 + 1e-6))
    with_mean, _, _ = fisher(['a', 'c_x', 'c_y', 'mean'])
    assert with_mean.fisher_matrix.shape == (P + E, P + E)
    sm = np.asarray(with_mean.get_kwargs_sigma()['kwargs_background']['mean'])
    assert sm.shape == (E,) and np.all(sm > 0) and np.all(np.isfinite(sm))
    # a prior on the positions tightens them
    pri, _, _ = fisher(['a', 'c_x', 'c_y'], prior=Prior(prior_analytic=[['c_x', t['c_x'], 0.01], ['c_y', t['c_y'], 0.01]]))
    sp = pri.get_kwargs_sigma()['kwargs_analytic']
    assert np.all(np.asarray(sp['c_x']) <= 0.01) and np.all(np.asarray(sp['c_x']) <= sx * (1 + 1e-6))

    cov0 = get_flux_covariance(deepcopy(k_init), k_up, k_down, data, noise, model, refine_iterations=3)
    cov1 = get_flux_covariance(deepcopy(k_init), k_up, k_down, data, noise, model, refine_iterations=3, free_positions=True)
    assert cov1.shape == cov0.shape == (E, M, M) and np.all(np.isfinite(cov1))
    d0, d1 = (np.stack([np.diag(c) for c in cv]) for cv in (cov0, cov1))
    assert np.all(np.sqrt(d1) >= np.sqrt(d0) * (1 - 1e-6))
    cc, scx, scy = get_position_covariance(deepcopy(k_init), k_up, k_down, data, noise, model, refine_iterations=3)
    assert cc.shape == (2 * M, 2 * M) and scx.shape == scy.shape == (M,)
    assert np.allclose(np.sqrt(np.diag(cc)), np.concatenate([scx, scy]), rtol=1e-6) and np.all(np.isfinite(cc))
    su = get_flux_uncertainties(deepcopy(k_init), k_up, k_down, data, noise, model, refine_iterations=3)
    assert np.all(np.sqrt(d1).ravel() >= su * (1 - 1e-5))


def test_roi_fit_marginalises_the_positions(ctx):
    """The ROI fit at 5 x 16 x 16, M = 3 with marginalize_positions: the new entries, and the default unchanged."""
    from lightcurver_amd.processes.roi_modelling import fluxes_from_model, model_roi_cutouts, model_roi_cutouts_sharded
    from lightcurver_amd.starred.deconvolution.loss import Prior
    E, M, n, ss = 5, 3, 16, 2
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=12)
    t = ds['truth']
    off = (n - 1) / 2.0
    xs, ys = np.asarray(t['c_x']) + off, np.asarray(t['c_y']) + off

    def fit(**kw):
        return model_roi_cutouts(ds['data'].copy(), ds['noisemap'].copy(), ds['psf'], ss, xs, ys, fix_point_source_astrometry=0.5,
                                 roi_deconv_translations_iters=30, roi_deconv_all_iters=60, **kw)

    base, out = fit(), fit(marginalize_positions=True)
    assert 'astrometry_uncertainties' not in base and 'fluxes_sigma' not in base
    for k in ('kwargs_analytic', 'kwargs_background'):      # the fit itself is unchanged
        for name, v in base['kwargs_final'][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(out['kwargs_final'][k][name])), name
    au = out['astrometry_uncertainties']
    assert au['c_x_sigma'].shape == au['c_y_sigma'].shape == (M,) and au['covariance'].shape == (2 * M, 2 * M)
    assert np.all(np.isfinite(au['covariance'])) and np.all(au['c_x_sigma'] > 0) and np.all(au['c_y_sigma'] > 0)
    assert np.all(au['c_x_sigma'] <= 0.5) and np.all(au['c_y_sigma'] <= 0.5)      # no wider than the prior
    assert out['fluxes_sigma'].shape == (E * M,) and np.all(np.isfinite(out['fluxes_sigma']))
    args = (out['model'], out['kwargs_final'], out['kwargs_up'], out['kwargs_down'], out['data'], out['noisemap'], M,
            out['scale'], np.zeros(E))
    f0 = fluxes_from_model(*args)
    f1 = fluxes_from_model(*args, marginalize_positions=True,
                           prior=Prior(prior_analytic=[['c_x', xs - off, np.full(M, 0.5)], ['c_y', ys - off, np.full(M, 0.5)]]))
    assert 'astrometry_uncertainties' not in f0
    assert f1['d_fluxes'].shape == f0['d_fluxes'].shape == (M, E) and np.all(np.isfinite(f1['d_fluxes']))
    assert np.all(f1['d_fluxes'] >= f0['d_fluxes'] * (1 - 1e-6))
    assert np.array_equal(f1['fluxes'], f0['fluxes'])
    a1 = f1['astrometry_uncertainties']
    assert a1['covariance'].shape == (2 * M, 2 * M) and np.all(np.isfinite(a1['covariance']))
    with pytest.raises(NotImplementedError):
        model_roi_cutouts_sharded(ds['data'], ds['noisemap'], ds['psf'], ss, xs, ys, list(t['a'][:M]), 1.0,
                                  marginalize_positions=True)
