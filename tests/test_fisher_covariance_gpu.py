"""Flux covariance from the full Fisher information (lc_joint_fisher_flux_cov, JointFit.fisher_flux_covariance): with only the
fluxes free the model is linear in them, so F is the exact Hessian of 1/2 chi2, block diagonal over the epochs.  Checked
against torch.autograd.functional.hessian of the float64 oracle (as tests/test_oracle_cpu.py::test_fisher_is_hessian_diagonal
checks the diagonal), on both epoch paths - the FFT pipeline (h non-zero) and the point-source-only kernel (h zero) - at
every native stamp size, with masked pixels and rotated, shifted epochs; then the chunked template slab, the embedded sizes,
the batched star photometry, the STARRED facade and the sharded ROI fit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import model as om
from lightcurver_amd.synthetic import make_roi_dataset
from tests import helpers as H

pytestmark = pytest.mark.gpu

ALPHAS = [0.0, 120.0, 180.0]
SHIFTS = [(0.0, 0.0), (1.3, -0.7), (-2.1, 1.6)]   # data pixels


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


def _joint(ctx, ds, sig2, p, ss, M):
    from lightcurver_amd.joint import JointFit
    j = JointFit(ds['data'], sig2, ds['psf'], ss, M, ctx)
    j.set_params(**p)
    j.set_free(['a'])
    return j


def _oracle_hessian(ds, p, sig2, ss):
    """(E M, E M) Hessian of 1/2 sum w (data - model)^2 with respect to a, float64 (w = 0 where sigma2 is infinite)."""
    n = ds['data'].shape[-1]
    po = {k: om.T(v) for k, v in p.items()}
    data, psf = om.T(ds['data']), om.T(ds['psf'])
    s2 = sig2.astype(np.float32).astype(np.float64)  # (the device holds sigma2 in float32)
    w = om.T(np.where(np.isfinite(s2), 1.0 / np.where(np.isfinite(s2), s2, 1.0), 0.0))
    fn = lambda a: 0.5 * (w * (data - om.deconv_model({**po, 'a': a}, psf, ss, n)) ** 2).sum()
    return torch.autograd.functional.hessian(fn, po['a']).numpy()


def _check_against_oracle(j, ds, p, sig2, ss, M):
    E = ds['data'].shape[0]
    F, Cv, sig = j.fisher_flux_covariance()
    assert F.shape == Cv.shape == (E, M, M) and sig.shape == (E * M,)
    Hm = _oracle_hessian(ds, p, sig2, ss)
    for e in range(E):   # the epochs are independent: zero off-diagonal blocks in the oracle
        for f in range(E):
            if f != e:
                assert np.all(Hm[e * M:(e + 1) * M, f * M:(f + 1) * M] == 0.0), (e, f)
    s_cond = j.fisher_flux_sigma()
    for e in range(E):
        Hb = Hm[e * M:(e + 1) * M, e * M:(e + 1) * M]
        assert H.rel_err(F[e], Hb) < 3e-5, (e, H.rel_err(F[e], Hb))
        cond = np.linalg.cond(Hb)
        assert H.rel_err(Cv[e], np.linalg.inv(Hb)) < 3e-6 * cond + 1e-6, (e, cond, H.rel_err(Cv[e], np.linalg.inv(Hb)))
    d = np.stack([np.diag(F[e]) for e in range(E)]).ravel().astype(np.float64)
    assert np.max(np.abs(1.0 / np.sqrt(d) - s_cond) / s_cond) < 1e-6
    assert np.allclose(sig, np.sqrt(np.stack([np.diag(Cv[e]) for e in range(E)]).ravel()), rtol=1e-6)
    assert np.all(sig >= s_cond * (1 - 1e-6))
    return F, Cv, sig


SIZES = [(16, 1, 2), (16, 2, 3), (24, 2, 4), (32, 2, 2), (40, 2, 3), (64, 2, 4), (128, 2, 2)]


@pytest.mark.parametrize('n,ss,M', SIZES)
@pytest.mark.parametrize('background', [True, False], ids=['fft', 'ps'])
def test_native_sizes_match_the_oracle_hessian(ctx, n, ss, M, background):
    E = 2 if n == 128 else 3
    ds, p, sig2 = _problem(n, ss, M, 700 + n + ss + M, background, E=E)
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        _check_against_oracle(j, ds, p, sig2, ss, M)
    finally:
        j.close()


def _pair(ctx, n, sep, seed=31):
    """Two sources `sep` data pixels apart along x, h zero, no mask."""
    ds, p, sig2 = _problem(n, 2, 2, seed, False, E=2, mask_frac=0.0)
    p['c_x'] = np.array([-sep / 2.0, sep / 2.0])
    p['c_y'] = np.array([0.3, 0.3])
    return _joint(ctx, ds, sig2, p, 2, 2)


def _psf_fwhm_data_px(psf, ss=2):
    """FWHM of the PSF the data see (narrow PSF convolved with the FWHM = 2 high-resolution pixel Gaussian), data pixels."""
    P = np.asarray(psf[0], np.float64)
    N = P.shape[0]
    y, x = np.mgrid[:N, :N]
    m = P.sum()
    cx, cy = (P * x).sum() / m, (P * y).sum() / m
    var = (P * ((x - cx) ** 2 + (y - cy) ** 2)).sum() / m / 2.0
    return 2.3548 * np.sqrt(var + 0.8493218 ** 2) / ss


def test_blended_pair_is_anticorrelated(ctx):
    j = _pair(ctx, 32, 0.5)
    try:
        F, Cv, sig = j.fisher_flux_covariance()
        s_cond = j.fisher_flux_sigma()
    finally:
        j.close()
    for e in range(2):
        corr = Cv[e, 0, 1] / np.sqrt(Cv[e, 0, 0] * Cv[e, 1, 1])
        assert corr < -0.5, corr
    assert np.all(sig / s_cond > 1.5), sig / s_cond


def test_distant_pair_is_uncorrelated(ctx):
    n = 64
    sep = 10.0 * _psf_fwhm_data_px(make_roi_dataset(E=1, M=1, n=n, ss=2, seed=31)['psf'])
    assert sep < 0.75 * n, sep
    j = _pair(ctx, n, sep)
    try:
        F, Cv, sig = j.fisher_flux_covariance()
        s_cond = j.fisher_flux_sigma()
    finally:
        j.close()
    for e in range(2):
        corr = Cv[e, 0, 1] / np.sqrt(Cv[e, 0, 0] * Cv[e, 1, 1])
        assert abs(corr) < 1e-3, (sep, corr)
    assert np.allclose(sig, s_cond, rtol=1e-5)


@pytest.mark.parametrize('background', [True, False], ids=['fft', 'ps'])
def test_source_outside_the_stamp(ctx, background):
    """A third source far outside the stamp: F_ii = 0, sigma = inf, a zero row / column of C, and the other two sources'
    blocks as in a fit without it."""
    n, M, E = 24, 3, 3
    ds, p, sig2 = _problem(n, 2, M, 77, background, E=E)
    p['c_x'][2], p['c_y'][2] = 1000.0, -1000.0
    j = _joint(ctx, ds, sig2, p, 2, M)
    try:
        F, Cv, sig = j.fisher_flux_covariance()
        s_cond = j.fisher_flux_sigma()
    finally:
        j.close()
    p2 = dict(p, a=p['a'].reshape(E, M)[:, :2].ravel(), c_x=p['c_x'][:2], c_y=p['c_y'][:2])
    j2 = _joint(ctx, ds, sig2, p2, 2, 2)
    try:
        F2, C2, s2 = j2.fisher_flux_covariance()
    finally:
        j2.close()
    assert np.all(np.isinf(sig.reshape(E, M)[:, 2])) and np.all(np.isinf(s_cond.reshape(E, M)[:, 2]))
    assert np.all(F[:, 2, :] == 0) and np.all(F[:, :, 2] == 0)
    assert np.all(Cv[:, 2, :] == 0) and np.all(Cv[:, :, 2] == 0)
    assert np.allclose(F[:, :2, :2], F2, rtol=1e-6, atol=0)
    assert np.allclose(Cv[:, :2, :2], C2, rtol=1e-5, atol=0)
    assert np.allclose(sig.reshape(E, M)[:, :2].ravel(), s2, rtol=1e-5)


def test_singular_block_is_nan_and_the_call_succeeds(ctx):
    """Two sources at one position: every block is singular - NaN covariance and sigma, F finite."""
    n, M = 24, 2
    ds, p, sig2 = _problem(n, 2, M, 91, True, E=3)
    p['c_x'][1], p['c_y'][1] = p['c_x'][0], p['c_y'][0]
    j = _joint(ctx, ds, sig2, p, 2, M)
    try:
        F, Cv, sig = j.fisher_flux_covariance()
    finally:
        j.close()
    assert np.all(np.isfinite(F)) and np.all(F[:, 0, 0] > 0)
    assert np.all(np.isnan(Cv)) and np.all(np.isnan(sig))


def test_chunked_slab_equals_epoch_subsets(ctx):
    """300 epochs at n = 128, M = 8: the template slab (64 MiB) takes 128 epochs at a time, so three chunks; every output
    bit for bit that of separate objects over epoch subsets that do not follow the chunk boundaries."""
    from lightcurver_amd.joint import JointFit
    E, n, ss, M = 300, 128, 2, 8
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=5150, with_background=True)
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    sig2 = ds['noisemap'].astype(np.float64) ** 2

    def run(lo, hi):
        q = dict(p, a=p['a'][lo * M:hi * M], dx=p['dx'][lo:hi], dy=p['dy'][lo:hi], alpha=p['alpha'][lo:hi],
                 mean=p['mean'][lo:hi])
        j = JointFit(ds['data'][lo:hi], sig2[lo:hi], ds['psf'][lo:hi], ss, M, ctx)
        try:
            j.set_params(**q)
            j.set_free(['a'])
            return j.fisher_flux_covariance()
        finally:
            j.close()

    F, Cv, sig = run(0, E)
    bounds = [0, 100, 200, 300]
    parts = [run(lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])]
    assert np.array_equal(F, np.concatenate([q[0] for q in parts]))
    assert np.array_equal(Cv, np.concatenate([q[1] for q in parts]))
    assert np.array_equal(sig, np.concatenate([q[2] for q in parts]))
    assert np.all(np.isfinite(sig)) and np.all(sig > 0)


def _pad(x, p, fill=0.0):
    x = np.asarray(x)
    out = np.full((x.shape[0], x.shape[1] + 2 * p, x.shape[2] + 2 * p), fill, np.float64)
    out[:, p:-p, p:-p] = x
    return out


@pytest.mark.parametrize('n', [20, 28])
def test_embedded_sizes(ctx, n):
    """EmbeddedJointFit: bit for bit the padded native fit (the ring carries no weight), and the oracle at the caller's size."""
    from lightcurver_amd.joint import EmbeddedJointFit, JointFit, joint_fit_size
    ss, M = 2, 2
    ds, p, sig2 = _problem(n, ss, M, 300 + n, True, E=3)
    n_fit = joint_fit_size(n, ss)
    assert n_fit > n
    j = EmbeddedJointFit(ds['data'], sig2, ds['psf'], ss, M, ctx, n_fit)
    try:
        j.set_params(**p)
        j.set_free(['a'])
        F, Cv, sig = _check_against_oracle(j, ds, p, sig2, ss, M)
        big = JointFit(_pad(ds['data'], j.pad), _pad(sig2, j.pad, EmbeddedJointFit.RING_VARIANCE), j._psf_fit, ss, M, ctx)
        try:
            big.set_params(**dict(p, h=j._pad_h(p['h'])))
            big.set_free(['a'])
            Fb, Cb, sb = big.fisher_flux_covariance()
        finally:
            big.close()
    finally:
        j.close()
    assert np.array_equal(F, Fb) and np.array_equal(Cv, Cb) and np.array_equal(sig, sb)


@pytest.mark.parametrize('background,n,M', [(False, 16, 1), (False, 32, 2), (True, 24, 1), (True, 16, 2)])
def test_star_batch_blocks_equal_each_stars_own_fit(ctx, background, n, M):
    from lightcurver_amd.joint import JointFit, StarPhotometryBatch
    E_list = [4, 1, 6]
    stars = [make_roi_dataset(E=E, M=M, n=n, ss=2, seed=40 + g, with_background=background) for g, E in enumerate(E_list)]
    starts = []
    for ds in stars:
        p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
        if not background:
            p['h'] = np.zeros_like(p['h'])
        starts.append(p)
    single = []
    for ds, p in zip(stars, starts):
        j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], 2, M, ctx)
        j.set_params(**p)
        j.set_free(['a'])
        single.append(j.fisher_flux_covariance())
        j.close()
    b = StarPhotometryBatch([(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf']) for ds in stars], 2, M, ctx,
                            background=background)
    try:
        cat = {k: np.concatenate([p[k] for p in starts]) for k in ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha', 'mean')}
        cat['h'] = np.concatenate([p['h'] for p in starts]) if background else starts[0]['h']
        b.set_params(**cat)
        b.set_free(['a'])
        F, Cv, sig = b.fisher_flux_covariance()
        s_cond = b.fisher_flux_sigma()
    finally:
        b.close()
    for g, (Fs, Cs, ss_) in enumerate(single):
        e0, e1 = b.starts[g], b.starts[g + 1]
        assert np.array_equal(F[e0:e1], Fs), g
        assert np.array_equal(Cv[e0:e1], Cs), g
        assert np.array_equal(sig[e0 * M:e1 * M], ss_), g
    assert np.all(sig >= s_cond * (1 - 1e-6))


def test_facade_full_fisher(ctx):
    """FisherCovariance(diagonal_only=False) reached through setup_model / ParametersDeconv / Loss / Optimizer; the diagonal
    form unchanged; get_flux_covariance and flux_combination_sigma at the lightcurver level."""
    import warnings
    from copy import deepcopy
    from lightcurver_amd.starred.deconvolution.deconvolution import setup_model
    from lightcurver_amd.starred.deconvolution.loss import Loss
    from lightcurver_amd.starred.deconvolution.parameters import ParametersDeconv
    from lightcurver_amd.starred.optim.inference_base import FisherCovariance, block_diagonal
    from lightcurver_amd.starred.optim.optimization import Optimizer
    from lightcurver_amd.utilities.starred_utilities import (flux_combination_sigma, get_flux_covariance,
                                                             get_flux_uncertainties)
    E, M = 5, 3
    ds = make_roi_dataset(E=E, M=M, n=16, ss=2, seed=12)
    data, noise, s = ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64), ds['psf']
    t = ds['truth']
    model, k_init, k_up, k_down, k_fixed = setup_model(data, noise ** 2, s, t['c_x'], t['c_y'], 2, list(t['a']))
    frozen = deepcopy(k_init)
    frozen['kwargs_analytic'].pop('a')
    pars = ParametersDeconv(kwargs_init=k_init, kwargs_fixed=frozen, kwargs_up=k_up, kwargs_down=k_down)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        loss = Loss(data, model, pars, noise ** 2, regularization_terms='l1_starlet')
    optim = Optimizer(loss, pars, method='l-bfgs-b')
    full = FisherCovariance(pars, optim, diagonal_only=False)
    diag = FisherCovariance(pars, optim, diagonal_only=True)
    s_full = np.asarray(full.get_kwargs_sigma()['kwargs_analytic']['a'])
    s_diag = np.asarray(diag.get_kwargs_sigma()['kwargs_analytic']['a'])
    fit = loss.configure()
    fit.set_params(**pars._current)
    F, Cv, sig = fit.fisher_flux_covariance()
    assert np.array_equal(s_diag, fit.fisher_flux_sigma())
    assert np.array_equal(s_full, sig) and s_full.shape == (E * M,)
    assert np.all(s_full >= s_diag * (1 - 1e-6))
    assert np.array_equal(full.flux_covariance_blocks, Cv)
    assert full.covariance_matrix.shape == (E * M, E * M)
    assert np.array_equal(full.covariance_matrix, block_diagonal(Cv))
    assert np.array_equal(full.fisher_matrix, block_diagonal(F))
    with pytest.raises(NotImplementedError):
        diag.covariance_matrix
    cov = get_flux_covariance(deepcopy(k_init), k_up, k_down, data, noise, model, refine_iterations=3)
    assert cov.shape == (E, M, M) and np.all(np.isfinite(cov))
    su = get_flux_uncertainties(deepcopy(k_init), k_up, k_down, data, noise, model, refine_iterations=3)
    marg = np.sqrt(np.stack([np.diag(c) for c in cov]).ravel())
    assert np.all(marg >= su * (1 - 1e-5))
    w = np.array([1.0, 0.0, 1.0])
    comb = flux_combination_sigma(cov, w)
    assert comb.shape == (E,) and np.allclose(comb, [np.sqrt(w @ c @ w) for c in cov])


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def test_sharded_roi_fit_gathers_the_covariance(tmp_path):
    """model_roi_cutouts_sharded(return_flux_covariance=True) on two ranks sharing one GPU: the gathered fluxes_covariance
    equals, bit for bit, that of one object over all epochs at the gathered parameters (tests/_fisher_cov_worker.py)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_fisher_cov_worker.py')
    out = tmp_path / 'cov.npz'
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, worker, str(out)], env=env))
    codes = [pr.wait(timeout=600) for pr in procs]
    assert codes == [0, 0], codes
    g = np.load(out)
    E, M = 10, 2
    assert g['cov'].shape == (E, M, M) and g['sigma'].shape == (E * M,)
    assert np.array_equal(g['cov'], g['cov_one'])
    assert np.array_equal(g['sigma'], g['sigma_one'])
    assert np.all(np.sqrt(np.stack([np.diag(c) for c in g['cov']]).ravel()) >= g['sigma'] * (1 - 1e-6))
