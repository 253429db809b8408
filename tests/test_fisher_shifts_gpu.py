"""Fisher information with the epochs' translations free (lc_joint_fisher_shifts, JointFit.fisher_shifts): theta = (a, dx,
dy[, mean][, c_x, c_y]), alpha and h fixed.  The oracle is the forward-mode Jacobian of the float64
oracle.model.deconv_model with respect to (a, c_x, c_y, mean, dx, dy) and J^T W J; information and covariance are compared
in normalised form (F / sqrt(d d^T), d = diag F_oracle).  Then the floor-cell convention on the knots, the decoupling of an
isolated star, the blend the shifts hurt most, the device solve against its host restatement, the prior, a masked epoch,
determinism and chunking, the existing call left as it was, an embedded size, the refusals and the facade.
(The helpers are those of tests/test_fisher_positions_gpu.py, copied and widened.)"""
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
SHIFTS = [(0.15, -0.35), (1.3, -0.7), (-2.1, 1.6)]   # data pixels; none an integer in high-resolution pixels
KNOTS = [(0.0, 0.0), (1.3, -0.7), (-2.1, 1.6)]       # epoch 0 (alpha = 0) exactly on the knots
NAMES = ('a', 'c_x', 'c_y', 'mean', 'dx', 'dy')      # the dense order
F_BOUND = 1.4e-6     # the blocks that exist without the shifts (tests/test_fisher_positions_gpu.py)
# Rows and columns of dx, dy, normalised: four times the largest deviation from the float64 oracle measured on MI355X over
# the sizes below, 3.66e-7 at n = 16, ss = 1 ("Test bounds that differ from ...": the table per size, with the
# float32 run of the same oracle Jacobian beside it, 2.8e-7 ... 1.3e-6).
FS_BOUND = 1.5e-6
SIGMA_P = 0.05


def _problem(n, ss, M, seed, background, E=3, mask_frac=0.05, shifts=SHIFTS):
    """Dataset at the rotations / shifts above, float32-rounded parameters, a few masked pixels per epoch (sigma2 = inf
    for the device, weight 0 for the oracle)."""
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=seed, alpha=ALPHAS[:E], with_background=background,
                          dx=[s[0] for s in shifts[:E]], dy=[s[1] for s in shifts[:E]])
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


def _prior(p, sigma_p=SIGMA_P):
    M = p['c_x'].size
    return {'c_x_mean': p['c_x'], 'c_x_sigma': np.full(M, sigma_p), 'c_y_mean': p['c_y'], 'c_y_sigma': np.full(M, sigma_p)}


def _oracle_fisher(ds, p, sig2, ss):
    """J^T W J of the float64 oracle in the order a (E M), c_x, c_y, mean (E), dx (E), dy (E); forward-mode Jacobian."""
    E, n, _ = ds['data'].shape
    po = {k: om.T(v) for k, v in p.items()}
    psf = om.T(ds['psf'])
    fn = lambda *v: om.deconv_model({**po, **dict(zip(NAMES, v))}, psf, ss, n)
    J = torch.autograd.functional.jacobian(fn, tuple(po[k] for k in NAMES), vectorize=True, strategy='forward-mode')
    J = np.concatenate([j.reshape(E * n * n, -1).numpy() for j in J], axis=1)
    s2 = sig2.astype(np.float32).astype(np.float64)  # (the device holds sigma2 in float32)
    w = np.where(np.isfinite(s2), 1.0 / np.where(np.isfinite(s2), s2, 1.0), 0.0).reshape(-1)
    return J.T @ (w[:, None] * J)


SIZES = [(16, 1, 2), (16, 2, 3), (24, 2, 4), (40, 2, 3), (64, 2, 8), (128, 2, 2)]


@functools.lru_cache(maxsize=None)
def _case(n, ss, M, background=True, knots=False):
    """One problem per size and its oracle information (every block free), computed once and never modified."""
    E = 2 if n == 128 else 3
    ds, p, sig2 = _problem(n, ss, M, 900 + n + ss + M, background, E=E, shifts=KNOTS if knots else SHIFTS)
    Fo = _oracle_fisher(ds, p, sig2, ss)
    Fo.setflags(write=False)
    return ds, p, sig2, Fo


def _select(Fo, E, M, positions, mean, sigma_p=None):
    """The oracle's information of the free set (order a, c_x, c_y, mean, dx, dy), prior added; and which of its
    parameters are shifts."""
    k0 = E * M + 2 * M
    keep = list(range(E * M)) + (list(range(E * M, k0)) if positions else []) + (list(range(k0, k0 + E)) if mean else []) \
        + list(range(k0 + E, k0 + 3 * E))
    F = np.array(Fo[np.ix_(keep, keep)])
    if sigma_p is not None and positions:
        for k in range(E * M, k0):
            F[k, k] += 1.0 / sigma_p ** 2
    return F, np.array(keep) >= k0 + E


def _dense(res, M, covariance):
    k = 'C' if covariance else 'F'
    S = res[k + '_shared']
    return dense_from_arrowhead(res[k + '_local'], res[k + '_cross'] if S.size else None, S if S.size else None, M,
                                covariance=covariance, shifts=True)


def _sigma_dense(res):
    return np.concatenate([res['sigma_a'], res['sigma_c'], res['sigma_mean'], res['sigma_dx'], res['sigma_dy']]).astype(np.float64)


def _check_against_oracle(res, Fo, is_shift, M, label):
    """Information of the blocks that exist without the shifts within F_BOUND, the rows and columns of dx, dy within
    FS_BOUND, covariance and sigma within 3e-6 cond + 1e-6, all in normalised form; returns the measured figures."""
    d = np.sqrt(np.diag(Fo))
    nrm = np.outer(d, d)
    Fn = Fo / nrm
    dF = np.abs(_dense(res, M, False) / nrm - Fn)
    sh = is_shift[:, None] | is_shift[None, :]
    err_F, err_S = float(dF[~sh].max()), float(dF[sh].max())
    cond = float(np.linalg.cond(Fn))
    Cn = np.linalg.inv(Fn)
    err_C = H.rel_err(_dense(res, M, True) * nrm, Cn)
    err_s = float(np.max(np.abs(_sigma_dense(res) * d / np.sqrt(np.diag(Cn)) - 1.0)))
    print(f'{label}: max|dF~| = {err_F:.3g}, shifts {err_S:.3g}, cond = {cond:.3g}, rel_err C~ = {err_C:.3g}, sigma = {err_s:.3g}')
    assert err_F < F_BOUND, (label, err_F)
    assert err_S < FS_BOUND, (label, err_S)
    assert err_C < 3e-6 * cond + 1e-6, (label, cond, err_C)
    assert err_s < 3e-6 * cond + 1e-6, (label, cond, err_s)
    return err_F, err_S, cond, err_C


def _shapes(res, E, M, mean, positions):
    Lp, Sh = M + (1 if mean else 0) + 2, (2 * M if positions else 0)
    assert res['F_local'].shape == res['C_local'].shape == (E, Lp, Lp)
    assert res['F_cross'].shape == res['C_cross'].shape == (E, Lp, Sh)
    assert res['F_shared'].shape == res['C_shared'].shape == (Sh, Sh)
    assert res['sigma_a'].shape == (E * M,) and res['sigma_c'].shape == (Sh,)
    assert res['sigma_mean'].shape == ((E,) if mean else (0,))
    assert res['sigma_dx'].shape == res['sigma_dy'].shape == (E,)


def _run(ctx, case, ss, M, mean, positions, label):
    ds, p, sig2, Fo = case
    E = ds['data'].shape[0]
    j = _joint(ctx, ds, sig2, p, ss, M, prior=_prior(p) if positions else None)
    try:
        res = j.fisher_shifts(positions=positions, mean=mean)
    finally:
        j.close()
    _shapes(res, E, M, mean, positions)
    F, is_shift = _select(Fo, E, M, positions, mean, SIGMA_P)
    return _check_against_oracle(res, F, is_shift, M, label)


@pytest.mark.parametrize('n,ss,M', SIZES)
@pytest.mark.parametrize('mean', [False, True], ids=['', 'mean'])
@pytest.mark.parametrize('positions', [False, True], ids=['c-fixed', 'c-prior'])
def test_native_sizes_match_the_oracle_jacobian(ctx, n, ss, M, mean, positions):
    _run(ctx, _case(n, ss, M), ss, M, mean, positions, f'n={n} ss={ss} M={M} mean={mean} c={positions}')


def test_epoch_on_the_knots(ctx):
    """alpha = 0, dx = dy = 0: the sample positions are the knots themselves, exact in float32, and the derivative is the
    forward difference of the cell floor selects."""
    n, ss, M = 16, 2, 3
    _run(ctx, _case(n, ss, M, knots=True), ss, M, True, True, 'on the knots')


def _flux_block(res, M):
    return res['C_local'][:, :M, :M].astype(np.float64)


def test_isolated_star_decouples(ctx):
    """M = 1, h = 0: fluxes and shifts decouple, the flux covariance is that with the shifts fixed.  The profile is even
    about the star and its derivative odd, so their weighted product sums to zero - for weights that are even too: the
    variance is uniform here and nothing is masked, at n = 32, where the wings cut by the stamp's edge no longer count
    (oracle: 5e-7 of the covariance; with the signal-dependent noise map of the other tests 1e-3, at n = 16 1e-2)."""
    n, ss, M, E = 32, 2, 1, 3
    ds, p, sig2 = _problem(n, ss, M, 41, False, E=E, mask_frac=0.0)
    sig2 = np.full_like(sig2, float(np.median(sig2)))
    F, _ = _select(_oracle_fisher(ds, p, sig2, ss), E, M, False, False)
    d = np.sqrt(np.diag(F))
    cond = np.linalg.cond(F / np.outer(d, d))
    tol = 3e-6 * cond + 1e-6
    oracle = H.rel_err(np.linalg.inv(F)[:E, :E], np.linalg.inv(F[:E, :E]))
    assert oracle < tol / 3, oracle             # the problem itself decouples
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        res = j.fisher_shifts()
        fixed = j.fisher_positions(positions=False)
    finally:
        j.close()
    err = max(H.rel_err(_flux_block(res, M)[e], _flux_block(fixed, M)[e]) for e in range(E))
    print(f'isolated star: C_local of the fluxes, shifts free against fixed: {err:.3g} (oracle {oracle:.3g}), cond {cond:.3g}')
    assert err < tol, (err, cond)


def _blend():
    """The M = 2 blend of DESIGN.md section 3 (make_roi_dataset(E=3, M=2, n=16, ss=2, seed=5) at the rotations and shifts above)."""
    ds = make_roi_dataset(E=3, M=2, n=16, ss=2, seed=5, alpha=ALPHAS, with_background=True,
                          dx=[s[0] for s in SHIFTS], dy=[s[1] for s in SHIFTS])
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    return ds, p, ds['noisemap'].astype(np.float64) ** 2


def test_blend_pays_for_the_shifts(ctx):
    ds, p, sig2 = _blend()
    j = _joint(ctx, ds, sig2, p, 2, 2)
    try:
        free = j.fisher_shifts()['sigma_a']
        fixed = j.fisher_positions(positions=False)['sigma_a']
    finally:
        j.close()
    ratio = free / fixed
    print(f'blend: sigma(a) shifts free / fixed = {ratio}')
    assert np.all(free >= fixed * (1 - 1e-6))
    assert ratio.max() > 2.0, ratio      # oracle: 4.77 / 1.65


@pytest.mark.parametrize('n,ss,M,mean,positions', [(16, 2, 3, True, True), (24, 2, 4, False, False), (64, 2, 8, True, True)])
def test_device_solve_is_the_host_restatement(ctx, n, ss, M, mean, positions):
    ds, p, sig2, _ = _case(n, ss, M)
    j = _joint(ctx, ds, sig2, p, ss, M, prior=_prior(p) if positions else None)
    try:
        res = j.fisher_shifts(positions=positions, mean=mean)
    finally:
        j.close()
    sh = res['F_shared'].size > 0
    ref = arrowhead_covariance(res['F_local'], res['F_cross'] if sh else None, res['F_shared'] if sh else None, shifts=True)
    Fd = _dense(res, M, False)
    d = np.sqrt(np.diag(Fd))
    cond = np.linalg.cond(Fd / np.outer(d, d))
    tol = 3e-6 * cond + 1e-6
    for k in ('C_local', 'C_cross', 'C_shared'):
        if res[k].size:
            assert H.rel_err(res[k], ref[k]) < tol, (k, H.rel_err(res[k], ref[k]), tol)
    assert np.allclose(res['sigma_a'], ref['sigma_local'][:, :M].ravel(), rtol=tol)
    assert np.allclose(res['sigma_c'], ref['sigma_shared'], rtol=tol)
    assert np.allclose(res['sigma_dx'], ref['sigma_local'][:, -2], rtol=tol)
    assert np.allclose(res['sigma_dy'], ref['sigma_local'][:, -1], rtol=tol)
    if mean:
        assert np.allclose(res['sigma_mean'], ref['sigma_local'][:, M], rtol=tol)


def test_prior_enters_the_shared_block(ctx):
    n, ss, M = 24, 2, 4
    ds, p, sig2, Fo = _case(n, ss, M)
    E = ds['data'].shape[0]
    j = _joint(ctx, ds, sig2, p, ss, M, prior=_prior(p, 0.02))
    try:
        res = j.fisher_shifts(positions=True)      # prior=None: used, because one is set
        fixed = j.fisher_shifts()
    finally:
        j.close()
    F, is_shift = _select(Fo, E, M, True, False, 0.02)
    _check_against_oracle(res, F, is_shift, M, 'prior 0.02')
    F0, _ = _select(Fo, E, M, True, False)
    k = np.arange(E * M, E * M + 2 * M)
    added = np.diag(_dense(res, M, False))[k] - np.diag(F0)[k]
    assert np.allclose(added, 1.0 / 0.02 ** 2, rtol=1e-4), added
    assert fixed['F_shared'].size == 0 and np.array_equal(fixed['F_local'], res['F_local'])


def test_masked_epoch_is_left_out(ctx):
    n, ss, M, E = 16, 2, 3, 3
    ds, p, sig2 = _problem(n, ss, M, 63, True, E=E)
    sig2[1] = np.inf
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        res = j.fisher_shifts(mean=True)
    finally:
        j.close()
    for k in ('sigma_dx', 'sigma_dy', 'sigma_mean'):
        assert np.isinf(res[k][1]) and np.all(np.isfinite(res[k][[0, 2]])), (k, res[k])
    sa = res['sigma_a'].reshape(E, M)
    assert np.all(np.isinf(sa[1])) and np.all(np.isfinite(sa[[0, 2]]))
    assert np.all(res['F_local'][1] == 0) and np.all(res['C_local'][1] == 0)


def test_chunks_and_determinism(ctx):
    """150 epochs at n = 64: the slab takes 128 epochs, so two chunks.  Two calls agree bit for bit; the epochs' blocks do
    not depend on where the chunks are cut; NULL outputs in any combination."""
    from lightcurver_amd import _lib
    from lightcurver_amd.joint import JointFit
    E, n, ss, M = 150, 64, 2, 2
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=5151, with_background=True)
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    sig2 = ds['noisemap'].astype(np.float64) ** 2

    def make(lo, hi):
        q = dict(p, a=p['a'][lo * M:hi * M], dx=p['dx'][lo:hi], dy=p['dy'][lo:hi], alpha=p['alpha'][lo:hi],
                 mean=p['mean'][lo:hi])
        j = JointFit(ds['data'][lo:hi], sig2[lo:hi], ds['psf'][lo:hi], ss, M, ctx)
        j.set_params(**q)
        j.set_loss(prior=_prior(p))
        return j

    j = make(0, E)
    try:
        res = j.fisher_shifts(positions=True, mean=True)
        again = j.fisher_shifts(positions=True, mean=True)
        lib, names = _lib.lib(), _lib.FISHER_SHIFTS_FIELDS
        for given in ([], ['sigma_dy'], ['F_local', 'C_cross', 'sigma_dx'], ['C_shared', 'sigma_a', 'sigma_mean']):
            bufs = {k: np.full_like(res[k], -7.0) for k in given}
            out = _lib.FisherShiftsOut(*[_lib.ptr(bufs.get(k)) for k in names])
            assert lib.lc_joint_fisher_shifts(j.h, 7, ctypes.byref(out)) == 0, given
            for k in given:
                assert np.array_equal(bufs[k], res[k]), k
    finally:
        j.close()
    for k in res:
        assert np.array_equal(res[k], again[k], equal_nan=True), k
    for k in ('sigma_a', 'sigma_c', 'sigma_dx', 'sigma_dy', 'sigma_mean'):
        assert np.all(np.isfinite(res[k])), k
    parts = []
    for lo, hi in ((0, 70), (70, E)):
        jp = make(lo, hi)
        try:
            parts.append(jp.fisher_shifts(positions=True, mean=True))
        finally:
            jp.close()
    for k in ('F_local', 'F_cross'):
        assert np.array_equal(res[k], np.concatenate([q[k] for q in parts])), k


def test_existing_call_is_unchanged(ctx):
    """fisher_positions after a fisher_shifts call on the same object: the bits of a fresh object."""
    n, ss, M = 24, 2, 4
    ds, p, sig2, _ = _case(n, ss, M)
    fresh = _joint(ctx, ds, sig2, p, ss, M)
    try:
        want = fresh.fisher_positions(mean=True)
    finally:
        fresh.close()
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        j.fisher_shifts(mean=True)
        got = j.fisher_positions(mean=True)
    finally:
        j.close()
    for k in want:
        assert np.array_equal(want[k], got[k], equal_nan=True), k


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
    assert n_fit == 24
    j = EmbeddedJointFit(ds['data'], sig2, ds['psf'], ss, M, ctx, n_fit)
    try:
        j.set_params(**p)
        res = j.fisher_shifts(mean=True)
        big = JointFit(_pad(ds['data'], j.pad), _pad(sig2, j.pad, EmbeddedJointFit.RING_VARIANCE), j._psf_fit, ss, M, ctx)
        try:
            big.set_params(**dict(p, h=j._pad_h(p['h'])))
            ref = big.fisher_shifts(mean=True)
        finally:
            big.close()
    finally:
        j.close()
    _shapes(res, E, M, True, False)
    for k in res:
        assert np.array_equal(res[k], ref[k]), k


def test_refusals_leave_the_outputs_untouched(ctx):
    from lightcurver_amd import _lib
    from lightcurver_amd.joint import StarPhotometryBatch
    n, ss, M = 16, 2, 3
    ds, p, sig2, _ = _case(n, ss, M)
    E = ds['data'].shape[0]
    lib = _lib.lib()

    def refused(h, flags, code, **bufs):
        keep = {k: np.full(v, -7.0, np.float32) for k, v in bufs.items()}
        out = _lib.FisherShiftsOut(**{k: _lib.ptr(v) for k, v in keep.items()})
        assert lib.lc_joint_fisher_shifts(h, flags, ctypes.byref(out)) == code, (flags, code)
        for k, v in keep.items():
            assert np.all(v == -7.0), k

    b = StarPhotometryBatch([(ds['data'], sig2, ds['psf'])], ss, M, ctx)
    try:
        with pytest.raises(NotImplementedError):
            b.fisher_shifts()
        refused(b.h, 0, -3, sigma_a=E * M, sigma_dx=E)            # LC_ERR_UNSUPPORTED: a batched object
    finally:
        b.close()
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        refused(j.h, 8, -1, sigma_a=E * M)                        # LC_ERR_INVALID: an unknown flag
        refused(j.h, 2, -1, sigma_c=2 * M, sigma_dx=E)            # a shared output with the positions fixed
        refused(j.h, 0, -1, sigma_mean=E, sigma_dy=E)             # sigma_mean without LC_FISHER_MEAN
        refused(j.h, 4, -1, sigma_a=E * M)                        # LC_FISHER_PRIOR without LC_FISHER_POSITIONS
        refused(j.h, 5, -3, sigma_a=E * M, sigma_dx=E)            # LC_FISHER_PRIOR, no prior in the loss
        refused(j.h, 1, -3, sigma_a=E * M, sigma_c=2 * M)         # the gauge: positions free without a prior
        with pytest.raises(_lib.LcError, match='gauge'):
            j.fisher_shifts(positions=True)
        j.set_loss(prior=_prior(p))
        refused(j.h, 1, -3, sigma_a=E * M, sigma_c=2 * M)         # ... and with a prior set but not asked for
        res = j.fisher_shifts(positions=True)
        for k in ('sigma_a', 'sigma_c', 'sigma_dx', 'sigma_dy'):
            assert np.all(np.isfinite(res[k])), k
    finally:
        j.close()


def test_facade(ctx):
    """FisherCovariance(free = a, dx, dy[, ...]) through setup_model / ParametersDeconv / Loss / Optimizer and the
    lightcurver-level helpers: the new entries, and the defaults unchanged."""
    import warnings
    from copy import deepcopy
    from lightcurver_amd.starred.deconvolution.deconvolution import setup_model
    from lightcurver_amd.starred.deconvolution.loss import Loss, Prior
    from lightcurver_amd.starred.deconvolution.parameters import ParametersDeconv
    from lightcurver_amd.starred.optim.inference_base import FisherCovariance
    from lightcurver_amd.starred.optim.optimization import Optimizer
    from lightcurver_amd.utilities.starred_utilities import (get_flux_covariance, get_position_covariance,
                                                             get_shift_uncertainties)
    E, M = 5, 3
    ds = make_roi_dataset(E=E, M=M, n=16, ss=2, seed=12)
    data, noise, s = ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64), ds['psf']
    t = ds['truth']
    model, k_init, k_up, k_down, k_fixed = setup_model(data, noise ** 2, s, t['c_x'], t['c_y'], 2, list(t['a']))
    prior = Prior(prior_analytic=[['c_x', t['c_x'], 0.05], ['c_y', t['c_y'], 0.05]])

    def fisher(free, prior=None, diagonal_only=False):
        frozen = deepcopy(k_init)
        for k in free:
            frozen['kwargs_analytic' if k != 'mean' else 'kwargs_background'].pop(k)
        pars = ParametersDeconv(kwargs_init=k_init, kwargs_fixed=frozen, kwargs_up=k_up, kwargs_down=k_down)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            loss = Loss(data, model, pars, noise ** 2, regularization_terms='l1_starlet', prior=prior)
        return FisherCovariance(pars, Optimizer(loss, pars, method='l-bfgs-b'), diagonal_only=diagonal_only)

    s0 = np.asarray(fisher(['a']).get_kwargs_sigma()['kwargs_analytic']['a'])
    full = fisher(['a', 'dx', 'dy'])
    sig = full.get_kwargs_sigma()['kwargs_analytic']
    sa, sdx, sdy = (np.asarray(sig[k]) for k in ('a', 'dx', 'dy'))
    assert sa.shape == (E * M,) and sdx.shape == sdy.shape == (E,)
    assert np.all(np.isfinite(sa)) and np.all(sdx > 0) and np.all(sdy > 0) and np.all(np.isfinite(sdx + sdy))
    assert np.all(sa >= s0 * (1 - 1e-6))
    P = E * M + 2 * E
    Fm, Cm = full.fisher_matrix, full.covariance_matrix
    assert Fm.shape == Cm.shape == (P, P)
    d = np.sqrt(np.diag(Fm))
    cond = np.linalg.cond(Fm / np.outer(d, d))
    assert H.rel_err(Cm * np.outer(d, d), np.linalg.inv(Fm / np.outer(d, d))) < 3e-6 * cond + 1e-6
    assert np.allclose(np.sqrt(np.diag(Cm))[E * M:], np.concatenate([sdx, sdy]), rtol=1e-6)
    assert full.flux_covariance_blocks.shape == (E, M, M)
    sd = fisher(['a', 'dx', 'dy'], diagonal_only=True).get_kwargs_sigma()['kwargs_analytic']
    assert np.allclose(np.asarray(sd['dx']), 1.0 / np.sqrt(np.diag(Fm)[E * M:E * M + E]), rtol=1e-6)
    everything = fisher(['a', 'c_x', 'c_y', 'dx', 'dy', 'mean'], prior=prior)
    assert everything.fisher_matrix.shape == (P + 2 * M + E, P + 2 * M + E)
    assert everything.position_covariance.shape == (2 * M, 2 * M)
    sm = np.asarray(everything.get_kwargs_sigma()['kwargs_background']['mean'])
    assert sm.shape == (E,) and np.all(sm > 0) and np.all(np.isfinite(sm))
    from lightcurver_amd import _lib
    with pytest.raises(_lib.LcError, match='gauge'):           # the positions beside the shifts, no prior
        fisher(['a', 'c_x', 'c_y', 'dx', 'dy']).compute_fisher_information()

    args = (k_up, k_down, data, noise, model)
    cov0 = get_flux_covariance(deepcopy(k_init), *args, refine_iterations=3)
    again = get_flux_covariance(deepcopy(k_init), *args, refine_iterations=3, free_shifts=False)
    cov1 = get_flux_covariance(deepcopy(k_init), *args, refine_iterations=3, free_shifts=True)
    cov2 = get_flux_covariance(deepcopy(k_init), *args, refine_iterations=3, free_shifts=True, free_positions=True, prior=prior)
    assert np.array_equal(cov0, again)
    assert cov2.shape == cov1.shape == cov0.shape == (E, M, M) and np.all(np.isfinite(cov1)) and np.all(np.isfinite(cov2))
    d0, d1, d2 = (np.stack([np.diag(c) for c in cv]) for cv in (cov0, cov1, cov2))
    assert np.all(d1 >= d0 * (1 - 1e-6)) and np.all(d2 >= d1 * (1 - 1e-6))
    sx, sy = get_shift_uncertainties(deepcopy(k_init), *args, refine_iterations=3)
    assert sx.shape == sy.shape == (E,) and np.all(sx > 0) and np.all(sy > 0) and np.all(np.isfinite(sx + sy))
    cc, scx, scy = get_position_covariance(deepcopy(k_init), *args, refine_iterations=3, prior=prior, free_shifts=True)
    cf, _, _ = get_position_covariance(deepcopy(k_init), *args, refine_iterations=3, prior=prior)
    assert cc.shape == (2 * M, 2 * M) and np.all(np.diag(cc) >= np.diag(cf) * (1 - 1e-6)) and np.all(scx <= 0.05 * (1 + 1e-6))


def test_roi_fit_marginalises_the_shifts(ctx):
    """The ROI fit at 5 x 16 x 16, M = 3 with marginalize_shifts: the new entries, and the default unchanged."""
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

    base, out, both = fit(), fit(marginalize_shifts=True), fit(marginalize_shifts=True, marginalize_positions=True)
    assert 'shift_uncertainties' not in base and 'fluxes_sigma' not in base
    for k in ('kwargs_analytic', 'kwargs_background'):      # the fit itself is unchanged
        for name, v in base['kwargs_final'][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(out['kwargs_final'][k][name])), name
            assert np.array_equal(np.asarray(v), np.asarray(both['kwargs_final'][k][name])), name
    for res in (out, both):
        su = res['shift_uncertainties']
        assert su['dx_sigma'].shape == su['dy_sigma'].shape == (E,)
        assert np.all(su['dx_sigma'] > 0) and np.all(su['dy_sigma'] > 0) and np.all(np.isfinite(su['dx_sigma'] + su['dy_sigma']))
        assert res['fluxes_sigma'].shape == (E * M,) and np.all(np.isfinite(res['fluxes_sigma']))
    assert 'astrometry_uncertainties' not in out and both['astrometry_uncertainties']['covariance'].shape == (2 * M, 2 * M)
    assert np.all(both['fluxes_sigma'] >= out['fluxes_sigma'] * (1 - 1e-6))
    args = (out['model'], out['kwargs_final'], out['kwargs_up'], out['kwargs_down'], out['data'], out['noisemap'], M,
            out['scale'], np.zeros(E))
    f0 = fluxes_from_model(*args)
    f1 = fluxes_from_model(*args, marginalize_shifts=True)
    f2 = fluxes_from_model(*args, marginalize_shifts=True, marginalize_positions=True,
                           prior=Prior(prior_analytic=[['c_x', xs - off, np.full(M, 0.5)], ['c_y', ys - off, np.full(M, 0.5)]]))
    assert 'shift_uncertainties' not in f0 and 'astrometry_uncertainties' not in f1 and 'astrometry_uncertainties' in f2
    assert f1['d_fluxes'].shape == f0['d_fluxes'].shape == (M, E) and np.all(np.isfinite(f1['d_fluxes']))
    assert np.all(f1['d_fluxes'] >= f0['d_fluxes'] * (1 - 1e-6)) and np.all(f2['d_fluxes'] >= f1['d_fluxes'] * (1 - 1e-6))
    assert np.array_equal(f1['fluxes'], f0['fluxes'])
    assert f1['shift_uncertainties']['dx_sigma'].shape == (E,)
    with pytest.raises(NotImplementedError):
        model_roi_cutouts_sharded(ds['data'], ds['noisemap'], ds['psf'], ss, xs, ys, list(t['a'][:M]), 1.0,
                                  marginalize_shifts=True)


def test_star_photometry_marginalises_the_shifts(ctx):
    """One star at 5 x 16 x 16, 50 iterations: the existing keys as they are, and the marginal errors beside them."""
    from lightcurver_amd.processes.star_photometry import do_one_star_forward_modelling
    E, n, ss = 5, 16, 2
    ds = make_roi_dataset(E=E, M=1, n=n, ss=ss, seed=3)

    def run(**kw):
        return do_one_star_forward_modelling(ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64), ds['psf'], ss,
                                             n_iter=50, **kw)

    for sky in (False, True):
        base = run(uniform_background_per_epoch=sky)
        out = run(uniform_background_per_epoch=sky, marginalize_shifts=True)
        assert 'fluxes_uncertainties_marginal' not in base
        for k, v in base.items():
            if k == 'kwargs_final':
                for grp in ('kwargs_analytic', 'kwargs_background'):
                    for name, w in v[grp].items():
                        assert np.array_equal(np.asarray(w), np.asarray(out[k][grp][name])), name
            else:
                assert np.array_equal(np.asarray(v), np.asarray(out[k]), equal_nan=True), k
        m = out['fluxes_uncertainties_marginal']
        assert m.shape == (E,) and np.all(np.isfinite(m)) and np.all(m >= out['fluxes_uncertainties'] * (1 - 1e-5))
