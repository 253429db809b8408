"""Flux uncertainties from the diagonal Fisher information, the way the reference's
lightcurver/utilities/starred_utilities.py:10-39 obtains them from STARRED: every parameter except the
fluxes is frozen at its fitted value, the fluxes are polished by a few L-BFGS-B iterations and the
1-sigma is read off the Hessian diagonal of the chi2.  ``get_flux_covariance`` does the same and returns the
covariance of the fluxes of every epoch (the inverse of the full Fisher information, block diagonal over the
epochs), which ``flux_combination_sigma`` turns into the error of a sum of fluxes (blended images).  With
``free_positions`` (and ``free_mean``) the source positions c_x, c_y (the epochs' constants) are free in the information as
well - ``FisherCovariance`` with those blocks free, conditional on dx, dy, alpha and h - and the covariances are marginal
over them; ``get_position_covariance`` returns that of the positions.  With ``free_shifts`` the epochs' translations dx, dy
are free in the information too (``JointFit.fisher_shifts``; conditional on alpha and h only), ``get_shift_uncertainties``
returns their 1-sigma; the positions beside the shifts need the ``prior``.  The L-BFGS-B polish stays on the fluxes."""
import warnings
from copy import deepcopy

import numpy as np

from ..starred.deconvolution.loss import Loss
from ..starred.deconvolution.parameters import ParametersDeconv
from ..starred.optim.inference_base import FisherCovariance
from ..starred.optim.optimization import Optimizer


def _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations, diagonal_only,
                     free_positions=False, free_mean=False, prior=None, free_shifts=False):
    frozen = deepcopy(kwargs)
    frozen['kwargs_analytic'].pop('a')
    pars = ParametersDeconv(kwargs_init=kwargs, kwargs_fixed=frozen, kwargs_up=kwargs_up, kwargs_down=kwargs_down)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')  # "lambda is not normalized": h is frozen here, the term is a constant
        loss = Loss(data, model, pars, np.asarray(noisemap) ** 2, regularization_terms='l1_starlet')
    optim = Optimizer(loss, pars, method='l-bfgs-b')
    if refine_iterations > 0:
        optim.minimize(maxiter=int(refine_iterations))
    if free_positions or free_mean or free_shifts:  # the information at the polished fluxes, with the further blocks free
        best = deepcopy(pars.best_fit_values(as_kwargs=True)) if refine_iterations > 0 else deepcopy(kwargs)
        frozen = deepcopy(best)
        frozen['kwargs_analytic'].pop('a')
        if free_positions:
            frozen['kwargs_analytic'].pop('c_x')
            frozen['kwargs_analytic'].pop('c_y')
        if free_mean:
            frozen['kwargs_background'].pop('mean')
        if free_shifts:
            frozen['kwargs_analytic'].pop('dx')
            frozen['kwargs_analytic'].pop('dy')
        pars = ParametersDeconv(kwargs_init=best, kwargs_fixed=frozen, kwargs_up=kwargs_up, kwargs_down=kwargs_down)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            loss = Loss(data, model, pars, np.asarray(noisemap) ** 2, regularization_terms='l1_starlet', prior=prior)
        optim = Optimizer(loss, pars, method='l-bfgs-b')
    fisher = FisherCovariance(pars, optim, diagonal_only=diagonal_only)
    fisher.compute_fisher_information()
    return fisher


def get_flux_uncertainties(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations=10):
    """One uncertainty per entry of kwargs['kwargs_analytic']['a'] (same epoch-major order)."""
    fisher = _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations, True)
    return np.array(fisher.get_kwargs_sigma()['kwargs_analytic']['a'])


def get_flux_covariance(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations=10,
                        free_positions=False, free_mean=False, prior=None, free_shifts=False):
    """(E, M, M): the covariance of the M fluxes of every epoch, after the same L-BFGS-B polish of the fluxes as
    ``get_flux_uncertainties``.  Its diagonal is the square of the marginal 1-sigma (the flux's error with the other
    fluxes of its epoch free), which is at least that of ``get_flux_uncertainties`` (the others held fixed).
    ``free_positions`` / ``free_mean``: marginal over c_x, c_y / the epochs' constants as well (``prior``: the ``Prior`` on
    c_x, c_y of the fit, which then enters the information); conditional on dx, dy, alpha and h.  ``free_shifts``: marginal
    over the epochs' translations dx, dy too (with ``free_positions`` only under a ``prior``)."""
    fisher = _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations, False,
                              free_positions, free_mean, prior, free_shifts)
    return np.array(fisher.flux_covariance_blocks, dtype=np.float64)


def position_covariance_of(fisher):
    """(cov (2M, 2M), sigma_c_x (M), sigma_c_y (M)) of a ``FisherCovariance`` with the positions free."""
    cov = np.array(fisher.position_covariance, dtype=np.float64)
    sig = np.sqrt(np.diag(cov))
    M = sig.size // 2
    return cov, sig[:M], sig[M:]


def get_position_covariance(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations=10, free_mean=False,
                            prior=None, free_shifts=False):
    """(cov (2M, 2M), sigma_c_x (M), sigma_c_y (M)): the marginal covariance of the source positions (c_x, then c_y; data
    pixels) with the fluxes (and with ``free_mean`` the epochs' constants) free, dx, dy, alpha and h fixed - with
    ``free_shifts`` dx, dy free as well, which needs the ``prior``."""
    fisher = _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations, False, True,
                              free_mean, prior, free_shifts)
    return position_covariance_of(fisher)


def get_shift_uncertainties(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations=10,
                            free_positions=False, free_mean=False, prior=None):
    """(sigma_dx (E), sigma_dy (E)): the marginal 1-sigma of the epochs' translations (data pixels) with the fluxes free
    (and the positions under their ``prior`` / the epochs' constants), alpha and h fixed."""
    fisher = _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations, False,
                              free_positions, free_mean, prior, True)
    sig = fisher.get_kwargs_sigma()['kwargs_analytic']
    return np.array(sig['dx'], dtype=np.float64), np.array(sig['dy'], dtype=np.float64)


def flux_combination_sigma(cov, weights):
    """1-sigma of sum_i weights[i] a_{e,i} in every epoch, sqrt(w^T C_e w), from the (E, M, M) covariance blocks.  For the
    sum of two blended images A and D (M = 4): weights = [1, 0, 0, 1]."""
    cov = np.asarray(cov, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if cov.ndim != 3 or cov.shape[1:] != (w.size, w.size):
        raise ValueError(f'cov must be (E, {w.size}, {w.size}) for {w.size} weights, got {cov.shape}')
    return np.sqrt(np.einsum('i,eij,j->e', w, cov, w))
