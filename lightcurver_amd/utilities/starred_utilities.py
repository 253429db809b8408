"""Flux uncertainties from the diagonal Fisher information, the way the reference's
lightcurver/utilities/starred_utilities.py:10-39 obtains them from STARRED: every parameter except the
fluxes is frozen at its fitted value, the fluxes are polished by a few L-BFGS-B iterations and the
1-sigma is read off the Hessian diagonal of the chi2.  ``get_flux_covariance`` does the same and returns the
covariance of the fluxes of every epoch (the inverse of the full Fisher information, block diagonal over the
epochs), which ``flux_combination_sigma`` turns into the error of a sum of fluxes (blended images)."""
from copy import deepcopy

import numpy as np

from ..starred.deconvolution.loss import Loss
from ..starred.deconvolution.parameters import ParametersDeconv
from ..starred.optim.inference_base import FisherCovariance
from ..starred.optim.optimization import Optimizer


def _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations, diagonal_only):
    frozen = deepcopy(kwargs)
    frozen['kwargs_analytic'].pop('a')
    pars = ParametersDeconv(kwargs_init=kwargs, kwargs_fixed=frozen, kwargs_up=kwargs_up, kwargs_down=kwargs_down)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')  # "lambda is not normalized": h is frozen here, the term is a constant
        loss = Loss(data, model, pars, np.asarray(noisemap) ** 2, regularization_terms='l1_starlet')
    optim = Optimizer(loss, pars, method='l-bfgs-b')
    if refine_iterations > 0:
        optim.minimize(maxiter=int(refine_iterations))
    fisher = FisherCovariance(pars, optim, diagonal_only=diagonal_only)
    fisher.compute_fisher_information()
    return fisher


def get_flux_uncertainties(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations=10):
    """One uncertainty per entry of kwargs['kwargs_analytic']['a'] (same epoch-major order)."""
    fisher = _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations, True)
    return np.array(fisher.get_kwargs_sigma()['kwargs_analytic']['a'])


def get_flux_covariance(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations=10):
    """(E, M, M): the covariance of the M fluxes of every epoch, after the same L-BFGS-B polish of the fluxes as
    ``get_flux_uncertainties``.  Its diagonal is the square of the marginal 1-sigma (the flux's error with the other
    fluxes of its epoch free), which is at least that of ``get_flux_uncertainties`` (the others held fixed)."""
    fisher = _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, refine_iterations, False)
    return np.array(fisher.flux_covariance_blocks, dtype=np.float64)


def flux_combination_sigma(cov, weights):
    """1-sigma of sum_i weights[i] a_{e,i} in every epoch, sqrt(w^T C_e w), from the (E, M, M) covariance blocks.  For the
    sum of two blended images A and D (M = 4): weights = [1, 0, 0, 1]."""
    cov = np.asarray(cov, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if cov.ndim != 3 or cov.shape[1:] != (w.size, w.size):
        raise ValueError(f'cov must be (E, {w.size}, {w.size}) for {w.size} weights, got {cov.shape}')
    return np.sqrt(np.einsum('i,eij,j->e', w, cov, w))
