"""``FisherCovariance`` for the use the reference makes of it - the 1-sigma of the fluxes with everything else fixed
(lightcurver/utilities/starred_utilities.py:36-38, ``diagonal_only=True``) - and its full form with only the fluxes free
(``diagonal_only=False``): the Fisher information of the fluxes is block diagonal over the epochs, each block M x M, and
the marginal 1-sigma comes from its inverse."""
import numpy as np

from ..deconvolution.deconvolution import nest_kwargs


def block_diagonal(blocks):
    """Dense (E * M, E * M) array with the (E, M, M) ``blocks`` on its diagonal, in the epoch-major order of ``a``."""
    blocks = np.asarray(blocks)
    E, M, _ = blocks.shape
    out = np.zeros((E * M, E * M), blocks.dtype)
    for e in range(E):
        out[e * M:(e + 1) * M, e * M:(e + 1) * M] = blocks[e]
    return out


class FisherCovariance:
    def __init__(self, param_class, optimizer_class, diagonal_only=True):
        if list(param_class.free) != ['a']:
            raise NotImplementedError("Fisher information is built for the fluxes 'a' only (the reference's use)")
        self._param = param_class
        self._optim = optimizer_class
        self.diagonal_only = bool(diagonal_only)
        self._sigma = None
        self._F = self._C = None

    def compute_fisher_information(self):
        fit = self._optim._loss.configure()
        fit.set_params(**self._param._current)
        if self.diagonal_only:
            self._sigma = fit.fisher_flux_sigma()
        else:
            self._F, self._C, self._sigma = fit.fisher_flux_covariance()

    def get_kwargs_sigma(self):
        """1-sigma of every free parameter in the nested kwargs shape: with ``diagonal_only=False`` the marginal errors
        sqrt(diag C), with ``diagonal_only=True`` 1 / sqrt(diag F)."""
        if self._sigma is None:
            self.compute_fisher_information()
        flat = {k: np.zeros_like(v) for k, v in self._param._current.items()}
        flat['a'] = self._sigma
        return nest_kwargs(flat)

    def _blocks(self):
        if self.diagonal_only:
            raise NotImplementedError('the full Fisher matrix needs diagonal_only=False')
        if self._F is None:
            self.compute_fisher_information()
        return self._F, self._C

    @property
    def flux_covariance_blocks(self):
        """(E, M, M): the covariance of the fluxes of every epoch (the epochs are independent)."""
        return self._blocks()[1]

    @property
    def fisher_matrix(self):
        """(E * M, E * M) Fisher information of the fluxes, dense, block diagonal over the epochs."""
        return block_diagonal(self._blocks()[0])

    @property
    def covariance_matrix(self):
        """(E * M, E * M) covariance of the fluxes, dense, block diagonal over the epochs."""
        return block_diagonal(self._blocks()[1])
