"""Host side of the flux covariance from the full Fisher information: the combination error of a sum of fluxes, the dense
block-diagonal assembly of the STARRED facade, which free sets FisherCovariance accepts, and the C entry point's
declaration and binding (lc_joint_fisher_flux_cov)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_cov(rng, E, M):
    A = rng.standard_normal((E, M, M))
    return np.einsum('eij,ekj->eik', A, A) + 0.1 * np.eye(M)


def test_flux_combination_sigma_is_w_c_w():
    from lightcurver_amd.utilities.starred_utilities import flux_combination_sigma
    rng = np.random.default_rng(3)
    E, M = 7, 4
    cov = _random_cov(rng, E, M)
    w = np.array([1.0, 0.0, 0.0, 1.0])   # A + D of a four-image lens
    got = flux_combination_sigma(cov, w)
    assert got.shape == (E,)
    assert np.allclose(got, [np.sqrt(w @ cov[e] @ w) for e in range(E)], rtol=1e-14)
    # a single source: its own marginal error
    assert np.allclose(flux_combination_sigma(cov, [0, 1, 0, 0]), np.sqrt(cov[:, 1, 1]), rtol=1e-14)
    # the covariance matters: the sum of an anti-correlated pair is better determined than in quadrature
    c = np.array([[[1.0, -0.8], [-0.8, 1.0]]])
    assert flux_combination_sigma(c, [1, 1])[0] < np.sqrt(2.0)
    with pytest.raises(ValueError):
        flux_combination_sigma(cov, [1.0, 1.0])


def test_block_diagonal_assembly():
    from lightcurver_amd.starred.optim.inference_base import block_diagonal
    rng = np.random.default_rng(5)
    E, M = 4, 3
    blocks = _random_cov(rng, E, M).astype(np.float32)
    D = block_diagonal(blocks)
    assert D.shape == (E * M, E * M) and D.dtype == np.float32
    for e in range(E):
        for f in range(E):
            blk = D[e * M:(e + 1) * M, f * M:(f + 1) * M]
            assert np.array_equal(blk, blocks[e] if e == f else np.zeros((M, M), np.float32)), (e, f)
    # the inverse of the dense matrix is the dense matrix of the inverted blocks (epoch-major order of `a`)
    assert np.allclose(np.linalg.inv(D.astype(np.float64)), block_diagonal(np.linalg.inv(blocks.astype(np.float64))),
                       rtol=1e-4, atol=1e-6)


class _Params:
    def __init__(self, free):
        self.free = free
        self._current = {}


def test_facade_accepts_the_full_form_for_the_fluxes_only():
    from lightcurver_amd.starred.optim.inference_base import FisherCovariance
    full = FisherCovariance(_Params(['a']), None, diagonal_only=False)
    assert not full.diagonal_only
    assert FisherCovariance(_Params(['a']), None, diagonal_only=True).diagonal_only
    for free in (['a', 'dx'], ['h'], ['c_x']):
        for diag in (True, False):
            with pytest.raises(NotImplementedError):
                FisherCovariance(_Params(free), None, diagonal_only=diag)


def test_entry_point_is_declared_and_bound():
    from lightcurver_amd import _lib
    assert 'lc_joint_fisher_flux_cov' in _lib.SIGNATURES
    ret, args = _lib.SIGNATURES['lc_joint_fisher_flux_cov']
    assert len(args) == 4
    with open(os.path.join(ROOT, 'include', 'lcmi.h')) as f:
        header = f.read()
    assert re.search(r'int\s+lc_joint_fisher_flux_cov\s*\(\s*lc_joint\s*\*\s*j\s*,\s*float\s*\*\s*fisher\s*,\s*float\s*\*\s*cov\s*,'
                     r'\s*float\s*\*\s*sigma\s*\)\s*;', header)
    from lightcurver_amd.joint import JointFit, StarPhotometryBatch, EmbeddedJointFit
    for cls in (JointFit, StarPhotometryBatch, EmbeddedJointFit):
        assert callable(getattr(cls, 'fisher_flux_covariance', None)), cls


def test_sharded_roi_fit_takes_the_switch():
    import inspect
    from lightcurver_amd.processes.roi_modelling import model_roi_cutouts_sharded
    sig = inspect.signature(model_roi_cutouts_sharded)
    assert sig.parameters['return_flux_covariance'].default is False
