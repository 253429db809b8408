"""Host side of the Fisher information with the positions free: the float64 arrowhead solve (arrowhead_covariance) and the
dense assembly (dense_from_arrowhead) against numpy's inverse of the assembled matrix, the degenerate rules, the free sets
FisherCovariance accepts, and the entry point's declaration."""
import ctypes
import os
import re

import numpy as np
import pytest

from lightcurver_amd.starred.optim.inference_base import (FisherCovariance, arrowhead_covariance, dense_from_arrowhead)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrowhead(E, M, mean, seed, npix=40):
    """Blocks of J^T J for a random Jacobian with the arrowhead's structure: epoch e's pixels see a_e, mean_e and c."""
    rng = np.random.default_rng(seed)
    Lp, S = M + (1 if mean else 0), 2 * M
    Fl, Fx, Fs = np.zeros((E, Lp, Lp)), np.zeros((E, Lp, S)), np.zeros((S, S))
    for e in range(E):
        J = rng.standard_normal((npix, Lp + S)) * rng.uniform(0.5, 2.0, Lp + S)
        G = J.T @ J
        Fl[e], Fx[e] = G[:Lp, :Lp], G[:Lp, Lp:]
        Fs += G[Lp:, Lp:]
    return Fl, Fx, Fs


def _compare(Fl, Fx, Fs, M, keep=None):
    """arrowhead_covariance + dense_from_arrowhead against np.linalg.inv of the dense information (restricted to `keep`)."""
    D = dense_from_arrowhead(Fl, Fx, Fs, M)
    res = arrowhead_covariance(Fl, Fx, Fs)
    C = dense_from_arrowhead(res['C_local'], res['C_cross'], res['C_shared'], M, covariance=True)
    keep = np.arange(D.shape[0]) if keep is None else np.asarray(keep)
    Dk = D[np.ix_(keep, keep)]
    ref = np.linalg.inv(Dk)
    cond = np.linalg.cond(Dk)
    assert np.abs(C[np.ix_(keep, keep)] - ref).max() <= 1e-10 * cond * np.abs(ref).max(), cond
    gone = np.setdiff1d(np.arange(D.shape[0]), keep)
    assert np.all(C[gone] == 0) and np.all(C[:, gone] == 0)
    return res, C, ref


@pytest.mark.parametrize('M', [1, 3])
@pytest.mark.parametrize('mean', [False, True])
def test_arrowhead_solve_is_the_dense_inverse(M, mean):
    E = 4
    Fl, Fx, Fs = _arrowhead(E, M, mean, 10 * M + mean)
    D = dense_from_arrowhead(Fl, Fx, Fs, M)
    P = E * (M + mean) + 2 * M
    assert D.shape == (P, P) and np.array_equal(D, D.T)
    # the order of set_free: a (epoch-major), c_x, c_y, mean
    assert D[0, 0] == Fl[0, 0, 0] and D[E * M, E * M] == Fs[0, 0] and D[M, E * M + 1] == Fx[1, 0, 1]
    assert np.all(D[:M, M:2 * M] == 0)                      # different epochs do not couple
    if mean:
        assert D[E * M + 2 * M + 2, E * M + 2 * M + 2] == Fl[2, M, M] and D[2 * M, E * M + 2 * M + 2] == Fl[2, 0, M]
    res, C, ref = _compare(Fl, Fx, Fs, M)
    sig = np.sqrt(np.diag(ref))
    assert np.allclose(res['sigma_local'][:, :M].ravel(), sig[:E * M], rtol=1e-10)
    assert np.allclose(res['sigma_shared'], sig[E * M:E * M + 2 * M], rtol=1e-10)
    if mean:
        assert np.allclose(res['sigma_local'][:, M], sig[E * M + 2 * M:], rtol=1e-10)
    # cross-epoch flux covariance: B_e C_cc B_f^T
    B, Ccc = res['B'], res['C_shared']
    assert np.allclose(C[:M, M:2 * M], (B[0] @ Ccc @ B[1].T)[:M, :M], rtol=1e-9, atol=1e-14)


def test_positions_fixed_is_the_block_inverse():
    Fl, _, _ = _arrowhead(3, 2, True, 5)
    res = arrowhead_covariance(Fl, None, None)
    for e in range(3):
        assert np.allclose(res['C_local'][e], np.linalg.inv(Fl[e]), rtol=1e-10)
    assert res['C_shared'].shape == (0, 0) and res['sigma_shared'].shape == (0,)
    D = dense_from_arrowhead(res['C_local'], None, None, 2, covariance=True)
    assert D.shape == (9, 9) and np.allclose(D[:2, :2], res['C_local'][0][:2, :2])


def test_zeroed_local_parameter_is_left_out():
    E, M = 4, 3
    Fl, Fx, Fs = _arrowhead(E, M, True, 21)
    Fl[1, 2, :] = Fl[1, :, 2] = 0.0     # source 2 is not seen in epoch 1
    Fx[1, 2, :] = 0.0
    k = 1 * M + 2
    keep = [i for i in range(E * (M + 1) + 2 * M) if i != k]
    res, C, _ = _compare(Fl, Fx, Fs, M, keep)
    assert np.isinf(res['sigma_local'][1, 2]) and np.isfinite(np.delete(res['sigma_local'].ravel(), 1 * (M + 1) + 2)).all()
    assert np.all(res['C_local'][1, 2] == 0) and np.all(res['C_cross'][1, 2] == 0)


def test_zeroed_shared_parameter_and_its_rescue_by_a_prior():
    E, M = 4, 3
    Fl, Fx, Fs = _arrowhead(E, M, False, 22)
    Fx[:, :, 4] = 0.0                   # c_y of source 1 moves nothing
    Fs[4, :] = Fs[:, 4] = 0.0
    k = E * M + 4
    keep = [i for i in range(E * M + 2 * M) if i != k]
    res, _, _ = _compare(Fl, Fx, Fs, M, keep)
    assert np.isinf(res['sigma_shared'][4]) and np.isfinite(np.delete(res['sigma_shared'], 4)).all()
    sp = 0.05
    Fp = Fs.copy()
    Fp[4, 4] = 1.0 / sp ** 2            # the prior's 1 / sigma_p^2 on the diagonal of F_shared
    res, _, _ = _compare(Fl, Fx, Fp, M)
    assert np.isclose(res['sigma_shared'][4], sp, rtol=1e-12)


def test_failed_pivot_makes_every_covariance_nan():
    E, M = 4, 3
    Fl, Fx, Fs = _arrowhead(E, M, True, 23)
    # a duplicated column: source 1 of epoch 2 is source 0 again
    Fl[2, 1, :], Fl[2, :, 1] = Fl[2, 0, :].copy(), Fl[2, :, 0].copy()
    Fl[2, 1, 1] = Fl[2, 0, 0]
    Fx[2, 1] = Fx[2, 0]
    res = arrowhead_covariance(Fl, Fx, Fs)
    for k in ('C_local', 'C_cross', 'C_shared', 'sigma_local', 'sigma_shared'):
        assert np.all(np.isnan(res[k])), k
    assert np.all(np.isnan(dense_from_arrowhead(res['C_local'], res['C_cross'], res['C_shared'], M, covariance=True)))
    # ... and in the shared block: c_y of source 0 is c_x of source 0 again
    Fl, Fx, Fs = _arrowhead(E, M, True, 24)
    Fx[:, :, M] = Fx[:, :, 0]
    Fs[M, :], Fs[:, M] = Fs[0, :].copy(), Fs[:, 0].copy()
    Fs[M, M] = Fs[0, 0]
    res = arrowhead_covariance(Fl, Fx, Fs)
    assert np.all(np.isnan(res['C_local'])) and np.all(np.isnan(res['sigma_shared']))


def test_dense_form_refuses_beyond_4096_parameters():
    E, M = 1366, 3          # 1366 * 3 = 4098
    with pytest.raises(ValueError):
        dense_from_arrowhead(np.zeros((E, M, M)), None, None, M)
    with pytest.raises(ValueError):
        dense_from_arrowhead(np.zeros((2, 5, 5)), None, None, 3)


class _Params:
    def __init__(self, free):
        self.free = free
        self._current = {}


def test_free_sets():
    for free in (['a'], ['a', 'mean'], ['a', 'c_x', 'c_y'], ['a', 'c_x', 'c_y', 'mean']):
        for diag in (True, False):
            f = FisherCovariance(_Params(free), None, diagonal_only=diag)
            assert f.diagonal_only == diag
    for free in (['a', 'dx'], ['a', 'c_x'], ['c_x', 'c_y'], ['a', 'c_x', 'c_y', 'h'], ['mean']):
        with pytest.raises(NotImplementedError):
            FisherCovariance(_Params(free), None, diagonal_only=False)
    with pytest.raises(NotImplementedError):
        FisherCovariance(_Params(['a']), None, diagonal_only=False).position_covariance


def test_entry_point_is_declared_and_bound():
    from lightcurver_amd import _lib
    from lightcurver_amd.joint import EmbeddedJointFit, JointFit, StarPhotometryBatch
    ret, args = _lib.SIGNATURES['lc_joint_fisher_positions']
    assert ret is ctypes.c_int and len(args) == 3
    with open(os.path.join(ROOT, 'include', 'lcmi.h')) as f:
        header = f.read()
    assert re.search(r'int\s+lc_joint_fisher_positions\s*\(\s*lc_joint\s*\*\s*j\s*,\s*int\s+flags\s*,\s*'
                     r'const\s+lc_fisher_positions_out\s*\*\s*out\s*\)\s*;', header)
    m = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*lc_fisher_positions_out\s*;', re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    fields = re.findall(r'\*\s*(\w+)', m.group(1))
    assert fields == [n for n, _ in _lib.FisherPositionsOut._fields_] == list(_lib.FISHER_POSITIONS_FIELDS)
    assert ctypes.sizeof(_lib.FisherPositionsOut) == 9 * ctypes.sizeof(ctypes.c_void_p)
    for name, value in (('POSITIONS', 1), ('MEAN', 2), ('PRIOR', 4)):
        assert re.search(r'#define\s+LC_FISHER_%s\s+%d\b' % (name, value), header)
        assert getattr(_lib, 'FISHER_' + name) == value
    assert EmbeddedJointFit.fisher_positions is JointFit.fisher_positions
    assert StarPhotometryBatch.fisher_positions is not JointFit.fisher_positions


def test_roi_entry_points_take_the_switch():
    import inspect
    from lightcurver_amd.processes import roi_modelling as R
    from lightcurver_amd.utilities import starred_utilities as U
    for fn in (R.model_roi_cutouts, R.model_roi_cutouts_sharded, R.fluxes_from_model):
        assert inspect.signature(fn).parameters['marginalize_positions'].default is False
    p = inspect.signature(U.get_flux_covariance).parameters
    assert p['free_positions'].default is False and p['free_mean'].default is False and p['prior'].default is None
    assert callable(U.get_position_covariance)
    with pytest.raises(NotImplementedError):
        R.model_roi_cutouts_sharded(None, None, None, 2, [0.0], [0.0], [1.0], 1.0, marginalize_positions=True)
