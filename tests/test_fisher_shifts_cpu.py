"""Host side of the Fisher information with the epochs' translations free: the arrowhead solve and the dense assembly with
the wider local block (a_e, mean_e, dx_e, dy_e) against numpy's inverse, the free sets FisherCovariance accepts, the gauge
between the positions and the shifts in the float64 oracle, the entry point's declaration, the Python switches - and a guard
that the problems of tests/test_fisher_shifts_gpu.py do test the background term of the dx, dy columns."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from lightcurver_amd.starred.optim.inference_base import (FisherCovariance, arrowhead_covariance, dense_from_arrowhead)
from tests import test_fisher_shifts_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrowhead(E, M, mean, seed, npix=60):
    """Blocks of J^T J for a random Jacobian with the arrowhead's structure: epoch e's pixels see a_e, mean_e, dx_e, dy_e and c."""
    rng = np.random.default_rng(seed)
    Lp, S = M + (1 if mean else 0) + 2, 2 * M
    Fl, Fx, Fs = np.zeros((E, Lp, Lp)), np.zeros((E, Lp, S)), np.zeros((S, S))
    for e in range(E):
        J = rng.standard_normal((npix, Lp + S)) * rng.uniform(0.5, 2.0, Lp + S)
        Gm = J.T @ J
        Fl[e], Fx[e] = Gm[:Lp, :Lp], Gm[:Lp, Lp:]
        Fs += Gm[Lp:, Lp:]
    return Fl, Fx, Fs


@pytest.mark.parametrize('M', [1, 3])
@pytest.mark.parametrize('mean', [False, True], ids=['Lp=M+2', 'Lp=M+3'])
@pytest.mark.parametrize('positions', [True, False])
def test_wider_local_block_against_the_dense_inverse(M, mean, positions):
    E = 4
    Fl, Fx, Fs = _arrowhead(E, M, mean, 100 + 10 * M + mean)
    if not positions:
        Fx = Fs = None
    Lp, S = M + mean + 2, (2 * M if positions else 0)
    D = dense_from_arrowhead(Fl, Fx, Fs, M, shifts=True)
    P = E * Lp + S
    assert D.shape == (P, P) and np.array_equal(D, D.T)
    # the dense order: a (epoch-major), c_x, c_y, mean, dx, dy
    first = E * M + S + (E if mean else 0)
    assert D[0, 0] == Fl[0, 0, 0] and D[first + 1, first + 1] == Fl[1, Lp - 2, Lp - 2]
    assert D[first + E + 2, first + E + 2] == Fl[2, Lp - 1, Lp - 1] and D[2 * M, first + 2] == Fl[2, 0, Lp - 2]
    assert D[first + 1, first + E + 1] == Fl[1, Lp - 2, Lp - 1] and D[first, first + 1] == 0   # epochs do not couple
    if mean:
        assert D[E * M + S + 3, first + E + 3] == Fl[3, M, Lp - 1]
    if positions:
        assert D[E * M + 1, first + 2] == Fx[2, Lp - 2, 1]
    res = arrowhead_covariance(Fl, Fx, Fs, shifts=True)
    C = dense_from_arrowhead(res['C_local'], res['C_cross'] if positions else None, res['C_shared'] if positions else None, M,
                             covariance=True, shifts=True)
    ref = np.linalg.inv(D)
    assert np.abs(C - ref).max() <= 1e-10 * np.linalg.cond(D) * np.abs(ref).max()
    sig = np.sqrt(np.diag(ref))
    assert np.allclose(res['sigma_local'][:, :M].ravel(), sig[:E * M], rtol=1e-10)
    assert np.allclose(res['sigma_local'][:, Lp - 2], sig[first:first + E], rtol=1e-10)
    assert np.allclose(res['sigma_local'][:, Lp - 1], sig[first + E:], rtol=1e-10)


def test_dense_form_needs_the_keyword():
    with pytest.raises(ValueError):
        dense_from_arrowhead(np.zeros((2, 5, 5)), None, None, 3)           # without the keyword: as before
    assert dense_from_arrowhead(np.zeros((2, 5, 5)), None, None, 3, shifts=True).shape == (10, 10)
    assert dense_from_arrowhead(np.zeros((2, 6, 6)), None, None, 3, shifts=True).shape == (12, 12)
    with pytest.raises(ValueError):
        dense_from_arrowhead(np.zeros((2, 7, 7)), None, None, 3, shifts=True)
    with pytest.raises(ValueError):
        dense_from_arrowhead(np.zeros((2, 4, 4)), None, None, 3, shifts=True)


class _Params:
    def __init__(self, free):
        self.free = free
        self._current = {}


def test_free_sets():
    for free in (['a', 'dx', 'dy'], ['a', 'dx', 'dy', 'mean'], ['a', 'c_x', 'c_y', 'dx', 'dy'],
                 ['a', 'c_x', 'c_y', 'dx', 'dy', 'mean']):
        for diag in (True, False):
            f = FisherCovariance(_Params(free), None, diagonal_only=diag)
            assert f._shifts and f._positions == ('c_x' in free) and f._mean == ('mean' in free)
    for free in (['a'], ['a', 'mean'], ['a', 'c_x', 'c_y'], ['a', 'c_x', 'c_y', 'mean']):
        assert not FisherCovariance(_Params(free), None)._shifts
    for free in (['a', 'dx'], ['a', 'dy'], ['dx', 'dy'], ['a', 'dx', 'dy', 'alpha'], ['a', 'dx', 'dy', 'h'], ['a', 'c_x', 'dx', 'dy'],
                 ['a', 'c_x'], ['c_x', 'c_y'], ['a', 'c_x', 'c_y', 'h'], ['mean']):
        with pytest.raises(NotImplementedError):
            FisherCovariance(_Params(free), None, diagonal_only=False)


def test_gauge_between_positions_and_shifts():
    """h = 0, M = 2 (the blend of DESIGN.md section 3): with c and the shifts free a common translation of the sources
    costs nothing - the oracle's information is singular, and the 0.05 px prior repairs it."""
    ds, p, sig2 = G._blend()
    p = dict(p, h=np.zeros_like(p['h']))
    E, M = 3, 2
    Fo = G._oracle_fisher(ds, p, sig2, 2)

    def cond(sigma_p):
        F, _ = G._select(Fo, E, M, True, False, sigma_p)
        d = np.sqrt(np.diag(F))
        return np.linalg.cond(F / np.outer(d, d))

    free, pinned = cond(None), cond(0.05)
    print(f'cond of the normalised information, a, c, dx, dy free: {free:.3g} without a prior, {pinned:.3g} with 0.05 px')
    assert free > 1e12 and pinned < 1e3


@pytest.mark.parametrize('n,ss,M', G.SIZES)
def test_background_term_is_being_tested(n, ss, M):
    """The with-background problems of the GPU tests: the oracle's normalised dx, dy entries with h and with h = 0 differ by
    at least 100 times the bound those entries are held to - an implementation without the background part fails there."""
    ds, p, sig2, Fo = G._case(n, ss, M)
    E = ds['data'].shape[0]
    Fz = G._oracle_fisher(ds, dict(p, h=np.zeros_like(p['h'])), sig2, ss)
    d = np.sqrt(np.diag(Fo))
    k0 = E * M + 2 * M + E
    diff = (np.abs(Fo - Fz) / np.outer(d, d))
    big = max(diff[k0:, :].max(), diff[:, k0:].max())
    print(f'n={n} ss={ss} M={M}: dx, dy entries with h against h = 0: {big:.3g}')
    assert big >= 100 * G.FS_BOUND, big


def test_entry_point_is_declared_and_bound():
    from lightcurver_amd import _lib
    from lightcurver_amd.joint import EmbeddedJointFit, JointFit, StarPhotometryBatch
    ret, args = _lib.SIGNATURES['lc_joint_fisher_shifts']
    assert ret is ctypes.c_int and len(args) == 3
    with open(os.path.join(ROOT, 'include', 'lcmi.h')) as f:
        header = f.read()
    assert re.search(r'int\s+lc_joint_fisher_shifts\s*\(\s*lc_joint\s*\*\s*j\s*,\s*int\s+flags\s*,\s*'
                     r'const\s+lc_fisher_shifts_out\s*\*\s*out\s*\)\s*;', header)
    m = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*lc_fisher_shifts_out\s*;', re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    fields = re.findall(r'\*\s*(\w+)', m.group(1))
    assert fields == [n for n, _ in _lib.FisherShiftsOut._fields_] == list(_lib.FISHER_SHIFTS_FIELDS)
    assert fields[-2:] == ['sigma_dx', 'sigma_dy'] and fields[:9] == list(_lib.FISHER_POSITIONS_FIELDS)
    assert ctypes.sizeof(_lib.FisherShiftsOut) == 11 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.FisherPositionsOut) == 9 * ctypes.sizeof(ctypes.c_void_p)
    assert 'gauge' in header
    assert EmbeddedJointFit.fisher_shifts is JointFit.fisher_shifts
    assert StarPhotometryBatch.fisher_shifts is not JointFit.fisher_shifts
    p = inspect.signature(JointFit.fisher_shifts).parameters
    assert p['positions'].default is False and p['mean'].default is False and p['prior'].default is None


def test_python_switches_and_their_defaults():
    from lightcurver_amd.processes import roi_modelling as R
    from lightcurver_amd.processes import star_photometry as S
    from lightcurver_amd.utilities import starred_utilities as U
    for fn in (R.model_roi_cutouts, R.model_roi_cutouts_sharded, R.fluxes_from_model, S.do_one_star_forward_modelling):
        assert inspect.signature(fn).parameters['marginalize_shifts'].default is False
    for fn in (U.get_flux_covariance, U.get_position_covariance):
        assert inspect.signature(fn).parameters['free_shifts'].default is False
    p = inspect.signature(U.get_shift_uncertainties).parameters
    assert p['free_positions'].default is False and p['free_mean'].default is False and p['prior'].default is None
    for fn in (arrowhead_covariance, dense_from_arrowhead):
        assert inspect.signature(fn).parameters['shifts'].default is False
    with pytest.raises(NotImplementedError):
        R.model_roi_cutouts_sharded(None, None, None, 2, [0.0], [0.0], [1.0], 1.0, marginalize_shifts=True)
    with pytest.raises(ValueError):       # positions and shifts free, no prior: the gauge
        R.model_roi_cutouts(np.zeros((2, 16, 16)), np.ones((2, 16, 16)), None, 2, [7.5], [7.5], marginalize_positions=True,
                            marginalize_shifts=True)
