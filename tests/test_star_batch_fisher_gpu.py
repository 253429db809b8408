"""Fisher information of a batched star photometry with the epochs' shifts free (lc_joint_groups_fisher_shifts,
StarPhotometryBatch.fisher_shifts_per_star, do_many_stars_forward_modelling(marginalize_shifts=True)).  With every star's
position fixed the epochs do not couple, and the per-epoch arithmetic is that of lc_joint_fisher_shifts: every star of a batch
must give the bits of its own JointFit.  Then the float64 oracle Jacobian, a star across a chunk boundary, one singular star
among good ones, the refusals and NULL outputs, and the step function.
(Helpers and bounds: tests/test_fisher_shifts_gpu.py, unchanged.)"""
import ctypes
import functools

import numpy as np
import pytest

from lightcurver_amd.synthetic import make_roi_dataset
from tests.test_fisher_shifts_gpu import _check_against_oracle, _joint, _oracle_fisher, _problem, _select

pytestmark = pytest.mark.gpu

EPOCHS = (3, 1, 2)
PER_EPOCH = ('F_local', 'C_local', 'sigma_mean', 'sigma_dx', 'sigma_dy')
NAMES = ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha', 'mean')


@functools.lru_cache(maxsize=None)
def _stars(n, ss, M, background, epochs=EPOCHS):
    """One problem per star (rotations 0 / 120 / 180 degrees, non-integer shifts, a few masked pixels), made once."""
    return tuple(_problem(n, ss, M, 7000 + 10 * n + ss + M + 100 * g, background, E=E) for g, E in enumerate(epochs))


def _batch(ctx, stars, ss, M, background):
    from lightcurver_amd.joint import StarPhotometryBatch
    b = StarPhotometryBatch([(ds['data'], sig2, ds['psf']) for ds, _, sig2 in stars], ss, M, ctx, background=background)
    par = {k: np.concatenate([p[k] for _, p, _ in stars]) for k in NAMES}
    # (a batch without backgrounds holds one all-zero grid: _problem(background=False) has h = 0 for every star)
    par['h'] = np.concatenate([p['h'] for _, p, _ in stars]) if background else np.zeros(b.N * b.N)
    b.set_params(**par)
    return b


def _own(ctx, star, ss, M, mean):
    ds, p, sig2 = star
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        return j.fisher_shifts(mean=mean)
    finally:
        j.close()


def _part(b, res, g):
    """Star g's part of the concatenated result."""
    out = {k: b.split(res[k], k)[g] for k in PER_EPOCH if res[k].size}
    out['sigma_a'] = b.split(res['sigma_a'], 'a')[g]
    return out


def _assert_star_equals(b, res, g, own, label):
    part = _part(b, res, g)
    for k, v in part.items():
        assert v.shape == own[k].shape, (label, g, k, v.shape, own[k].shape)
        assert np.array_equal(v, own[k], equal_nan=True), (label, g, k)
    for k in ('F_cross', 'F_shared', 'C_cross', 'C_shared', 'sigma_c'):
        assert own[k].size == 0 and k not in res


CASES = [(16, 2, 1, False), (16, 1, 1, False), (24, 2, 2, False), (16, 2, 1, True), (24, 2, 2, True)]


@pytest.mark.parametrize('mean', [False, True], ids=['', 'mean'])
@pytest.mark.parametrize('n,ss,M,background', CASES)
def test_each_star_is_its_own_call(ctx, n, ss, M, background, mean):
    stars = _stars(n, ss, M, background)
    if background:
        assert all(np.any(p['h'] != 0) for _, p, _ in stars)
    b = _batch(ctx, stars, ss, M, background)
    try:
        res = b.fisher_shifts_per_star(mean=mean)
    finally:
        b.close()
    E, Lp = sum(EPOCHS), M + (1 if mean else 0) + 2
    assert res['F_local'].shape == res['C_local'].shape == (E, Lp, Lp)
    assert res['sigma_a'].shape == (E * M,) and res['sigma_dx'].shape == res['sigma_dy'].shape == (E,)
    assert res['sigma_mean'].shape == ((E,) if mean else (0,))
    assert res['star_ok'].dtype == bool and res['star_ok'].shape == (len(EPOCHS),) and res['star_ok'].all()
    for g, star in enumerate(stars):
        own = _own(ctx, star, ss, M, mean)
        assert all(np.all(np.isfinite(own[k])) for k in own)
        _assert_star_equals(b, res, g, own, (n, ss, M, background, mean))


@pytest.mark.parametrize('mean', [False, True], ids=['', 'mean'])
@pytest.mark.parametrize('n,ss,M', [(16, 2, 1), (24, 2, 2)])
def test_every_star_matches_the_oracle_jacobian(ctx, n, ss, M, mean):
    stars = _stars(n, ss, M, True)
    b = _batch(ctx, stars, ss, M, True)
    try:
        res = b.fisher_shifts_per_star(mean=mean)
    finally:
        b.close()
    for g, (ds, p, sig2) in enumerate(stars):
        E, Lp = EPOCHS[g], M + (1 if mean else 0) + 2
        part = _part(b, res, g)
        part.setdefault('sigma_mean', np.zeros(0, np.float32))
        part.update(F_cross=np.zeros((E, Lp, 0), np.float32), C_cross=np.zeros((E, Lp, 0), np.float32),
                    F_shared=np.zeros((0, 0), np.float32), C_shared=np.zeros((0, 0), np.float32), sigma_c=np.zeros(0, np.float32))
        F, is_shift = _select(_star_oracle(n, ss, M, g), E, M, False, mean)
        _check_against_oracle(part, F, is_shift, M, f'n={n} ss={ss} M={M} mean={mean} star {g}')


@functools.lru_cache(maxsize=None)
def _star_oracle(n, ss, M, g):
    ds, p, sig2 = _stars(n, ss, M, True)[g]
    Fo = _oracle_fisher(ds, p, sig2, ss)
    Fo.setflags(write=False)
    return Fo


def test_chunk_boundary_inside_a_star(ctx):
    """Three stars of 180 epochs at n = 32, ss = 2: 540 epochs, the slab takes 512, so the third star's epochs lie on both
    sides of the cut.  Every star's information is that of its own JointFit (one chunk each); two calls agree bit for bit."""
    from lightcurver_amd.joint import JointFit, StarPhotometryBatch
    n, ss, M, E = 32, 2, 1, 180
    stars = []
    for g in range(3):
        ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=8100 + g, with_background=True)
        p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
        stars.append((ds, p, ds['noisemap'].astype(np.float64) ** 2))
    b = _batch(ctx, stars, ss, M, True)
    try:
        res = b.fisher_shifts_per_star(mean=True)
        again = b.fisher_shifts_per_star(mean=True)
    finally:
        b.close()
    for k in res:
        assert np.array_equal(res[k], again[k], equal_nan=True), k
    assert res['star_ok'].all() and all(np.all(np.isfinite(res[k])) for k in res)
    for g, star in enumerate(stars):
        own = _own(ctx, star, ss, M, True)
        assert np.array_equal(b.split(res['F_local'], 'F_local')[g], own['F_local']), g
        _assert_star_equals(b, res, g, own, 'chunks')


@pytest.mark.parametrize('background', [False, True], ids=['', 'background'])
def test_one_bad_star_stays_alone(ctx, background):
    """Star 1's two sources at one position: duplicate columns, the pivot test fails in each of its epochs.  Only star 1 is
    NaN; a fully masked epoch of star 2 is left out (sigma = +inf) as in its own call."""
    n, ss, M, epochs = 16, 2, 2, (2, 3, 3)
    stars = [(ds, dict(p), sig2.copy()) for ds, p, sig2 in _stars(n, ss, M, background, epochs)]
    bad = stars[1][1]
    bad['c_x'] = np.full(M, bad['c_x'][0])
    bad['c_y'] = np.full(M, bad['c_y'][0])
    stars[2][2][1] = np.inf
    b = _batch(ctx, stars, ss, M, background)
    try:
        res = b.fisher_shifts_per_star(mean=True)
    finally:
        b.close()
    assert res['star_ok'].tolist() == [True, False, True]
    part = _part(b, res, 1)
    assert np.all(np.isfinite(part['F_local']))
    for k in ('C_local', 'sigma_a', 'sigma_mean', 'sigma_dx', 'sigma_dy'):
        assert np.all(np.isnan(part[k])), k
    for g in (0, 2):
        _assert_star_equals(b, res, g, _own(ctx, stars[g], ss, M, True), 'bad star')
    assert all(np.all(np.isfinite(v)) for v in _part(b, res, 0).values())
    last = _part(b, res, 2)
    assert np.all(last['F_local'][1] == 0) and np.all(last['C_local'][1] == 0)
    for k in ('sigma_mean', 'sigma_dx', 'sigma_dy'):
        assert np.isposinf(last[k][1]) and np.all(np.isfinite(last[k][[0, 2]])), k
    sa = last['sigma_a'].reshape(3, M)
    assert np.all(np.isposinf(sa[1])) and np.all(np.isfinite(sa[[0, 2]])) and np.all(np.isfinite(last['C_local']))


def test_refusals_leave_the_outputs_untouched(ctx):
    from lightcurver_amd import _lib
    n, ss, M = 16, 2, 1
    stars = _stars(n, ss, M, False)
    E, G = sum(EPOCHS), len(EPOCHS)
    lib = _lib.lib()

    def refused(obj, flags, code, match, **bufs):
        keep = {k: np.full(v, -7.0, np.float32) for k, v in bufs.items()}
        ok = np.full(G, -7, np.int32)
        out = _lib.FisherShiftsOut(**{k: _lib.ptr(v) for k, v in keep.items()})
        rc = lib.lc_joint_groups_fisher_shifts(obj.h, flags, ctypes.byref(out), ok.ctypes.data_as(_lib.ip))
        assert rc == code, (flags, rc, code)
        for k, v in keep.items():
            assert np.all(v == -7.0), k
        assert np.all(ok == -7)
        if match:
            with pytest.raises(_lib.LcError, match=match):
                obj._chk(rc, 'groups_fisher_shifts')

    b = _batch(ctx, stars, ss, M, False)
    try:
        refused(b, 8, -1, None, sigma_a=E * M)                               # LC_ERR_INVALID: an unknown flag
        for k, size in (('F_cross', 1), ('F_shared', 1), ('C_cross', 1), ('C_shared', 1), ('sigma_c', 2 * M)):
            refused(b, 2, -1, 'shared', sigma_a=E * M, **{k: size})          # a shared output
        refused(b, 0, -1, 'LC_FISHER_MEAN', sigma_mean=E, sigma_dy=E)        # sigma_mean without LC_FISHER_MEAN
        for flags in (1, 4, 5, 7):                                           # LC_ERR_UNSUPPORTED, and the message says both
            refused(b, flags, -3, 'no prior', sigma_a=E * M, sigma_dx=E)
            refused(b, flags, -3, 'singular', sigma_a=E * M, sigma_dx=E)
    finally:
        b.close()
    ds, p, sig2 = stars[0]
    j = _joint(ctx, ds, sig2, p, ss, M)
    try:
        refused(j, 0, -3, 'lc_joint_fisher_shifts', sigma_a=EPOCHS[0] * M, sigma_dx=EPOCHS[0])   # not a batched object
        assert not hasattr(j, 'fisher_shifts_per_star')
    finally:
        j.close()


@pytest.mark.parametrize('background', [False, True], ids=['', 'background'])
def test_null_outputs_and_the_object_afterwards(ctx, background):
    """Any subset of the outputs NULL: the same bits in the rest.  After the call the batch is the batch it was:
    fisher_flux_sigma() and five AdaBelief iterations give the bits of a fresh batch."""
    from lightcurver_amd import _lib
    n, ss, M = 16, 2, 1
    stars = _stars(n, ss, M, background)
    G = len(EPOCHS)
    lib = _lib.lib()

    def fit(b):
        sigma = b.fisher_flux_sigma()
        W = b.propagate_noise() if background else None
        b.set_loss(W=W, lam_scales=3.0, lam_hf=3.0)
        b.set_free(['a', 'c_x', 'c_y', 'dx', 'dy', 'mean'] + (['h'] if background else []))
        b.run_adabelief(5, init_learning_rate=1e-3)
        return dict(b.get_params(), sigma=sigma, hist=b.loss_history())

    fresh = _batch(ctx, stars, ss, M, background)
    try:
        want = fit(fresh)
    finally:
        fresh.close()
    b = _batch(ctx, stars, ss, M, background)
    try:
        res = b.fisher_shifts_per_star(mean=True)
        given_sets = ([], ['sigma_dy'], ['F_local', 'sigma_dx'], ['C_local', 'sigma_a', 'sigma_mean'], ['star_ok'],
                      ['F_local', 'C_local', 'sigma_a', 'sigma_mean', 'sigma_dx', 'sigma_dy', 'star_ok'])
        for given in given_sets:
            bufs = {k: np.full_like(res[k], -7.0) for k in given if k != 'star_ok'}
            ok = np.full(G, -7, np.int32) if 'star_ok' in given else None
            out = _lib.FisherShiftsOut(**{k: _lib.ptr(v) for k, v in bufs.items()})
            rc = lib.lc_joint_groups_fisher_shifts(b.h, 2, ctypes.byref(out), None if ok is None else ok.ctypes.data_as(_lib.ip))
            assert rc == 0, given
            for k, v in bufs.items():
                assert np.array_equal(v, res[k]), (given, k)
            if ok is not None:
                assert np.array_equal(ok, np.ones(G, np.int32)), given
        with pytest.raises(NotImplementedError):
            b.fisher_shifts()
        with pytest.raises(NotImplementedError):
            b.fisher_positions()
        got = fit(b)
    finally:
        b.close()
    for k in want:
        assert np.array_equal(want[k], got[k]), k


def _flat(k_final):
    both = {**k_final['kwargs_analytic'], **k_final['kwargs_background']}
    return {k: np.asarray(both[k]) for k in NAMES + ('h',)}


@pytest.mark.parametrize('n,sky,starlet', [(16, False, False), (16, True, False), (20, False, False), (20, True, False),
                                           (16, False, True)],
                         ids=['n16', 'n16-sky', 'n20', 'n20-sky', 'n16-starlet'])
def test_step_function_marginalises_the_shifts(ctx, n, sky, starlet):
    """Three stars, 5 / 3 / 4 epochs, 50 iterations: the existing keys as they were, and beside them the marginal errors -
    those of a JointFit (an EmbeddedJointFit at n = 20) set to the star's final parameters."""
    from lightcurver_amd.joint import EmbeddedJointFit, JointFit, joint_fit_size
    from lightcurver_amd.processes.star_photometry import do_many_stars_forward_modelling
    ss, epochs = 2, (5, 3, 4)
    sets = [make_roi_dataset(E=E, M=1, n=n, ss=ss, seed=8300 + n + g) for g, E in enumerate(epochs)]

    def run(**kw):
        stacks = [(ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64), ds['psf']) for ds in sets]
        return stacks, do_many_stars_forward_modelling(stacks, ss, n_iter=50, uniform_background_per_epoch=sky,
                                                       starlet_global_background=starlet, **kw)

    _, base = run()
    stacks, out = run(marginalize_shifts=True)       # (data and noise map rescaled in place: what the fit saw)
    n_fit = joint_fit_size(n, ss)
    assert n_fit == (16 if n == 16 else 24)
    for g, (old, new) in enumerate(zip(base, out)):
        assert 'fluxes_uncertainties_marginal' not in old and set(new) == set(old) | {'fluxes_uncertainties_marginal'}
        for k, v in old.items():
            if k == 'kwargs_final':
                for grp in v:
                    for name, w in v[grp].items():
                        assert np.array_equal(np.asarray(w), np.asarray(new[k][grp][name])), (g, name)
            else:
                assert np.array_equal(np.asarray(v), np.asarray(new[k]), equal_nan=True), (g, k)
        m = new['fluxes_uncertainties_marginal']
        assert m.shape == (epochs[g],) and m.dtype == np.float64 and np.all(np.isfinite(m))
        assert np.all(m >= new['fluxes_uncertainties'] * (1 - 1e-5)), (g, m, new['fluxes_uncertainties'])
        data, noisemap, psf = stacks[g]
        j = JointFit(data, noisemap ** 2, psf, ss, 1, ctx) if n_fit == n else EmbeddedJointFit(data, noisemap ** 2, psf, ss, 1, ctx, n_fit)
        try:
            j.set_params(**_flat(new['kwargs_final']))
            C = j.fisher_shifts(mean=sky)['C_local']
        finally:
            j.close()
        assert np.array_equal(m, new['scale'] * np.sqrt(np.array(C[:, 0, 0], dtype=np.float64))), (g, m)
