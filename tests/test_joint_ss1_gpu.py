"""The joint fit at subsampling 1 above the 16 x 16 fixture size: the epoch kernels of N = 24 ... 128 without the binned rows of
subsampling 2, the point-source-only kernel, noise propagation, Fisher information, trajectories (the cluster form at
n = 128 among them), the embedding of a size without a kernel, and PSF stamps of another side - each with the check and the
bounds the same quantity has at subsampling 2 (tests/test_joint_gpu.py, test_joint_sizes_gpu.py, test_fisher_positions_gpu.py,
test_fisher_shifts_gpu.py, test_joint_psf_size_gpu.py), against the float64 oracle."""
import numpy as np
import pytest

from oracle import model as om, optim as oo
from lightcurver_amd.synthetic import make_roi_dataset
from tests import helpers as H
from tests import test_joint_gpu as TJ
from tests import test_fisher_positions_gpu as FP
from tests import test_fisher_shifts_gpu as FS
from tests import test_fisher_covariance_gpu as FC
from tests import test_joint_psf_size_gpu as PS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('E,M,n,ss,alpha', [(3, 2, 32, 1, 0.0), (3, 2, 24, 1, 2.0), (2, 3, 64, 1, 0.3), (2, 2, 128, 1, 0.0),
                                            # the sizes beside them, as tests/test_joint_gpu.py has them at subsampling 2
                                            # (24, 40, 56: transforms over 8 lanes, run-time-N update; 24 also translated only)
                                            (3, 2, 24, 1, 0.0), (2, 2, 40, 1, 0.3), (2, 1, 48, 1, 0.0), (2, 2, 56, 1, 0.0)])
def test_model_loss_and_gradients(ctx, E, M, n, ss, alpha):
    """Every loss term on; alpha = 0 takes the 4-tap translation path, the others the ordered-gather T^T (their epochs are
    shifted as well: make_roi_dataset draws dx, dy for every epoch).  3e-5 model / chi2 / loss, 1e-4 gradients per block, 1e-5
    deconvolved scene."""
    TJ._check_model_loss_and_gradients(ctx, E, M, n, ss, alpha)


@pytest.mark.parametrize('n', [24, 32, 64, 128])
def test_no_background_path(ctx, n):
    """h == 0 and fixed: the separable point-source kernel (csrc/joint_ps.h) at every new N - one or two strips per thread
    under the four-wave limit (24, 32), four strips without it (64), the outputs through global memory (128)."""
    ss, E = 1, (5 if n < 128 else 2)
    ds, j, po, data, sig2, psf = TJ._setup(ctx, E, 1, n, ss, 5 + n, with_h=False)
    j.set_loss(lam_scales=3.0, lam_hf=3.0)
    free = ['a', 'c_x', 'c_y', 'dx', 'dy']
    j.set_free(free)
    L, g = oo.value_and_grad(lambda q: om.deconv_loss(q, data, sig2, psf, ss, lam_scales=3.0, lam_hf=3.0), po, free)
    loss, grads = j.loss_grad(free)
    model, chi2_e = j.model()
    j.close()
    mo = om.deconv_model(po, psf, ss, n)
    fig = dict(loss=abs(loss - L) / abs(L), model=H.rel_err(model, mo.numpy()), **{k: H.rel_err(grads[k], g[k].numpy()) for k in free})
    print(f'point sources only n={n}:', {k: '%.2e' % v for k, v in fig.items()})
    assert fig['loss'] < 3e-5 and fig['model'] < 3e-5
    for k in free:
        assert fig[k] < 1e-4, k


def test_no_background_path_two_sources(ctx):
    """Two sources: the filter outputs of every size go through the global scratch."""
    n, ss = 64, 1
    ds, j, po, data, sig2, psf = TJ._setup(ctx, 3, 2, n, ss, 71, with_h=False)
    free = ['a', 'c_x', 'c_y', 'dx', 'dy', 'mean']
    j.set_loss(lam_positivity_ps=5.0)
    j.set_free(free)
    L, g = oo.value_and_grad(lambda q: om.deconv_loss(q, data, sig2, psf, ss, lam_pos_ps=5.0), po, free)
    loss, grads = j.loss_grad(free)
    j.close()
    assert abs(loss - L) / abs(L) < 3e-5
    for k in free:
        assert H.rel_err(grads[k], g[k].numpy()) < 1e-4, k


@pytest.mark.parametrize('E,n,ss', [(3, 32, 1), (2, 64, 1),
                                    # the ek_aux build of the epoch kernel with transforms over 8 lanes
                                    (3, 24, 1), (2, 40, 1), (2, 56, 1)])
def test_noise_propagation_and_fisher(ctx, monkeypatch, E, n, ss):
    ds, j, po, data, sig2, psf = TJ._setup(ctx, E, 2, n, ss, 11 + n)
    monkeypatch.delenv('LCMI_NOISE_HOST', raising=False)
    W = j.propagate_noise()
    Wo = om.propagate_noise_deconv(sig2, psf, ss).numpy()
    assert W.shape == Wo.shape
    print(f'noise n={n}: W {H.rel_err(W, Wo):.2e}, per scale', ['%.2e' % H.rel_err(W[s], Wo[s]) for s in range(W.shape[0])])
    assert H.rel_err(W, Wo) < 1e-4
    for s in range(W.shape[0]):
        assert H.rel_err(W[s], Wo[s]) < 2e-4, s
    monkeypatch.setenv('LCMI_NOISE_HOST', '1')
    Wh = j.propagate_noise()
    monkeypatch.delenv('LCMI_NOISE_HOST')
    s = j.fisher_flux_sigma()
    j.close()
    so = om.fisher_flux_sigma(po, sig2, psf, ss).numpy()
    print(f'noise n={n}: host W {H.rel_err(Wh, Wo):.2e}, fisher_flux_sigma {H.rel_err(s, so):.2e}')
    assert H.rel_err(Wh, Wo) < 3e-5
    assert H.rel_err(s, so) < 3e-5


def _trajectory(ctx, E, M, n, ss, with_h, T, seed):
    """tests/test_joint_gpu.py::test_adabelief_trajectory at (E, T): the device run, the oracle's, and the figures."""
    ds, j, po, data, sig2, psf = TJ._setup(ctx, E, M, n, ss, seed, with_h=with_h)
    W = om.propagate_noise_deconv(sig2, psf, ss)
    free = ['a', 'c_x', 'c_y', 'dx', 'dy', 'mean'] + (['h'] if with_h else [])
    j.set_loss(W=W.numpy(), lam_scales=1.0, lam_hf=1.0, lam_positivity=10.0)
    j.set_free(free)
    j.run_adabelief(T, init_learning_rate=1e-3, schedule_learning_rate=True)
    info = j.cluster_info()          # (the form of the run's last epoch launch: asked before anything else launches one)
    hist, got = j.loss_history(), j.get_params()
    j.close()
    fn = lambda q: om.deconv_loss(q, data, sig2, psf, ss, W=W, lam_scales=1.0, lam_hf=1.0, lam_pos=10.0)
    pf, lh, l0 = oo.adabelief(fn, po, free, 1e-3, T, schedule=True)
    return hist, got, info, np.array([l0] + lh), pf


def _judge_trajectory(hist, got, ref, pf, T, with_h, tag):
    fig = dict(hist=np.abs(hist - ref).max() / np.abs(ref).max(), a=H.rel_err(got['a'], pf['a'].numpy()),
               c_x=np.abs(got['c_x'] - pf['c_x'].numpy()).max(), dx=np.abs(got['dx'] - pf['dx'].numpy()).max())
    if with_h:
        dh = np.abs(got['h'] - pf['h'].numpy())
        fig.update(dh_max=dh.max(), dh_med=np.median(dh))
    print(tag, {k: '%.2e' % v for k, v in fig.items()})
    assert hist.shape == (T + 1,)
    assert fig['hist'] < 2e-4 and fig['a'] < 2e-4 and fig['c_x'] < 5e-4 and fig['dx'] < 5e-4
    if with_h:
        assert fig['dh_max'] < 0.05 * T * 1e-3 and fig['dh_med'] < 1e-5


@pytest.mark.parametrize('n,ss,with_h', [(32, 1, True), (64, 1, True), (24, 1, False),
                                         # h free at the sizes of the run-time-N update (8-lane transforms)
                                         (24, 1, True), (40, 1, True), (56, 1, True)])
def test_adabelief_trajectory(ctx, n, ss, with_h):
    T = 25
    hist, got, info, ref, pf = _trajectory(ctx, 4, 2, n, ss, with_h, T, 40 + n)
    _judge_trajectory(hist, got, ref, pf, T, with_h, f'trajectory n={n} ss={ss}')


def test_adabelief_trajectory_at_128_in_both_forms(ctx, monkeypatch):
    """n = 128, two epochs, five iterations inside the device loop: the cluster form (six four-wave workgroups per epoch,
    what the object selects with so few epochs) and, with LCMI_CLUSTER=0, the one-workgroup kernel, each against the
    oracle's trajectory with the bounds above (the two differ in the order of the epoch sums: no bit equality)."""
    n, ss, E, M, T = 128, 1, 2, 2, 5
    monkeypatch.delenv('LCMI_CLUSTER', raising=False)
    hist, got, info, ref, pf = _trajectory(ctx, E, M, n, ss, True, T, 40 + n)
    assert info[0] >= 2 and info[1] == 0, info       # several workgroups per epoch, no fall-back
    _judge_trajectory(hist, got, ref, pf, T, True, f'trajectory n={n} cluster {info}')
    monkeypatch.setenv('LCMI_CLUSTER', '0')
    hist0, got0, info0, _, _ = _trajectory(ctx, E, M, n, ss, True, T, 40 + n)
    assert tuple(info0) == (0, 0)
    _judge_trajectory(hist0, got0, ref, pf, T, True, f'trajectory n={n} one workgroup')


# ---- embedding -------------------------------------------------------------------------------------------------------------
def _embedded_figures(ctx, n, ss, n_fit):
    """tests/test_joint_sizes_gpu.py::test_embedded_evaluation_is_the_native_size_one's figures: the embedded evaluation against
    the oracle at the caller's size, without the starlet term."""
    from lightcurver_amd.joint import make_joint_fit, EmbeddedJointFit, joint_fit_size
    E, M = 3, 2
    assert joint_fit_size(n, ss) == n_fit
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=300 + n)
    rng = np.random.default_rng(n)
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    p['a'] = p['a'] * rng.uniform(0.9, 1.1, p['a'].shape)
    p['dx'] = p['dx'] + rng.normal(0, 0.05, E)
    p['mean'] = rng.normal(0, 1e-3, E)
    p['h'] = p['h'] * rng.uniform(0.8, 1.2, p['h'].shape)
    sig2 = ds['noisemap'].astype(np.float64) ** 2
    j = make_joint_fit(ds['data'], sig2, ds['psf'], ss, M, ctx)
    assert isinstance(j, EmbeddedJointFit) and j.n == n and j.N == n * ss and j.sizes['h'] == (n * ss) ** 2
    j.set_params(**p)
    j.set_loss(lam_positivity=20.0, lam_positivity_ps=5.0, lam_flux_uniformity=0.7)
    free = ['a', 'c_x', 'c_y', 'dx', 'dy', 'h', 'mean']
    j.set_free(free)
    po = {k: om.T(v) for k, v in p.items()}
    data, s2, psf = om.T(ds['data']), om.T(sig2), om.T(ds['psf'])
    model, chi2_e = j.model()
    mo = om.deconv_model(po, psf, ss, n)
    assert model.shape == (E, n, n)
    L, g = oo.value_and_grad(lambda q: om.deconv_loss(q, data, s2, psf, ss, lam_pos=20.0, lam_pos_ps=5.0, lam_fu=0.7), po, free)
    loss, grads = j.loss_grad(free)
    j.close()
    for k in free:
        assert grads[k].shape == g[k].numpy().ravel().shape, k
    Nn = n * ss
    mg = 8 * ss // 2      # the margin of the subsampling-2 test (8 high-resolution pixels) in data pixels
    gh, gho = grads['h'].reshape(Nn, Nn), g['h'].numpy().reshape(Nn, Nn)
    return dict(model=H.rel_err(model, mo.numpy()), chi2=H.rel_err(chi2_e, (((data - mo) ** 2) / s2).sum((-1, -2)).numpy()),
                loss=abs(loss - L) / abs(L), grad=max(H.rel_err(grads[k], g[k].numpy()) for k in free if k != 'h'),
                grad_h=np.abs(gh - gho)[mg:-mg, mg:-mg].max() / np.abs(gho).max())


def test_embedded_evaluation_at_28(ctx):
    """n = 28 is fitted in 32 at either subsampling.  The yardstick is what the same evaluation measures at subsampling 2
    (tests/test_joint_sizes_gpu.py), with a factor 2 over it: the edge effects of the embedding - the background sampled with
    zeros beyond the window, the cut profile convolved back in - reach as many high-resolution pixels at subsampling 1, which
    are twice as many data pixels of the caller's stamp.  Both figures are printed (DESIGN.md section 7 records them)."""
    ref = _embedded_figures(ctx, 28, 2, 32)
    got = _embedded_figures(ctx, 28, 1, 32)
    print('embedded 28 -> 32 at ss = 2:', {k: '%.2e' % v for k, v in ref.items()})
    print('embedded 28 -> 32 at ss = 1:', {k: '%.2e' % v for k, v in got.items()})
    for k in ref:
        assert got[k] < 2.0 * ref[k], (k, got[k], ref[k])


# ---- Fisher information with positions / shifts free ---------------------------------------------------------------------------
def _normalised_error(dense, Fo):
    d = np.sqrt(np.diag(Fo))
    nrm = np.outer(d, d)
    return float(np.abs(dense / nrm - Fo / nrm).max())


def _positions_free(ctx, n):
    E, M, ss = 3, 2, 1
    ds, p, sig2 = FP._problem(n, ss, M, 900 + n + ss + M, True, E=E)
    Fo = FP._oracle_fisher(ds, p, sig2, ss)
    j = FP._joint(ctx, ds, sig2, p, ss, M)
    try:
        res = j.fisher_positions(positions=True, mean=True)
    finally:
        j.close()
    F = FP._select(Fo, E, M, True, True)
    err = _normalised_error(FP._dense(res, M, False), F)
    cond = float(np.linalg.cond(F / np.outer(np.sqrt(np.diag(F)), np.sqrt(np.diag(F)))))
    d = np.sqrt(np.diag(F))
    err_C = H.rel_err(FP._dense(res, M, True) * np.outer(d, d), np.linalg.inv(F / np.outer(d, d)))
    print(f'positions free n={n} ss={ss}: max|dF~| = {err:.3g}, cond = {cond:.3g}, rel_err C~ = {err_C:.3g}')
    assert err < 3e-5
    assert err_C < 3e-6 * cond + 1e-6


def test_fisher_with_positions_free(ctx):
    _positions_free(ctx, 32)


@pytest.mark.parametrize('n', [24, 56])
def test_fisher_with_positions_free_at_the_8_lane_sizes(ctx, n):
    _positions_free(ctx, n)


def _shifts_free(ctx, positions, n):
    E, M, ss = 3, 2, 1
    ds, p, sig2, Fo = _shift_case(n, ss, M)
    j = FS._joint(ctx, ds, sig2, p, ss, M, prior=FS._prior(p) if positions else None)
    try:
        res = j.fisher_shifts(positions=positions, mean=True)
    finally:
        j.close()
    FS._shapes(res, E, M, True, positions)
    F, is_shift = FS._select(Fo, E, M, positions, True, FS.SIGMA_P)
    err = _normalised_error(FS._dense(res, M, False), F)
    d = np.sqrt(np.diag(F))
    cond = float(np.linalg.cond(F / np.outer(d, d)))
    err_C = H.rel_err(FS._dense(res, M, True) * np.outer(d, d), np.linalg.inv(F / np.outer(d, d)))
    print(f'shifts free n={n} ss={ss} c={positions}: max|dF~| = {err:.3g}, cond = {cond:.3g}, rel_err C~ = {err_C:.3g}')
    assert err < 3e-5
    assert err_C < 3e-6 * cond + 1e-6


@pytest.mark.parametrize('positions', [False, True], ids=['c-fixed', 'c-prior'])
def test_fisher_with_shifts_free(ctx, positions):
    _shifts_free(ctx, positions, 32)


@pytest.mark.parametrize('n', [24, 56])
@pytest.mark.parametrize('positions', [False, True], ids=['c-fixed', 'c-prior'])
def test_fisher_with_shifts_free_at_the_8_lane_sizes(ctx, positions, n):
    _shifts_free(ctx, positions, n)


_SHIFT_CASES = {}


def _shift_case(n, ss, M):
    """One problem and its oracle information for both cases above, computed once and never modified."""
    if (n, ss, M) not in _SHIFT_CASES:
        ds, p, sig2 = FS._problem(n, ss, M, 900 + n + ss + M, True, E=3)
        Fo = FS._oracle_fisher(ds, p, sig2, ss)
        Fo.setflags(write=False)
        _SHIFT_CASES[(n, ss, M)] = (ds, p, sig2, Fo)
    return _SHIFT_CASES[(n, ss, M)]


def test_flux_covariance_with_a_background_at_24(ctx):
    """fisher_flux_covariance through the template mode of the 8-lane epoch kernel (h non-zero: the FFT pipeline) at n = 24,
    three sources, masked pixels, epochs at 0, 120 and 180 degrees: the comparison of tests/test_fisher_covariance_gpu.py
    (3e-5 on every block of F against the oracle's Hessian, 3e-6 cond + 1e-6 on its inverse)."""
    n, ss, M = 24, 1, 3
    ds, p, sig2 = FC._problem(n, ss, M, 700 + n + ss + M, True, E=3)
    Hm = FC._oracle_hessian(ds, p, sig2, ss)
    j = FC._joint(ctx, ds, sig2, p, ss, M)
    try:
        F, Cv, _ = j.fisher_flux_covariance()
        blocks = [Hm[e * M:(e + 1) * M, e * M:(e + 1) * M] for e in range(3)]
        print(f'flux covariance n={n} ss={ss}: F', ['%.2e' % H.rel_err(F[e], blocks[e]) for e in range(3)],
              'C', ['%.2e (cond %.3g)' % (H.rel_err(Cv[e], np.linalg.inv(blocks[e])), np.linalg.cond(blocks[e])) for e in range(3)])
        FC._check_against_oracle(j, ds, p, sig2, ss, M)
    finally:
        j.close()


# ---- PSF stamps of another side ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [24, 40])
def test_psf_stamps_of_another_side(ctx, P):
    """N = 32 at subsampling 1 with 24-wide stamps (placed exactly) and 40-wide ones (windowed to the grid)."""
    PS._check_model_loss_and_gradients(ctx, 3, 2, 32, 1, P)


@pytest.mark.parametrize('n,P', [(24, 32), (40, 24)])
def test_psf_stamps_of_another_side_at_the_8_lane_sizes(ctx, n, P):
    """The grids of the 8-lane transforms: N = 24 with 32-wide stamps (windowed), N = 40 with 24-wide ones (placed)."""
    PS._check_model_loss_and_gradients(ctx, 3, 2, n, 1, P)
