"""The joint fit's resampling T_e (rotation by alpha, shift by (dx, dy), bilinear interpolation with replicated edges) and
its adjoint at the geometry production fits have: alpha = angles_to_north - angles_to_north[0] from plate solving
(roi_modelling.py), 180 degrees for half the frames after a German-mount pier flip, any angle in an alt-az field, and
shifts of several pixels.  Every kernel form that runs the adjoint (phase D of the epoch kernel: the one-workgroup kernels,
the n = 64 cluster form, the phased global-spectrum launches) against the float64 oracle.

Tolerances as in test_joint_gpu.py: 3e-5 on models, chi2 per epoch and losses, 1e-4 on every gradient relative to its
largest element - and on the two-pixel border ring of dL/dh relative to the ring's own largest element: the ring collects
every clamped sample, and an error there hides under the interior's scale.

Rotated epochs keep the fractional part of ss * dx and ss * dy away from an integer: the interpolant has a kink there and
the dx / dy gradients are one-sided (fp32 cosf(90 deg) is -4.4e-8, not 0).  Exact integer and half-pixel shifts are taken
on the translated path only, where fp32 and fp64 compute the sample positions exactly."""
import numpy as np
import pytest

from oracle import model as om, optim as oo
from lightcurver_amd.synthetic import make_roi_dataset
from tests import helpers as H

pytestmark = pytest.mark.gpu

FREE = ['a', 'c_x', 'c_y', 'dx', 'dy', 'h', 'mean']

# (alpha per epoch in degrees, (ss dx, ss dy) per epoch in high-resolution pixels).  Every rotated set holds 180 degrees with
# a shift of one to three data pixels and an angle in (90, 180); epoch 0 sits at 0 degrees as in the product.
# (Near-aligned angles - 0.3, 89.5, 179 - sweep the fractional sample position slowly across the grid: their shifts are
# chosen so that no sample of any stamp size below lands within 2e-5 of a kink; geometry_problem checks it.)
ROT_1 = ([0.0, 270.0, 180.0, 120.0, 359.9], [(0.37, -0.21), (-2.6, 3.4), (-5.3, -4.7), (2.71, -0.28), (5.3, 2.6)])
ROT_2 = ([0.0, 89.5, 180.0, 179.0, -135.0], [(0.0, 0.0), (2.71, -0.19), (-2.6, 3.4), (-5.37, -4.67), (0.37, -0.21)])
ROT_3 = ([0.3, 90.0, 180.0, 150.0, 30.0], [(0.35, -0.26), (5.3, -2.6), (2.6, -5.3), (-2.71, 3.38), (-0.37, 0.21)])
# translated: exact integer and half-pixel shifts (fxc = 0: the four-tap stencil loses two taps)
TRANS = ([0.0, 0.0, 0.0, 0.0], [(0.0, 0.0), (2.0, -3.0), (0.5, -1.5), (-5.0, 2.5)])
GEOM = {'rot1': ROT_1, 'rot2': ROT_2, 'rot3': ROT_3, 'trans': TRANS}

LAM_ON = dict(lam_scales=1.5, lam_hf=0.8, lam_pos=20.0, lam_pos_ps=5.0, lam_fu=0.7, lam_pts=0.3)


def ring_mask(N, width=2):
    m = np.ones((N, N), bool)
    m[width:-width, width:-width] = False
    return m


def ring_rel_err(got, ref, N):
    m = ring_mask(N)
    return H.rel_err(np.reshape(got, (N, N))[m], np.reshape(ref, (N, N))[m])


def kink_distance(N, alpha, sdx, sdy):
    """Smallest distance of a sample coordinate (Xs, Ys) of the N x N scene to an integer inside the grid, in float64.
    Where it is below float32's rounding of the position, the two implementations take different one-sided slopes."""
    c0 = (N - 1) / 2.0
    a = np.radians(alpha)
    u, v = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    qx, qy = v - c0 - sdx, u - c0 - sdy
    d = 1.0
    for Z in (c0 + np.cos(a) * qx + np.sin(a) * qy, c0 + np.cos(a) * qy - np.sin(a) * qx):
        Z = Z[(Z > -0.5) & (Z < N - 0.5)]
        if Z.size:
            d = min(d, float(np.abs(Z - np.round(Z)).min()))
    return d


def geometry_problem(n, ss, alphas, shifts, seed, M=2, with_background=True, rough=True):
    """Dataset drawn at the given angles and at the given shifts plus ~0.05 data pixels, parameters jittered from the truth
    (residuals are not zero) with the shifts exactly as given, and - with `rough` - a background with pixel-scale noise
    and a band of structure along the edges, where the clamped samples replicate it.  Every parameter is rounded to
    float32 first: the oracle sees the values the device holds."""
    from scipy.ndimage import gaussian_filter
    E = len(alphas)
    N = n * ss
    for a, (sx, sy) in zip(alphas, shifts):
        if a % 360.0 != 0.0:
            assert kink_distance(N, a, sx, sy) > 2e-5, (N, a, sx, sy)
    rng = np.random.default_rng(seed + 1)
    dx = np.array([s[0] for s in shifts]) / ss
    dy = np.array([s[1] for s in shifts]) / ss
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=seed, alpha=alphas, with_background=with_background,
                          dx=dx + rng.normal(0, 0.05, E), dy=dy + rng.normal(0, 0.05, E))
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    p['a'] = p['a'] * rng.uniform(0.9, 1.1, p['a'].shape)
    p['c_x'] = p['c_x'] + rng.normal(0, 0.1, M)
    p['c_y'] = p['c_y'] + rng.normal(0, 0.1, M)
    p['dx'], p['dy'] = dx, dy
    p['mean'] = rng.normal(0, 1e-3, E)
    if with_background and rough:
        h = p['h'].reshape(N, N)
        hmax = np.abs(h).max()
        h = h * rng.uniform(0.8, 1.2, h.shape) + 0.02 * hmax * rng.standard_normal(h.shape)
        field = gaussian_filter(rng.standard_normal((N, N)), 1.5, mode='wrap')
        edge = ring_mask(N, 3)
        h[edge] += 0.3 * hmax * (0.5 + field[edge] / np.abs(field).max())
        p['h'] = h.reshape(-1)
    elif not with_background:
        p['h'] = np.zeros_like(p['h'])
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    return ds, p


def _joint(ctx, ds, p, ss, M):
    from lightcurver_amd.joint import JointFit
    j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], ss, M, ctx)
    j.set_params(**p)
    return j


def _oracle_inputs(ds, p):
    return ({k: om.T(v) for k, v in p.items()}, om.T(ds['data']), om.T(ds['noisemap']) ** 2, om.T(ds['psf']))


def check_evaluation(j, ds, p, n, ss, M, dxy_tol=1e-4, outputs=True):
    """Model, chi2 per epoch, loss and every gradient block (the ring of dL/dh on its own) against the oracle, once with
    every loss term on and once with the data term alone (the ring then carries the data term only); with `outputs`
    also the deconvolved scene of every epoch and the Fisher flux errors."""
    N = n * ss
    po, data, sig2, psf = _oracle_inputs(ds, p)
    model, chi2_e = j.model()
    mo = om.deconv_model(po, psf, ss, n)
    print(f'evaluation n={n} ss={ss}: model {H.rel_err(model, mo.numpy()):.2e} chi2 per epoch '
          f'{H.rel_err(chi2_e, (((data - mo) ** 2) / sig2).sum((-1, -2)).numpy()):.2e}')
    assert H.rel_err(model, mo.numpy()) < 3e-5
    assert H.rel_err(chi2_e, (((data - mo) ** 2) / sig2).sum((-1, -2)).numpy()) < 3e-5
    W = om.propagate_noise_deconv(sig2, psf, ss)
    prior = [('c_x', po['c_x'] + 0.05, np.full(M, 0.5)), ('c_y', po['c_y'] - 0.02, np.full(M, 0.7))]
    legs = [(dict(W=W.numpy(), lam_scales=1.5, lam_hf=0.8, lam_positivity=20.0, lam_positivity_ps=5.0,
                  lam_flux_uniformity=0.7, lam_pts_source=0.3,
                  prior=dict(c_x_mean=prior[0][1].numpy(), c_x_sigma=prior[0][2], c_y_mean=prior[1][1].numpy(),
                             c_y_sigma=prior[1][2])),
             lambda q: om.deconv_loss(q, data, sig2, psf, ss, W=W, prior=prior, **LAM_ON)),
            (dict(), lambda q: om.deconv_loss(q, data, sig2, psf, ss))]
    j.set_free(FREE)
    for i, (cfg, fn) in enumerate(legs):
        j.set_loss(**cfg)
        L, g = oo.value_and_grad(fn, po, FREE)
        loss, grads = j.loss_grad(FREE)
        print(f'evaluation n={n} ss={ss} leg {i}: loss {abs(loss - float(L)) / abs(float(L)):.2e}',
              {k: '%.2e' % H.rel_err(grads[k], g[k].numpy()) for k in FREE}, f'ring of h {ring_rel_err(grads["h"], g["h"].numpy(), N):.2e}')
        assert abs(loss - float(L)) / abs(float(L)) < 3e-5, (i, loss, float(L))
        for k in FREE:
            assert H.rel_err(grads[k], g[k].numpy()) < (dxy_tol if k in ('dx', 'dy') else 1e-4), (i, k)
        assert ring_rel_err(grads['h'], g['h'].numpy(), N) < 1e-4, (i, ring_rel_err(grads['h'], g['h'].numpy(), N))
    if outputs:
        for e in range(len(p['dx'])):
            sc, bg = j.deconvolved(e)
            so, bo = om.deconv_deconvolved(po, e, N, ss)
            assert H.rel_err(sc, so.numpy()) < 1e-5 and H.rel_err(bg, bo.numpy()) < 1e-5, e
        assert H.rel_err(j.fisher_flux_sigma(), om.fisher_flux_sigma(po, sig2, psf, ss).numpy()) < 3e-5


@pytest.fixture
def debug_global():
    """The global-spectrum kernels forced onto small stamps (lc_joint_set_debug_global), switched off again afterwards."""
    from lightcurver_amd import _lib
    lib = _lib.lib()
    lib.lc_joint_set_debug_global(1)
    yield
    lib.lc_joint_set_debug_global(0)


# the default kernel of every instantiated stamp size; a subset of angle x shift sets per size (about 60 s of GPU time
# for the file), 180 degrees with a moderate shift and an angle in (90, 180) at every size
@pytest.mark.parametrize('n,ss,geom', [(16, 1, 'rot1'), (16, 1, 'trans'),
                                       (16, 2, 'rot1'), (16, 2, 'rot2'), (16, 2, 'rot3'), (16, 2, 'trans'),
                                       (24, 2, 'rot2'), (32, 2, 'rot1'), (32, 2, 'rot3'), (32, 2, 'trans'),
                                       (40, 2, 'rot2'), (48, 2, 'rot3'), (56, 2, 'rot1'), (64, 2, 'rot2'), (64, 2, 'trans'),
                                       # subsampling 1 (no binned rows: the branch beside FOLD): the sizes whose transforms
                                       # run over 8 lanes, then those over 16
                                       (24, 1, 'rot1'), (24, 1, 'rot2'), (24, 1, 'trans'), (40, 1, 'rot2'), (40, 1, 'trans'),
                                       (56, 1, 'rot3'), (56, 1, 'trans'),
                                       (32, 1, 'rot3'), (48, 1, 'rot1'), (64, 1, 'rot2'), (64, 1, 'trans')])
def test_default_kernels(ctx, monkeypatch, n, ss, geom):
    monkeypatch.delenv('LCMI_N128_SPLIT', raising=False)
    alphas, shifts = GEOM[geom]
    ds, p = geometry_problem(n, ss, alphas, shifts, 900 + n + ss)
    j = _joint(ctx, ds, p, ss, 2)
    check_evaluation(j, ds, p, n, ss, 2)
    j.close()


@pytest.mark.parametrize('parts,geom', [('1', 'rot1'), ('4', 'rot3')])
def test_n64_phased_launches(ctx, monkeypatch, parts, geom):
    """n = 64 through the global-spectrum kernels (LCMI_N128_SPLIT=1): one kernel, or one launch per phase with the epoch
    spread over four workgroups."""
    monkeypatch.setenv('LCMI_N128_SPLIT', '1')
    monkeypatch.setenv('LCMI_EPOCH_PARTS', parts)
    alphas, shifts = GEOM[geom]
    ds, p = geometry_problem(64, 2, alphas, shifts, 950 + int(parts))
    j = _joint(ctx, ds, p, 2, 2)
    check_evaluation(j, ds, p, 64, 2, 2, outputs=False)
    j.close()


@pytest.mark.parametrize('n,geom', [(16, 'rot2'), (16, 'trans'), (32, 'rot1')])
def test_forced_global_kernels(ctx, monkeypatch, debug_global, n, geom):
    monkeypatch.delenv('LCMI_EPOCH_PARTS', raising=False)
    alphas, shifts = GEOM[geom]
    ds, p = geometry_problem(n, 2, alphas, shifts, 960 + n)
    j = _joint(ctx, ds, p, 2, 2)
    check_evaluation(j, ds, p, n, 2, 2, outputs=False)
    j.close()


def test_n128_two_epochs(ctx):
    """The n = 128 instantiation (phased global-spectrum launches) at the size of test_joint_large_gpu's n = 128 tests: a
    pier-flipped epoch and one at 120 degrees.  dx / dy: the bound test_n128_loss_gradients_and_steps gives them (fp32 sums
    of 65536 products)."""
    ds, p = geometry_problem(128, 2, [120.0, 180.0], [(2.71, -0.28), (-5.3, -4.7)], 977)
    j = _joint(ctx, ds, p, 2, 2)
    check_evaluation(j, ds, p, 128, 2, 2, dxy_tol=3e-4, outputs=False)
    j.close()


def test_n128_two_epochs_at_subsampling_1(ctx, monkeypatch):
    """n = 128 at subsampling 1 (N = 128: the one-workgroup epoch kernel and its cluster form) at the angles and shifts
    above.  The cluster form runs inside the library's own loops only (cluster_parts), so beside the single evaluation -
    dx / dy at the bound of test_n128_two_epochs, for its reason: fp32 sums over a 128 x 128 stamp - five iterations of the
    device loop run in the form the object selects for two epochs (several workgroups per epoch, which must not fall back)
    and, with LCMI_CLUSTER=0, in the one-workgroup kernel, each against one oracle trajectory."""
    monkeypatch.delenv('LCMI_N128_SPLIT', raising=False)
    monkeypatch.delenv('LCMI_CLUSTER', raising=False)
    alphas, shifts = [120.0, 180.0], [(2.71, -0.28), (-5.3, -4.7)]
    ds, p = geometry_problem(128, 1, alphas, shifts, 978)
    j = _joint(ctx, ds, p, 1, 2)
    check_evaluation(j, ds, p, 128, 1, 2, dxy_tol=3e-4, outputs=False)
    j.close()
    T = 5
    ds, p = _trajectory_problem(128, 979, alphas, shifts, ss=1)
    ref = oracle_trajectory(ds, p, T, ss=1)
    j = _joint(ctx, ds, p, 1, 2)
    info = check_trajectory(j, ds, p, 128, T, ss=1, ref=ref)
    j.close()
    assert info[0] >= 2 and info[1] == 0, info       # several workgroups per epoch, no fall-back
    monkeypatch.setenv('LCMI_CLUSTER', '0')
    j = _joint(ctx, ds, p, 1, 2)
    info = check_trajectory(j, ds, p, 128, T, ss=1, ref=ref)
    j.close()
    assert tuple(info) == (0, 0), info


# ROT_1's shift of each angle
@pytest.mark.parametrize('n,ss,alphas,shifts', [(16, 2, [0.0, 120.0, 180.0], [(0.37, -0.21), (2.6, -0.3), (-5.3, -4.7)]),
                                                (16, 1, [0.0, 180.0, 120.0], [(0.0, 0.0), (-2.6, 3.4), (5.3, 2.6)]),
                                                (32, 2, [0.0, 180.0, 120.0], [(0.0, 0.0), (-5.3, -4.7), (2.6, -0.3)])] +
                         # subsampling 1: one or two strips per thread (24), four strips without the four-wave limit (64),
                         # outputs and PSF through global memory (128)
                         [(n, 1, [0.0, 180.0, 120.0], [(0.37, -0.21), (-5.3, -4.7), (2.71, -0.28)]) for n in (24, 64, 128)])
def test_point_source_only_path(ctx, n, ss, alphas, shifts):
    """h == 0 and fixed (csrc/joint_ps.h) at 120 and 180 degrees: model, loss, gradients and Fisher flux errors."""
    M = 2
    ds, p = geometry_problem(n, ss, alphas, shifts, 980 + n + ss, M=M, with_background=False)
    j = _joint(ctx, ds, p, ss, M)
    po, data, sig2, psf = _oracle_inputs(ds, p)
    free = ['a', 'c_x', 'c_y', 'dx', 'dy', 'mean']
    j.set_loss(lam_positivity_ps=5.0, lam_flux_uniformity=0.4)
    j.set_free(free)
    model, chi2_e = j.model()
    mo = om.deconv_model(po, psf, ss, n)
    assert H.rel_err(model, mo.numpy()) < 3e-5
    assert H.rel_err(chi2_e, (((data - mo) ** 2) / sig2).sum((-1, -2)).numpy()) < 3e-5
    L, g = oo.value_and_grad(lambda q: om.deconv_loss(q, data, sig2, psf, ss, lam_pos_ps=5.0, lam_fu=0.4), po, free)
    loss, grads = j.loss_grad(free)
    fisher = H.rel_err(j.fisher_flux_sigma(), om.fisher_flux_sigma(po, sig2, psf, ss).numpy())
    j.close()
    print(f'point sources only n={n} ss={ss}: model {H.rel_err(model, mo.numpy()):.2e} loss {abs(loss - float(L)) / abs(float(L)):.2e}',
          {k: '%.2e' % H.rel_err(grads[k], g[k].numpy()) for k in free}, f'fisher {fisher:.2e}')
    assert abs(loss - float(L)) / abs(float(L)) < 3e-5
    for k in free:
        assert H.rel_err(grads[k], g[k].numpy()) < 1e-4, k
    assert fisher < 3e-5


def _trajectory_problem(n, seed, alphas, shifts, ss=2):
    # the jitter of test_joint_gpu's trajectories (a background close to the truth): a pixel moves by at most T * lr
    ds, p = geometry_problem(n, ss, alphas, shifts, seed, rough=False)
    rng = np.random.default_rng(seed + 2)
    p['h'] = (p['h'] * rng.uniform(0.8, 1.2, p['h'].shape) + 2e-3 * rng.standard_normal(p['h'].shape))
    p['h'] = p['h'].astype(np.float32).astype(np.float64)
    return ds, p


TRAJ_LAMS = dict(lam_scales=1.0, lam_hf=1.0, lam_pos=10.0, lam_pts=0.01, lam_fu=1.0)


def oracle_trajectory(ds, p, T, lr=1e-3, ss=2):
    """-> (W, loss history (T + 1,), final parameters) of oo.adabelief on the loss check_trajectory sets."""
    po, data, sig2, psf = _oracle_inputs(ds, p)
    W = om.propagate_noise_deconv(sig2, psf, ss)
    pf, lh, l0 = oo.adabelief(lambda q: om.deconv_loss(q, data, sig2, psf, ss, W=W, **TRAJ_LAMS), po, FREE, lr, T, schedule=True)
    return W, np.array([l0] + lh), pf


def check_trajectory(j, ds, p, n, T, lr=1e-3, ss=2, ref=None):
    """T AdaBelief iterations of the device loop against oo.adabelief (`ref`: oracle_trajectory of the same problem, where
    several runs share it); the ring of h as tight as the interior.  Returns cluster_info() of the run."""
    N = ss * n
    W, ref, pf = ref if ref is not None else oracle_trajectory(ds, p, T, lr, ss)
    j.set_params(**p)
    j.set_loss(W=W.numpy(), lam_scales=1.0, lam_hf=1.0, lam_positivity=10.0, lam_pts_source=0.01, lam_flux_uniformity=1.0)
    j.set_free(FREE)
    j.run_adabelief(T, init_learning_rate=lr, schedule_learning_rate=True)
    info = j.cluster_info()
    hist = j.loss_history()
    got = j.get_params()
    dh = np.abs(got['h'] - pf['h'].numpy()).reshape(N, N)
    m = ring_mask(N)
    ring, inner = dh[m], dh[~m]
    print(f'trajectory n={n} ss={ss} T={T} cluster_info {tuple(info)}:',
          dict(hist='%.2e' % (np.abs(hist - ref).max() / np.abs(ref).max()), a='%.2e' % H.rel_err(got['a'], pf['a'].numpy()),
               c_x='%.2e' % np.abs(got['c_x'] - pf['c_x'].numpy()).max(), dx='%.2e' % np.abs(got['dx'] - pf['dx'].numpy()).max(),
               dy='%.2e' % np.abs(got['dy'] - pf['dy'].numpy()).max(), dh_max='%.2e' % dh.max(), dh_med='%.2e' % np.median(dh),
               ring_med='%.2e' % np.median(ring), ring_p95='%.2e' % np.percentile(ring, 95),
               inner_p95='%.2e' % np.percentile(inner, 95)))
    assert hist.shape == (T + 1,)
    assert np.abs(hist - ref).max() / np.abs(ref).max() < 2e-4
    assert H.rel_err(got['a'], pf['a'].numpy()) < 2e-4
    assert np.abs(got['c_x'] - pf['c_x'].numpy()).max() < 5e-4
    assert np.abs(got['dx'] - pf['dx'].numpy()).max() < 5e-4
    assert np.abs(got['dy'] - pf['dy'].numpy()).max() < 5e-4
    assert dh.max() < 0.05 * T * lr and np.median(dh) < 1e-5
    # a ring that follows another gradient drifts by up to lr per iteration in most of its pixels: its median and 95th
    # percentile must be those of the interior, where only the odd sign flip of a ~0 starlet coefficient shows
    assert np.median(ring) < 1e-5, (np.median(ring), np.median(inner))
    assert np.percentile(ring, 95) < max(2.0 * np.percentile(inner, 95), 2e-5), (np.percentile(ring, 95), np.percentile(inner, 95))
    return info


@pytest.mark.parametrize('cluster', ['0', '6'])
def test_n64_device_loop_mixed_angles(ctx, monkeypatch, cluster):
    """20 iterations of lc_joint_run_adabelief on a mixed-angle fit at n = 64: the one-workgroup kernel (LCMI_CLUSTER=0) and
    the cluster form with six workgroups per epoch (phase D with cross-workgroup loads), which must not fall back."""
    monkeypatch.delenv('LCMI_N128_SPLIT', raising=False)
    monkeypatch.setenv('LCMI_CLUSTER', cluster)
    ds, p = _trajectory_problem(64, 990, *ROT_1)
    j = _joint(ctx, ds, p, 2, 2)
    assert check_trajectory(j, ds, p, 64, 20) == (int(cluster), 0)
    j.close()


@pytest.mark.parametrize('n', [24, 56, 64])
def test_device_loop_mixed_angles_at_subsampling_1(ctx, monkeypatch, n):
    """20 iterations of ROT_1 at subsampling 1: n = 24 and 56 (transforms over 8 lanes; regulariser, reduction and update of
    the run-time-N kernels inside the loop) and n = 64 (16 lanes, single-workgroup update); ring against interior as above."""
    monkeypatch.delenv('LCMI_N128_SPLIT', raising=False)
    monkeypatch.delenv('LCMI_CLUSTER', raising=False)
    ds, p = _trajectory_problem(n, 985 + n, *ROT_1, ss=1)
    j = _joint(ctx, ds, p, 1, 2)
    info = check_trajectory(j, ds, p, n, 20, ss=1)
    j.close()
    assert info[1] == 0, info


def test_rotation_flag_follows_alpha(ctx, monkeypatch, debug_global):
    """The object learns whether any epoch is rotated when alpha is set (lc_joint_set_param): the device loop may apply the
    translation-only adjoint stencil in the reduction (LCMI_STENCIL_REDUCE=1, global-spectrum kernels) only while none
    is.  One object, all translated, then one epoch at 180 degrees, then all translated again: single evaluations and a
    device loop against the oracle after each change."""
    monkeypatch.setenv('LCMI_STENCIL_REDUCE', '1')
    monkeypatch.delenv('LCMI_EPOCH_PARTS', raising=False)
    n = 16
    shifts = [(0.37, -0.21), (2.6, -0.3), (-2.6, 3.4), (-5.3, -4.7)]
    ds, p0 = _trajectory_problem(n, 995, [0.0, 0.0, 180.0, 0.0], shifts)
    j = _joint(ctx, ds, p0, 2, 2)
    for alphas in ([0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 180.0, 0.0], [0.0, 0.0, 0.0, 0.0]):
        p = dict(p0, alpha=np.array(alphas))
        j.set_params(**p)
        check_evaluation(j, ds, p, n, 2, 2, outputs=False)
        check_trajectory(j, ds, p, n, 20)
    j.close()
