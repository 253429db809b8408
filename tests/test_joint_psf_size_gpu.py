"""Joint fits with PSF stamps of a side P other than the grid's N = ss n (lc_joint_create_psf; the reference's defaults
are 48 x 48 stamps beside a 64 x 64 grid).  The float64 oracle is fed the P x P stamps themselves - its conv_same takes
any kernel size - or, for P > N, the stamps' central window cut by the tests' own statement of the rule
(tests/_psf_place.py, written independently of joint.place_psf).  Bounds: those tests/test_joint_gpu.py applies to the
same quantities - 3e-5 on models, per-epoch chi2 and losses, 1e-4 on gradients per block, 1e-4 on W overall and 2e-4 per
scale, 3e-5 on the Fisher sigma.  A fit made from the stamps and one made from the tests' placed (E, N, N) stack see the
same device array and must agree bit for bit."""
import ctypes as C
import re
import warnings

import numpy as np
import pytest

from oracle import model as om, optim as oo
from lightcurver_amd import _lib
from lightcurver_amd.synthetic import make_narrow_psf, make_roi_dataset
from tests import _psf_place as PP
from tests import helpers as H

pytestmark = pytest.mark.gpu

FREE = ['a', 'c_x', 'c_y', 'dx', 'dy', 'h', 'mean']


def _stamps(E, P, ss, seed):
    rng = np.random.default_rng(seed)
    return np.stack([make_narrow_psf(rng, P, ss)[0] for _ in range(E)])


def _problem(E, M, n, ss, P, seed, with_h=True):
    """Data and truth of make_roi_dataset, stamps of side P, a jittered point (the parity checks do not need the data to come
    from these PSFs), and the stack the oracle takes: the stamps, or their window where they are wider than the grid."""
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=seed)
    stamps = _stamps(E, P, ss, seed + 1)
    rng = np.random.default_rng(seed + 7)
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    p['a'] = p['a'] * rng.uniform(0.9, 1.1, p['a'].shape)
    p['c_x'] = p['c_x'] + rng.normal(0, 0.1, M)
    p['c_y'] = p['c_y'] + rng.normal(0, 0.1, M)
    p['dx'] = p['dx'] + rng.normal(0, 0.05, E)
    p['dy'] = p['dy'] + rng.normal(0, 0.05, E)
    p['mean'] = rng.normal(0, 1e-3, E)
    p['h'] = p['h'] * rng.uniform(0.8, 1.2, p['h'].shape) + 2e-3 * rng.standard_normal(p['h'].shape)
    if not with_h:
        p['h'] = np.zeros_like(p['h'])
    N = n * ss
    oracle_psf = stamps if P <= N else PP.place(stamps, N)
    return ds, stamps, p, oracle_psf


def _fit(ctx, ds, psf, ss, M, p=None):
    from lightcurver_amd.joint import JointFit
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)     # (P > N warns: test_warning_names_the_lost_flux)
        j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, psf, ss, M, ctx)
    if p is not None:
        j.set_params(**p)
    return j


def _check_model_loss_and_gradients(ctx, E, M, n, ss, P):
    ds, stamps, p, opsf = _problem(E, M, n, ss, P, 900 + n + P)
    j = _fit(ctx, ds, stamps, ss, M, p)
    assert j.psf_side == P
    po = {k: om.T(v) for k, v in p.items()}
    data, sig2, psf = om.T(ds['data']), om.T(ds['noisemap']) ** 2, om.T(opsf)
    W = om.propagate_noise_deconv(sig2, psf, ss)
    lam = dict(lam_scales=1.5, lam_hf=0.8, lam_pos=20.0, lam_pos_ps=5.0, lam_fu=0.7, lam_pts=0.3)
    prior = [('c_x', po['c_x'] + 0.05, np.full(M, 0.5)), ('c_y', po['c_y'] - 0.02, np.full(M, 0.7))]
    j.set_loss(W=W.numpy(), lam_scales=1.5, lam_hf=0.8, lam_positivity=20.0, lam_positivity_ps=5.0,
               lam_flux_uniformity=0.7, lam_pts_source=0.3,
               prior=dict(c_x_mean=prior[0][1].numpy(), c_x_sigma=prior[0][2], c_y_mean=prior[1][1].numpy(),
                          c_y_sigma=prior[1][2]))
    j.set_free(FREE)
    model, chi2_e = j.model()
    mo = om.deconv_model(po, psf, ss, n)
    L, g = oo.value_and_grad(lambda q: om.deconv_loss(q, data, sig2, psf, ss, W=W, prior=prior, **lam), po, FREE)
    loss, grads = j.loss_grad(FREE)
    j.close()
    figures = dict(model=H.rel_err(model, mo.numpy()),
                   chi2=H.rel_err(chi2_e, (((data - mo) ** 2) / sig2).sum((-1, -2)).numpy()),
                   loss=abs(loss - float(L)) / abs(float(L)), **{k: H.rel_err(grads[k], g[k].numpy()) for k in FREE})
    print(f'(E, M, n, ss, P) = {(E, M, n, ss, P)}:', {k: f'{v:.2e}' for k, v in figures.items()})
    assert figures['model'] < 3e-5 and figures['chi2'] < 3e-5 and figures['loss'] < 3e-5
    for k in FREE:
        assert figures[k] < 1e-4, k


@pytest.mark.parametrize('E,M,n,ss,P', [(3, 2, 16, 2, 8), (3, 2, 16, 2, 30), (3, 2, 16, 2, 31), (3, 2, 16, 2, 33),
                                        (3, 2, 16, 2, 48), (3, 1, 16, 1, 9), (3, 1, 16, 1, 24), (2, 2, 64, 2, 96)])
def test_model_loss_and_gradients(ctx, E, M, n, ss, P):
    """31: odd parity; 33: the offset is -1, one row and one column fall off on one side only; 48 and 24 (ss = 1): windowed;
    96 on 128: the global-spectrum / large-grid kernels at the 3 : 4 ratio of the reference's defaults."""
    _check_model_loss_and_gradients(ctx, E, M, n, ss, P)


def test_model_loss_and_gradients_forced_global_kernels(ctx):
    lib = _lib.lib()
    lib.lc_joint_set_debug_global(1)
    try:
        _check_model_loss_and_gradients(ctx, 3, 2, 16, 2, 24)
    finally:
        lib.lc_joint_set_debug_global(0)


@pytest.mark.parametrize('fft_only', [False, True])
def test_point_source_only_path(ctx, monkeypatch, fft_only):
    """h zero and fixed: the point-source kernel reads psf_dev itself, the FFT pipeline (LCMI_JOINT_FFT_ONLY=1) its spectra."""
    if fft_only:
        monkeypatch.setenv('LCMI_JOINT_FFT_ONLY', '1')
    else:
        monkeypatch.delenv('LCMI_JOINT_FFT_ONLY', raising=False)
    E, M, n, ss, P = 3, 1, 32, 2, 48
    ds, stamps, p, opsf = _problem(E, M, n, ss, P, 520, with_h=False)
    j = _fit(ctx, ds, stamps, ss, M, p)
    free = ['a', 'c_x', 'c_y', 'dx', 'dy', 'mean']
    j.set_loss(lam_positivity_ps=5.0, lam_flux_uniformity=0.4)
    j.set_free(free)
    po = {k: om.T(v) for k, v in p.items()}
    data, sig2, psf = om.T(ds['data']), om.T(ds['noisemap']) ** 2, om.T(opsf)
    model, chi2_e = j.model()
    mo = om.deconv_model(po, psf, ss, n)
    assert H.rel_err(model, mo.numpy()) < 3e-5
    assert H.rel_err(chi2_e, (((data - mo) ** 2) / sig2).sum((-1, -2)).numpy()) < 3e-5
    L, g = oo.value_and_grad(lambda q: om.deconv_loss(q, data, sig2, psf, ss, lam_pos_ps=5.0, lam_fu=0.4), po, free)
    loss, grads = j.loss_grad(free)
    assert abs(loss - float(L)) / abs(float(L)) < 3e-5
    for k in free:
        assert H.rel_err(grads[k], g[k].numpy()) < 1e-4, k
    assert H.rel_err(j.fisher_flux_sigma(), om.fisher_flux_sigma(po, sig2, psf, ss).numpy()) < 3e-5
    j.close()


@pytest.mark.parametrize('P', [24, 40])
def test_noise_propagation_and_fisher(ctx, monkeypatch, P):
    """Device W and Fisher sigma against the oracle; then the two host readers of the rule: W under LCMI_NOISE_HOST=1 (float64
    on the host, from the stamps at their own side) against the oracle and against the device form, and an object created under
    LCMI_SPECTRA_HOST=1, whose model must be the device form's, all to 3e-5."""
    E, M, n, ss = 4, 2, 16, 2
    monkeypatch.delenv('LCMI_NOISE_HOST', raising=False)
    monkeypatch.delenv('LCMI_SPECTRA_HOST', raising=False)
    ds, stamps, p, opsf = _problem(E, M, n, ss, P, 611 + P)
    j = _fit(ctx, ds, stamps, ss, M, p)
    po = {k: om.T(v) for k, v in p.items()}
    sig2, psf = om.T(ds['noisemap']) ** 2, om.T(opsf)
    W = j.propagate_noise()
    Wo = om.propagate_noise_deconv(sig2, psf, ss).numpy()
    assert W.shape == Wo.shape
    print(f'P = {P}: W {H.rel_err(W, Wo):.2e}, per scale', [f'{H.rel_err(W[s], Wo[s]):.2e}' for s in range(W.shape[0])])
    assert H.rel_err(W, Wo) < 1e-4
    for s in range(W.shape[0]):
        assert H.rel_err(W[s], Wo[s]) < 2e-4, s
    sig = j.fisher_flux_sigma()
    assert H.rel_err(sig, om.fisher_flux_sigma(po, sig2, psf, ss).numpy()) < 3e-5
    model, _ = j.model()
    monkeypatch.setenv('LCMI_NOISE_HOST', '1')
    Wh = j.propagate_noise()
    monkeypatch.delenv('LCMI_NOISE_HOST')
    print(f'P = {P}: host W against the oracle {H.rel_err(Wh, Wo):.2e}, against the device form {H.rel_err(Wh, W):.2e}')
    assert H.rel_err(Wh, Wo) < 3e-5 and H.rel_err(Wh, W) < 3e-5
    j.close()
    monkeypatch.setenv('LCMI_SPECTRA_HOST', '1')
    jh = _fit(ctx, ds, stamps, ss, M, p)
    monkeypatch.delenv('LCMI_SPECTRA_HOST')
    model_h, _ = jh.model()
    jh.close()
    assert H.rel_err(model_h, model) < 3e-5
    assert H.rel_err(model_h, om.deconv_model(po, psf, ss, n).numpy()) < 3e-5


def _everything(j, p, T=20):
    """What a fit computes, in one tuple of arrays: model, loss and gradients, W, Fisher sigma, and the parameters and the loss
    history after T AdaBelief steps from p."""
    j.set_params(**p)
    W = j.propagate_noise()
    j.set_loss(W=W, lam_scales=1.0, lam_hf=1.0, lam_positivity=10.0, lam_pts_source=0.3)
    j.set_free(FREE)
    model, chi2 = j.model()
    loss, grads = j.loss_grad(FREE)
    sig = j.fisher_flux_sigma()
    j.run_adabelief(T, init_learning_rate=1e-3, schedule_learning_rate=True)
    got = j.get_params()
    return ([model, chi2, np.float32(loss), W, sig, j.loss_history()] + [grads[k] for k in FREE]
            + [got[k] for k in sorted(got)])


def _assert_identical(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), i


@pytest.mark.parametrize('P', [8, 31, 48])
def test_stamps_and_placed_stack_are_one_fit(ctx, P):
    E, M, n, ss = 3, 2, 16, 2
    ds, stamps, p, _ = _problem(E, M, n, ss, P, 700 + P)
    placed = PP.place(stamps.astype(np.float32), n * ss)
    ja, jb = _fit(ctx, ds, stamps, ss, M), _fit(ctx, ds, placed, ss, M)
    assert ja.psf_side == P and jb.psf_side == n * ss
    ra, rb = _everything(ja, p), _everything(jb, p)
    ja.close()
    jb.close()
    _assert_identical(ra, rb)
    assert np.all(np.isfinite(ra[5])) and ra[5].shape == (21,)


def test_create_is_create_psf_at_the_grid_side(ctx, monkeypatch):
    """lc_joint_create against lc_joint_create_psf(psf_side = N): one object through each symbol, bit-equal."""
    E, M, n, ss = 3, 2, 16, 2
    ds, stamps, p, _ = _problem(E, M, n, ss, n * ss, 760)
    lib = _lib.lib()
    ra = _everything(_fit(ctx, ds, stamps, ss, M), p)
    calls = []

    def through_create(c, E_, M_, n_, ss_, side, d, s2, psf, out):
        calls.append(side)
        return lib.lc_joint_create(c, E_, M_, n_, ss_, d, s2, psf, out)
    monkeypatch.setattr(lib, 'lc_joint_create_psf', through_create, raising=False)
    jb = _fit(ctx, ds, stamps, ss, M)
    monkeypatch.undo()
    assert calls == [n * ss]
    _assert_identical(ra, _everything(jb, p))
    jb.close()


@pytest.mark.parametrize('P', [24, 44])
def test_embedded_size_windows_to_the_callers_grid(ctx, P):
    """n = 20 is fitted at 24 (grid 48): a 44-wide stamp is wider than the caller's 40 and narrower than 48, and must be cut
    to 40 all the same - what EmbeddedJointFit computes from the tests' placed (E, 40, 40) stack."""
    from lightcurver_amd.joint import EmbeddedJointFit, make_joint_fit
    E, M, n, ss = 3, 2, 20, 2
    ds, stamps, p, _ = _problem(E, M, n, ss, P, 800 + P)
    sig2 = ds['noisemap'].astype(np.float64) ** 2
    placed = PP.place(stamps.astype(np.float32), n * ss)
    if P > n * ss:
        with pytest.warns(UserWarning, match='wider than the 40 x 40 grid'):
            ja = make_joint_fit(ds['data'], sig2, stamps, ss, M, ctx)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            ja = make_joint_fit(ds['data'], sig2, stamps, ss, M, ctx)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        jb = make_joint_fit(ds['data'], sig2, placed, ss, M, ctx)
    assert isinstance(ja, EmbeddedJointFit) and isinstance(jb, EmbeddedJointFit) and ja.psf_side == P
    ra, rb = _everything(ja, p), _everything(jb, p)
    ja.close()
    jb.close()
    _assert_identical(ra, rb)


def test_roi_fit_at_the_reference_defaults(ctx):
    """stamp_size_stars = 24, stamp_size_ROI = 32, subsampling 2: psf (E, 48, 48) beside data (E, 32, 32)."""
    from lightcurver_amd.processes.roi_modelling import model_roi_cutouts
    E, M, n, ss, P = 4, 2, 32, 2, 48
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=31)
    stamps = _stamps(E, P, ss, 32).astype(np.float32)
    off = (n - 1) / 2.0
    xs, ys = np.asarray(ds['truth']['c_x']) + off, np.asarray(ds['truth']['c_y']) + off

    def fit(psf):
        with warnings.catch_warnings():
            warnings.filterwarnings('error', message='PSF stamps')      # 48 <= 64: nothing is windowed
            return model_roi_cutouts(ds['data'] * ds['scale'], ds['noisemap'] * ds['scale'], psf, ss, xs, ys,
                                     fix_point_source_astrometry=0.5, roi_deconv_translations_iters=30,
                                     roi_deconv_all_iters=60)
    out, ref = fit(stamps), fit(PP.place(stamps, n * ss))
    assert len(out['loss_history']) == 60 and np.all(np.isfinite(out['loss_history']))
    assert 1 <= len(out['loss_history_stage1']) <= 31 and np.all(np.isfinite(out['loss_history_stage1']))
    for grp in ('kwargs_analytic', 'kwargs_background'):
        for name, v in out['kwargs_final'][grp].items():
            assert np.all(np.isfinite(np.asarray(v))), name
            assert np.array_equal(np.asarray(v), np.asarray(ref['kwargs_final'][grp][name])), name
    assert np.array_equal(np.asarray(out['loss_history']), np.asarray(ref['loss_history']))
    assert np.array_equal(np.asarray(out['loss_history_stage1']), np.asarray(ref['loss_history_stage1']))


def test_one_star_forward_modelling_with_small_stamps(ctx):
    from lightcurver_amd.processes.star_photometry import do_one_star_forward_modelling
    E, n, ss, P = 4, 16, 2, 24
    ds = make_roi_dataset(E=E, M=1, n=n, ss=ss, seed=41)
    out = do_one_star_forward_modelling(ds['data'].astype(np.float64) * ds['scale'], ds['noisemap'].astype(np.float64) * ds['scale'],
                                        _stamps(E, P, ss, 42), ss, n_iter=30)
    assert len(out['loss_curve']) == 30 and np.all(np.isfinite(out['loss_curve']))
    assert np.asarray(out['fluxes']).shape == (E,) and np.all(np.isfinite(out['fluxes']))


def test_facade_model_and_noise_levels(ctx):
    """starred.Deconv / setup_model with s (E, P, P), and starred.utils.noise_utils.propagate_noise on that model: what a
    JointFit on the placed stack gives."""
    from lightcurver_amd.starred.deconvolution.deconvolution import setup_model
    from lightcurver_amd.starred.utils.noise_utils import propagate_noise
    E, M, n, ss, P = 3, 2, 16, 2, 24
    ds, stamps, p, _ = _problem(E, M, n, ss, P, 850)
    data, noise = ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64)
    t = ds['truth']
    model, k_init, _, _, _ = setup_model(data, noise ** 2, stamps, t['c_x'], t['c_y'], ss, list(t['a']), ctx=ctx)
    W = propagate_noise(model, noise, k_init, wavelet_type_list=['starlet'], method='SLIT', num_samples=500, seed=1,
                        likelihood_type='chi2', verbose=False, upsampling_factor=ss)[0]
    m = model.model(k_init)
    init = dict(k_init['kwargs_analytic'], **k_init['kwargs_background'])
    j = _fit(ctx, ds, PP.place(stamps.astype(np.float32), n * ss), ss, M,
             {k: np.asarray(v, dtype=np.float64) for k, v in init.items()})
    assert np.array_equal(W, j.propagate_noise())
    assert np.array_equal(m, j.model()[0])
    j.close()


def test_refusals_through_the_abi(ctx):
    """Refused on the host, before anything is allocated or launched: *out keeps its value, lc_last_error says why."""
    lib = _lib.lib()
    d = np.ones((2, 16, 16), np.float32)
    k = np.ones((2, 4, 4), np.float32)
    marker = 0x5A5A5A5A
    for side, rc, word in ((0, -1, b'psf_side'), (-3, -1, b'psf_side'), (46341, -3, b'2^31')):   # 46341^2 >= 2^31
        h = C.c_void_p(marker)
        assert lib.lc_joint_create_psf(ctx.h, 1, 1, 16, 2, side, _lib.ptr(d), _lib.ptr(d), _lib.ptr(k), C.byref(h)) == rc
        assert h.value == marker
        assert word in lib.lc_last_error(ctx.h)


def test_warning_names_the_lost_flux(ctx):
    from lightcurver_amd.joint import JointFit
    E, M, n, ss, P = 3, 1, 16, 2, 48
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=51)
    sig2 = ds['noisemap'].astype(np.float64) ** 2
    stamps = _stamps(E, P, ss, 52)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        j = JointFit(ds['data'], sig2, stamps, ss, M, ctx)
    j.close()
    seen = [w for w in seen if issubclass(w.category, UserWarning)]
    assert len(seen) == 1
    numbers = re.findall(r'[0-9]\.[0-9]+e[-+][0-9]+', str(seen[0].message))
    assert len(numbers) == 1
    want = PP.flux_outside(stamps.astype(np.float32), n * ss)
    assert want > 0 and abs(float(numbers[0]) - want) <= 1e-6 * want
    for side in (8, 31, 32):
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            JointFit(ds['data'], sig2, _stamps(E, side, ss, 53), ss, M, ctx).close()
