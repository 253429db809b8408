"""lc_diffim_frames and lc_frames_subtract_reference on the device (DESIGN.md §5 "Difference imaging") against the NumPy
restatement of tests/_diffim.py, at the small shapes where they can go wrong: 40 x 48, 17 x 19 (narrower than a tile),
67 x 131 (prime sides, several tiles both ways); r = 1, 2, 3 and 7; the three background degrees; one region and 2 x 3
uneven ones; K = 1 and 3; with and without variances, sigma and masks; a NaN in T and in R; clip_iters 0 and 2.

n_used, status and the NaN set of diff are compared exactly.  gram and rhs: every entry within (n_used + 4) 2^-53 sum w
|a_m| |a_n| of the long-double restatement (the summation bound for any order plus the product roundings).  diff: within
C_BOUND 2^-24 (sum |K_m| |R| + |bg| + |T|) of the float64 restatement, C_BOUND the next power of two >= 4 x the float32
restatement's own worst ratio (tests/test_diffim_cpu.py measures it).  The kernel itself only in the known-kernel case."""
import ctypes as C

import numpy as np
import pytest

from tests import _diffim as DI

pytestmark = pytest.mark.gpu

ALL = ('diff', 'kernel', 'bg', 'scale', 'n_used', 'chi2', 'status', 'gram', 'rhs')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return all(np.array_equal(_bits(a[key]), _bits(b[key])) for key in ALL if key in a)


@pytest.fixture(scope='module')
def run(ctx):
    from lightcurver_amd.processes.difference_imaging import match_and_subtract
    cache = {}

    def call(name):
        if name not in cache:
            c = DI.case(name)
            cache[name] = match_and_subtract(c['T'], c['R'], variance=c['var'], mask=c['mask'], sigma=c['sigma'],
                                             download=ALL, ctx=ctx, **c['settings'])
        return cache[name]
    return call


@pytest.mark.parametrize('name', list(DI.CASES))
def test_equals_the_restatement(run, name):
    c, want, got = DI.case(name), DI.wanted(name), run(name)
    r, bg_degree = c['settings']['r'], c['settings']['bg_degree']
    P = (2 * r + 1) ** 2 + DI.n_background(bg_degree)
    K, (H, W) = len(c['T']), c['R'].shape
    G = len(DI.regions_of((H, W), c['settings']['regions']))
    assert got['diff'].shape == (K, H, W) and got['diff'].dtype == np.float32 and got['gram'].shape == (K, G, P, P)
    worst_u = worst_b = worst_d = 0.0
    bits = True
    for k, ref in enumerate(want):
        assert np.array_equal(got['n_used'][k], ref['n_used']), (k, got['n_used'][k], ref['n_used'])
        assert np.array_equal(got['status'][k], ref['status']), (k, got['status'][k], ref['status'])
        assert np.array_equal(np.isnan(got['diff'][k]), np.isnan(ref['diff64'])), k
        assert not np.isinf(got['diff'][k]).any()
        for g, f in enumerate(ref['fits']):
            U, b, Ua, ba = DI.gram(f['A'], f['w'], f['t'])
            eu, eb = np.abs(got['gram'][k, g] - U), np.abs(got['rhs'][k, g] - b)
            unit = (f['n'] + 4) * 2.0 ** -53
            with np.errstate(invalid='ignore', divide='ignore'):
                worst_u = max(worst_u, float(np.nanmax(np.where(Ua > 0, eu / (unit * Ua), 0.0))))
                worst_b = max(worst_b, float(np.nanmax(np.where(ba > 0, eb / (unit * ba), 0.0))))
            assert np.all(eu <= unit * Ua), (k, g)
            assert np.all(eb <= unit * ba), (k, g)
            assert np.array_equal(got['gram'][k, g], got['gram'][k, g].T)
        ok = np.isfinite(ref['diff64'])
        err = np.abs(got['diff'][k][ok].astype(np.float64) - ref['diff64'][ok])
        bound = DI.diff_bound(ref['magnitude'][ok])
        worst_d = max(worst_d, float((err / bound).max()) if ok.any() else 0.0)
        assert np.all(err <= bound), (k, float((err / bound).max()))
        bits = bits and np.array_equal(_bits(got['diff'][k][ok]), _bits(ref['diff32'][ok]))
        good = ref['status'] == 0
        assert np.isnan(got['kernel'][k][~good]).all() and np.isnan(got['scale'][k][~good]).all() \
            and np.isnan(got['chi2'][k][~good]).all() and np.isnan(got['bg'][k][~good]).all()
        assert np.isfinite(got['kernel'][k][good]).all()
        assert np.allclose(got['scale'][k][good], got['kernel'][k][good].reshape(good.sum(), -1).sum(axis=1), rtol=1e-13)
        assert np.all(np.abs(got['chi2'][k][good] - ref['chi2'][good]) <= ref['chi2_slack'][good] + 1e-12 * ref['chi2'][good])
        assert not got['bg'][k][good][:, DI.n_background(bg_degree):].any()
    print(f'{name}: worst gram error {worst_u:.3f}, rhs {worst_b:.3f} of the bound; diff {worst_d:.3f} of the bound '
          f'(C_BOUND {DI.C_BOUND:g}); bits of the float32 restatement: {bits}; kernel {got["kernel_ms"]:.3f} ms, split '
          f'{got["split_ms"]}')


def test_known_kernel_element_by_element(ctx):
    """The well-conditioned known-kernel case: every element of the fitted kernel within 4 x the gap between the
    restatement's two float64 solutions (Cholesky of the normal equations, lstsq) on the same inputs."""
    from lightcurver_amd.processes.difference_imaging import match_and_subtract
    s = DI.known_kernel_scene()
    ref = DI.subtract(s['T'], s['R'], r=2, bg_degree=1, clip_iters=0)
    f = ref['fits'][0]
    gap = float(np.abs(f['x'] - f['x_lstsq']).max())
    got = match_and_subtract(s['T'], s['R'], r=2, bg_degree=1, clip_iters=0, ctx=ctx)
    assert got['diff'].shape == s['T'].shape and got['kernel'].shape == (1, 5, 5) and got['status'][0] == 0
    err = np.abs(np.concatenate([got['kernel'].reshape(-1), got['bg'][0, :3]]) - f['x'])
    print(f'gap between the two float64 solutions {gap:.3e}; device against the Cholesky restatement {err.max():.3e}; '
          f'against the truth {np.abs(got["kernel"][0] - s["K"]).max():.3e}; scale {got["scale"][0]:.9f}')
    assert np.all(err <= 4.0 * gap)
    assert np.abs(got['kernel'][0] - s['K']).max() < 1e-5 and abs(got['scale'][0] - 0.8) < 1e-5
    assert np.nanmax(np.abs(got['diff'])) < 2000 * 2.0 ** -21


def test_bits_do_not_depend_on_the_run_or_on_the_company(ctx, run):
    from lightcurver_amd.processes.difference_imaging import match_and_subtract
    for name in ('var_clip', 'regions'):
        c, first = DI.case(name), run(name)
        call = lambda sel: match_and_subtract(c['T'][sel], c['R'], variance=None if c['var'] is None else c['var'][sel],
                                              mask=None if c['mask'] is None else c['mask'][sel],
                                              sigma=None if c['sigma'] is None else c['sigma'][sel], download=ALL, ctx=ctx,
                                              **c['settings'])
        assert _same(call(slice(None)), first)
        for k in range(len(c['T'])):
            alone = call(slice(k, k + 1))
            assert all(np.array_equal(_bits(alone[key][0]), _bits(first[key][k])) for key in ALL), (name, k)
        swapped = call([2, 0, 1])
        assert all(np.array_equal(_bits(swapped[key][0]), _bits(first[key][2])) for key in ALL)


def test_null_outputs(ctx, run):
    from lightcurver_amd.processes.difference_imaging import match_and_subtract
    c, full = DI.case('sigma_clip'), run('sigma_clip')
    for download in (('scale',), ('diff',), ('n_used', 'status'), ('gram', 'rhs', 'chi2')):
        got = match_and_subtract(c['T'], c['R'], sigma=c['sigma'], download=download, ctx=ctx, **c['settings'])
        assert set(got) == set(download) | {'kernel_ms', 'split_ms'}
        assert all(np.array_equal(_bits(got[key]), _bits(full[key])) for key in download)
    one = match_and_subtract(c['T'][0], c['R'], sigma=1.0, ctx=ctx, **c['settings'])
    assert one['diff'].shape == c['R'].shape and np.array_equal(_bits(one['diff']), _bits(full['diff'][0]))


# ---- the frames form --------------------------------------------------------------------------------------------------------
def _transforms():
    th = np.deg2rad(1.7)
    rot = np.array([[np.cos(th), -np.sin(th), 1.3], [np.sin(th), np.cos(th), -0.8]])
    return [np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), rot, np.array([[1.01, 0.0, 0.4], [0.0, 0.99, 0.25]])]


@pytest.fixture(scope='module')
def fs(ctx):
    from lightcurver_amd.frames import FrameSet
    with FrameSet(DI.case('var_clip')['T'], ctx) as s:
        yield s


@pytest.mark.parametrize('order', (1, 3))
def test_frames_form_equals_the_host_form_on_the_coadd_of_one_frame(fs, ctx, order):
    from lightcurver_amd.processes.difference_imaging import match_and_subtract
    c = DI.case('var_clip')
    R = np.nan_to_num(c['R'])
    index, A = [2, 0, 1, 0], _transforms() + [_transforms()[1]]
    before = fs.planes()
    T = np.stack([fs.coadd([k], [a], order=order, combine='mean')['image'] for k, a in zip(index, A)])
    assert np.isnan(T).any() and np.isfinite(T[:, 5:-5, 5:-5]).all()
    settings = dict(r=2, bg_degree=1, regions=(2, 1), clip_iters=2, n_sigma=4.0)
    sigma = np.array([1.0, 1.5, 2.0, 1.5], np.float32)
    mask = np.zeros(T.shape, np.uint8)
    mask[:, 10:14, 20:30] = 1
    host = match_and_subtract(T, R, sigma=sigma, mask=mask, download=ALL, ctx=ctx, **settings)
    assert (host['status'] == 0).all()
    for scratch in (0, 1, 3, len(index)):
        got = fs.subtract_reference(index, A, R, order=order, sigma=sigma, mask=mask, download=ALL, scratch_frames=scratch,
                                    **settings)
        for key in ALL:
            assert np.array_equal(_bits(got[key]), _bits(host[key])), (key, scratch)
    assert np.array_equal(_bits(fs.planes()), _bits(before))
    with pytest.raises(ValueError, match='sigma is needed'):
        fs.subtract_reference(index, A, R)


def test_refusals_leave_the_outputs_untouched(fs, ctx):
    from lightcurver_amd import _lib
    lib = _lib.lib()
    c = DI.case('plain')
    T, R = np.ascontiguousarray(c['T']), np.ascontiguousarray(c['R'])
    K, H, W = T.shape
    fp, ip, dp, u8 = _lib.fp, _lib.ip, _lib.dp, C.POINTER(C.c_uint8)
    diff = np.full((2, H, W), 7.0, np.float32)           # the frames form below writes two frames of the same shape
    status = np.full((K, 64), 7, np.int32)
    out = _lib.DiffimOut()
    out.diff, out.status = diff.ctypes.data_as(fp), status.ctypes.data_as(ip)
    good = dict(r=2, bg_degree=1, gy=1, gx=1, clip_iters=1, n_sigma=4.0)
    cfg = lambda **kw: C.byref(_lib.DiffimCfg(*[{**good, **kw}[n] for n in ('r', 'bg_degree', 'gy', 'gx', 'clip_iters', 'n_sigma')]))
    bad_sigma = np.array([0.0], np.float32)
    DEFAULT = object()                                   # cfg_=None is the null pointer
    host = lambda K_=K, h=H, w=W, t=T, r=R, sigma=None, cfg_=DEFAULT, out_=out: lib.lc_diffim_frames(
        ctx.h, K_, h, w, None if t is None else t.ctypes.data_as(fp), None if r is None else r.ctypes.data_as(fp), None,
        None, None if sigma is None else sigma.ctypes.data_as(fp), cfg() if cfg_ is DEFAULT else cfg_,
        None if out_ is None else C.byref(out_), None)
    INVALID, UNSUPPORTED = -1, -3
    assert host(K_=0) == INVALID and host(t=None) == INVALID and host(r=None) == INVALID and host(out_=None) == INVALID
    assert host(out_=_lib.DiffimOut()) == INVALID and host(sigma=bad_sigma) == INVALID and host(cfg_=None) == INVALID
    for kw in (dict(r=0), dict(r=8), dict(bg_degree=-1), dict(bg_degree=3), dict(gy=0), dict(gx=0), dict(gy=9, gx=8),
               dict(clip_iters=-1), dict(n_sigma=0.0), dict(n_sigma=float('nan')), dict(n_sigma=float('inf'))):
        assert host(cfg_=cfg(**kw)) == INVALID, kw
    assert host(h=4, w=W) == UNSUPPORTED and host(cfg_=cfg(r=7), h=14, w=14) == UNSUPPORTED
    assert lib.lc_diffim_supported(15, 15, 7, 2, 1, 1) == 1 and lib.lc_diffim_supported(14, 15, 7, 2, 1, 1) == 0
    assert lib.lc_diffim_supported(40, 48, 3, 1, 8, 8) == 1 and lib.lc_diffim_supported(40, 48, 3, 1, 5, 13) == 0
    assert lib.lc_diffim_supported(46341, 46341, 3, 1, 1, 1) == 0
    # the frames form
    n = 2
    frame = np.array([0, 1], np.int32)
    affine = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (n, 1))
    sig = np.ones(n, np.float32)
    Rf = np.ascontiguousarray(np.nan_to_num(DI.case('var_clip')['R']))
    Hf, Wf = Rf.shape
    assert (Hf, Wf) == (H, W) and K == 1

    def frames(n_=n, frame_=frame, affine_=affine, ref=Rf, sigma=sig, order=3, scratch=0, cfg_=DEFAULT, out_=out, H_=Hf, W_=Wf):
        return lib.lc_frames_subtract_reference(
            fs.h, n_, None if frame_ is None else frame_.ctypes.data_as(ip), None if affine_ is None else affine_.ctypes.data_as(dp),
            H_, W_, 0, 0, order, None if ref is None else ref.ctypes.data_as(fp), None if sigma is None else sigma.ctypes.data_as(fp),
            None, cfg() if cfg_ is DEFAULT else cfg_, scratch, None if out_ is None else C.byref(out_), None)

    assert frames(n_=0) == INVALID and frames(frame_=None) == INVALID and frames(affine_=None) == INVALID
    assert frames(ref=None) == INVALID and frames(out_=None) == INVALID and frames(out_=_lib.DiffimOut()) == INVALID
    assert frames(frame_=np.array([0, 3], np.int32)) == INVALID and frames(frame_=np.array([-1, 0], np.int32)) == INVALID
    singular, infinite = affine.copy(), affine.copy()
    singular[1] = [1.0, 2.0, 0, 2.0, 4.0, 0]
    infinite[0, 2] = np.inf
    assert frames(affine_=singular) == INVALID and frames(affine_=infinite) == INVALID
    assert frames(order=2) == INVALID and frames(scratch=-1) == INVALID and frames(cfg_=None) == INVALID
    assert frames(sigma=np.array([1.0, np.nan], np.float32)) == INVALID
    for kw in (dict(r=0), dict(bg_degree=3), dict(gy=65), dict(clip_iters=-1), dict(n_sigma=-1.0)):
        assert frames(cfg_=cfg(**kw)) == INVALID, kw
    assert frames(H_=4, W_=4) == UNSUPPORTED
    assert (diff == 7.0).all() and (status == 7).all()
    # the set and the context are still usable
    assert frames() == 0 and np.isfinite(diff[:n, 2:-2, 2:-2]).all() and (status[0, 0], status[0, 1]) == (0, 0)
    assert host() == 0


# ---- physics ----------------------------------------------------------------------------------------------------------------
def test_difference_light_curves_find_the_variable_star(ctx):
    """Frames = the reference scene with one star brighter by delta, blurred, scaled by 0.7, on a tilted plane, with noise
    of known sigma and one 50 sigma hit: the aperture sums of D / scale give delta at the variable and 0 at the constant
    stars within 5 sigma sqrt(pi r^2) / scale (the aperture's own noise: 5 sigma of it); the hit is clipped from the fit
    and present in D."""
    from lightcurver_amd.processes.difference_imaging import difference_light_curves, match_and_subtract
    p, s = DI.PHYS, DI.physics_scene()
    sigma = np.full(p['n_frames'], p['sigma'], np.float32)
    base = dict(r=p['r'], bg_degree=1, n_sigma=4.0, sigma=sigma, ctx=ctx)
    got = match_and_subtract(s['T'], s['R'], clip_iters=2, **base)
    unclipped = match_and_subtract(s['T'], s['R'], clip_iters=0, download=('n_used',), **base)
    lc = difference_light_curves(got['diff'], got['scale'], s['xy'], p['aperture'], sigma=sigma, ctx=ctx)
    want = np.zeros(len(s['xy']))
    want[p['variable']] = p['delta']
    print('scale', got['scale'][:, 0], 'chi2', got['chi2'][:, 0], 'flux - wanted', np.round(lc['flux'] - want, 1), 'flux_err',
          lc['flux_err'][:, 0])
    assert (got['status'] == 0).all() and np.all(np.abs(got['scale'] - 0.7) < 0.01)
    assert np.allclose(lc['flux_err'], p['sigma'] * np.sqrt(np.pi * p['aperture'] ** 2) / got['scale'], rtol=1e-12)
    assert np.all(np.abs(lc['flux'] - want) < 5.0 * lc['flux_err'])
    assert np.all(got['diff'][(slice(None),) + p['hit_at']] > 40.0 * p['sigma'])
    for k in range(p['n_frames']):
        ref = DI.subtract(s['T'][k], s['R'], r=p['r'], bg_degree=1, clip_iters=2, n_sigma=4.0, sigma=p['sigma'])
        assert got['n_used'][k, 0] == ref['n_used'][0] < unclipped['n_used'][k, 0] and not ref['used'][p['hit_at']]
    # an aperture that touches the NaN border has no flux
    edge = difference_light_curves(got['diff'], got['scale'], [[3.0, 30.0]], p['aperture'], ctx=ctx)
    assert np.isnan(edge['flux']).all() and edge['flux_err'] is None
