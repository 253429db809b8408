"""The two-workgroup PSF kernels that are compiled for the launch they get (csrc/psf_kernels.h, LOOP_ONLY): the library runs
that form only for the optimisation loop - mode 1, no eval outputs, a regulariser, no heal (csrc/psf_batch.hip, `split`) - so
the N = 64 (C2) and N = 32 kernels take those four facts as constants and test none of them in the loop.  Role 0 of the C2
kernel also keeps the addresses it works by across the loop top and no longer zeroes the stars' gradient slots, which are all
assigned before they are read (TOP_LIVE).  N = 48 and N = 128 keep the run-time tests ("PSF fit: the two-workgroup
loop without its launch constants").

No operand and no order of a sum changes, so the one-workgroup form, which keeps every test and serves every other launch,
must give the same bits.  It is selected by LCMI_PSF_SINGLE_WG=1, which the library reads at every launch; like the tests this
one is modelled on (tests/test_psf_task_ahead_gpu.py) the variable is set and removed inside this process, no child is started.

Subsampling 2, every star its own flux (two decades inside a frame) and its own offset:
  n = 32 (C2), F = 3: S = 1, 8, 12; launches of 4 and of 5 + 4 + 4; once at a constant learning rate
  n = 16 (N = 32 kernel, 4 pixels per thread), F = 3, S = 8
  n = 64 (N = 128 kernel, pixel state in memory; keeps its run-time tests), F = 2, S = 8, launches of 4 + 4
Compared: loss history, pixel grid B, stars, and - after the fit - evaluate() with every output and results(), which run the
one-workgroup kernel on either side and so show that the outputs path is what it was.  The AdaBelief moments of grid and stars
have no accessor; they are compared through what they produce, the launches that continue from them: every shape and the
ext_grad case have a case of more than one launch (5 + 4 + 4, or 4 + 4 at n = 64 and with ext_grad).

ext_grad: run_adabelief itself takes no such switch, but the batch keeps the one the distortion scheme last set
(lc_psf_distortion_backward), so run_adabelief(4) behind a backward call is a two-workgroup launch with ext_grad - the
combination the kernel keeps a run-time test for.  One case runs it, twice in a row.

That these batches do run in two workgroups is shown by launches made to give up (LCMI_PSF_FORCE_ABORT): only a two-workgroup
launch can, the batch counts it, and the heal launch behind it - the one-workgroup kernel with heal = 1 - must restore and
redo the work."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import _psf_geometry as G

pytestmark = pytest.mark.gpu

SS = 2
AB = dict(init_learning_rate=1e-4)
_problems, _single = {}, {}


def _problem(n, S, F):
    """Stamps and starting parameters, made once per shape and left unchanged."""
    key = (n, S, F)
    if key not in _problems:
        lim = n / 4.0
        seed = 7000 + 100 * n + S
        xy = np.random.default_rng(seed).uniform(-lim, lim, (F, S, 2))
        ds = G.draw_dataset(n, SS, G.displaced(xy, seed + 1), seed + 2)
        _problems[key] = (ds, G.params_at(ds, xy, seed + 3), xy)
    return _problems[key]


def _batch(ctx, n, S, F):
    from lightcurver_amd.psf_batch import PsfBatch
    ds, plist, _ = _problem(n, S, F)
    b = PsfBatch(ds['data'], H.weights_from(ds), SS, ctx)
    b.set_moffat(H.moffat_array(plist))
    b.set_stars(H.stars_array(plist))
    b.set_grid(np.stack([p['B'].numpy() for p in plist]))
    b.propagate_noise()
    b.set_regularization(None, 1.0, 1.0)
    return b


def _with_ext_grad(ctx, b, n, S, F):
    """Leaves an external gradient in `b` and the switch for it set: the batch's own grid resampled to F * S single-star
    frames (identity plus a small distortion), their d loss / d B gathered back by the adjoint."""
    from lightcurver_amd.psf_batch import PsfBatch
    ds, plist, _ = _problem(n, S, F)
    rng = np.random.default_rng(77)
    star_b = PsfBatch(ds['data'].reshape(F * S, 1, n, n), H.weights_from(ds).reshape(F * S, 1, n, n), SS, ctx)
    star_b.set_moffat(np.repeat(H.moffat_array(plist), S, axis=0))
    star_b.set_stars(H.stars_array(plist).reshape(F * S, 1, 4))
    star_b.set_regularization(None, 0.0, 0.0)
    b.set_distortion(S, rng.uniform(-0.04, 0.04, (F, 9)), rng.uniform(-0.5, 0.5, (F, S, 2)))
    b.distortion_forward(star_b)
    star_b.evaluate()
    b.distortion_backward(star_b)
    g = b.get_ext_grad()
    star_b.close()
    assert np.all(np.isfinite(g)) and np.count_nonzero(g) > g.size // 2
    return g


def _outputs(b):
    out = dict(loss_history=b.loss_history(), grid=b.get_grid(), stars=b.get_stars())
    out.update({'evaluate.' + k: v for k, v in b.evaluate(model=True).items()})
    out.update({'results.' + k: v for k, v in b.results().items()})
    return out


def _fit(ctx, n, S, F, launches, single, schedule=True, ext_grad=False):
    key = (n, S, F, launches, schedule, ext_grad)
    if single and key in _single:
        return _single[key]
    if single:
        os.environ['LCMI_PSF_SINGLE_WG'] = '1'
    try:
        b = _batch(ctx, n, S, F)
        if ext_grad:
            _with_ext_grad(ctx, b, n, S, F)
        for k in launches:
            b.run_adabelief(k, schedule_learning_rate=schedule, **AB)
        out = _outputs(b)
        fallbacks = b.split_fallbacks
        b.close()
    finally:
        os.environ.pop('LCMI_PSF_SINGLE_WG', None)
    assert fallbacks == 0
    assert out['loss_history'].shape == (F, sum(launches) + 1)
    for k, v in out.items():
        assert np.all(np.isfinite(v)), k
    if single:
        _single[key] = out
    return out


def _same(two, one):
    assert two.keys() == one.keys()
    assert {'evaluate.model', 'evaluate.grad_grid', 'evaluate.grad_stars', 'results.residuals'} <= set(two)
    for k in two:
        np.testing.assert_array_equal(two[k], one[k], err_msg=k)


CASES = [(32, 1, 3), (32, 8, 3), (32, 12, 3), (16, 8, 3)]


def test_problems_have_distinct_stars():
    for n, S, F in CASES + [(64, 8, 2)]:
        ds, plist, xy = _problem(n, S, F)
        for f in range(F):
            assert len(set(xy[f, :, 0])) == S and len(set(xy[f, :, 1])) == S
            assert len(set(np.asarray(plist[f]['a']).tolist())) == S
            assert np.all(np.abs(xy[f]) <= n / 4.0)


@pytest.mark.parametrize('launches', [(4,), (5, 4, 4)])
@pytest.mark.parametrize('n,S,F', CASES)
def test_two_workgroups_equal_one(ctx, n, S, F, launches):
    _same(_fit(ctx, n, S, F, launches, single=False), _fit(ctx, n, S, F, launches, single=True))


def test_constant_learning_rate(ctx):
    _same(_fit(ctx, 32, 8, 3, (5, 4, 4), single=False, schedule=False), _fit(ctx, 32, 8, 3, (5, 4, 4), single=True, schedule=False))


def test_state_in_memory_kernel(ctx):
    """n = 64: the N = 128 two-workgroup kernel, which keeps its run-time tests.  The second launch continues from the moments
    the first left, of grid and stars (the give-up case below shares this reference)."""
    _same(_fit(ctx, 64, 8, 2, (4, 4), single=False), _fit(ctx, 64, 8, 2, (4, 4), single=True))


def test_external_gradient_in_two_workgroups(ctx):
    """run_adabelief(4), twice, with the external gradient of the distortion scheme switched on: ext_grad stays a run-time
    input of the two-workgroup kernel, and the second launch continues from the moments of the first.  The fit with it must
    differ from the fit without (else the case would show nothing)."""
    two = _fit(ctx, 32, 8, 3, (4, 4), single=False, ext_grad=True)
    _same(two, _fit(ctx, 32, 8, 3, (4, 4), single=True, ext_grad=True))
    assert not np.array_equal(two['grid'], _fit(ctx, 32, 8, 3, (4, 4), single=True)['grid'])


@pytest.mark.parametrize('n,S,F', [(32, 8, 3), (16, 8, 3), (64, 8, 2)])
def test_these_batches_run_in_two_workgroups_and_heal(ctx, n, S, F):
    """Role 1 of frame 0 told to stop showing up at iteration 2 (the library's test hook; tests/test_psf_task_ahead_gpu.py uses
    it the same way).  A one-workgroup launch has no partner to miss; a two-workgroup launch gives up, is redone by the heal
    launch, and is counted.  The redone launch and the two-workgroup launch behind it leave what the one-workgroup form leaves."""
    b = _batch(ctx, n, S, F)
    os.environ['LCMI_PSF_FORCE_ABORT'] = '2'
    try:
        b.run_adabelief(4, schedule_learning_rate=True, **AB)
    finally:
        os.environ.pop('LCMI_PSF_FORCE_ABORT', None)
    assert b.split_fallbacks == 1
    b.run_adabelief(4, schedule_learning_rate=True, **AB)
    assert b.split_fallbacks == 1
    got = _outputs(b)
    b.close()
    _same(got, _fit(ctx, n, S, F, (4, 4), single=True))
