"""The two-workgroup PSF fit at n = 32, subsampling 2, whose role 0 runs its wave tasks as a software pipeline
(csrc/psf_kernels.h, TASK_AHEAD): the row pass of a wave's next task is issued among the transposed column pass of the task
at hand, the first row pass stands in front of the loop and the last transposed pass alone.  The same kernel writes the
zero columns of V once per launch, in front of the iteration loop, where the edge tasks wrote them in every iteration
(V_ZERO_ONCE).

No operand, no lane's item and no order of a sum changes, so the one-workgroup form (LCMI_PSF_SINGLE_WG=1), which keeps the
plain task loop, must give the same bits.  n = 32 at subsampling 2 is the only stamp size that runs this kernel; F = 3 is
taken in two workgroups per frame like in tests/test_psf_serial_trim_gpu.py (no launch may fall back: asserted).  That the
library does take the two-workgroup form for these batches - it decides from the grid and the device, and with the
one-workgroup form on both sides the comparison would pass vacuously - is shown by the launch that is made to give up:
only a two-workgroup launch can, and the batch counts it.

Star counts - a wave's tasks are (star, block of 8 columns) number wid, wid + 8, ... of a group of 8 stars:
  S = 1   four waves have one task, four have none: the row pass in front of the loop is followed by the lone transposed pass
  S = 3   waves with two tasks (stars 0 and 2) beside waves with one (star 1)
  S = 8   four tasks per wave
  S = 12  a second group of stars whose later tasks are skipped; V is reused behind the group's barrier, its zero columns
          are not rewritten
Launches: 4 (the shortest the library runs in two workgroups), 5 + 4 + 4, and 5 + 4 + 4 at a constant learning rate.  The
AdaBelief moments of grid and stars have no accessor; they are compared through what they produce: the launches that
continue from the moments the launches before left behind.

Positions: a pipelined wave holds the taps and window bases of two stars at once, and consecutive tasks of a wave belong to
stars s and s + 2.  Every star has its own flux (two decades inside a frame) and its own offset; star 0 sits at +-n/4 in x and
-+n/4 in y, star 1 at +-n/4 in y, star 2 at -+n/4 in x (the sign alternates with the frame), so that stars 0 and 2 - consecutive
tasks of waves 0 to 3 - have window bases at opposite ends of the aprons, in both passes.

evaluate() is not part of this test: the library runs single evaluations in the one-workgroup form (csrc/psf_batch.hip), so
the model output and the exported gradients never come out of this kernel."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import _psf_geometry as G

pytestmark = pytest.mark.gpu

N_STAMP, SS, F = 32, 2, 3
_problems = {}


def _problem(S):
    """Stamps and starting parameters, made once per star count and left unchanged."""
    if S not in _problems:
        lim = N_STAMP / 4.0
        rng = np.random.default_rng(9100 + S)
        xy = rng.uniform(-lim, lim, (F, S, 2))
        for f in range(F):
            sign = 1.0 if f % 2 == 0 else -1.0
            xy[f, 0] = (sign * lim, -sign * lim)
            if S > 1:
                xy[f, 1, 1] = sign * lim
            if S > 2:
                xy[f, 2, 0] = -sign * lim
        ds = G.draw_dataset(N_STAMP, SS, G.displaced(xy, 9200 + S), 9300 + S)
        _problems[S] = (ds, G.params_at(ds, xy, 9400 + S), xy)
    return _problems[S]


def _batch(ctx, S):
    from lightcurver_amd.psf_batch import PsfBatch
    ds, plist, _ = _problem(S)
    b = PsfBatch(ds['data'], H.weights_from(ds), SS, ctx)
    b.set_moffat(H.moffat_array(plist))
    b.set_stars(H.stars_array(plist))
    b.set_grid(np.stack([p['B'].numpy() for p in plist]))
    b.propagate_noise()
    b.set_regularization(None, 1.0, 1.0)
    return b


def _fit(ctx, S, launches, single, schedule=True):
    if single:
        os.environ['LCMI_PSF_SINGLE_WG'] = '1'
    try:
        b = _batch(ctx, S)
        for k in launches:
            b.run_adabelief(k, init_learning_rate=1e-4, schedule_learning_rate=schedule)
        res = b.results()
        out = dict(loss_history=b.loss_history(), grid=b.get_grid(), stars=b.get_stars(),
                   **{'results.' + k: v for k, v in res.items()})
        fallbacks = b.split_fallbacks
        b.close()
    finally:
        os.environ.pop('LCMI_PSF_SINGLE_WG', None)
    assert fallbacks == 0
    assert out['loss_history'].shape == (F, sum(launches) + 1)
    for k, v in out.items():
        assert np.all(np.isfinite(v)), k
    return out


def _same(two, one):
    assert two.keys() == one.keys()
    for k in two:
        np.testing.assert_array_equal(two[k], one[k], err_msg=k)


def test_problem_has_the_positions_it_is_about():
    """Stars 0 and 2 (consecutive tasks of a wave) at opposite limits in x, stars 0 and 1 at opposite limits in y; all
    offsets and fluxes of a frame distinct."""
    lim = N_STAMP / 4.0
    for S in (1, 3, 8, 12):
        ds, plist, xy = _problem(S)
        for f in range(F):
            assert abs(xy[f, 0, 0]) == lim and xy[f, 0, 1] == -xy[f, 0, 0]
            if S > 2:
                assert xy[f, 2, 0] == -xy[f, 0, 0] and xy[f, 1, 1] == xy[f, 0, 0]
                assert len(set(np.round(SS * xy[f, :, 0]).astype(int))) > 2  # more than two window bases in x
            assert len(set(xy[f, :, 0])) == S and len(set(xy[f, :, 1])) == S
            assert len(set(np.asarray(plist[f]['a']).tolist())) == S


@pytest.mark.parametrize('S', [1, 12])
def test_these_batches_run_in_two_workgroups(ctx, S):
    """The shortest launch the other tests make (4 iterations), with role 1 of frame 0 told to stop showing up at iteration 2
    (LCMI_PSF_FORCE_ABORT, the library's test hook; tests/test_psf_gpu.py uses it the same way).  A one-workgroup launch has no
    partner to miss and reports nothing; a two-workgroup launch gives up, is redone, and is counted.  The redone launch and the
    two-workgroup launch behind it must leave what the one-workgroup form leaves."""
    b = _batch(ctx, S)
    os.environ['LCMI_PSF_FORCE_ABORT'] = '2'
    try:
        b.run_adabelief(4, init_learning_rate=1e-4, schedule_learning_rate=True)
    finally:
        os.environ.pop('LCMI_PSF_FORCE_ABORT', None)
    assert b.split_fallbacks == 1
    b.run_adabelief(4, init_learning_rate=1e-4, schedule_learning_rate=True)
    assert b.split_fallbacks == 1
    got = dict(loss_history=b.loss_history(), grid=b.get_grid(), stars=b.get_stars())
    b.close()
    one = _fit(ctx, S, (4, 4), single=True)
    for k in got:
        np.testing.assert_array_equal(got[k], one[k], err_msg=k)


@pytest.mark.parametrize('launches', [(4,), (5, 4, 4)])
@pytest.mark.parametrize('S', [1, 3, 8, 12])
def test_pipelined_tasks_equal_the_plain_loop(ctx, S, launches):
    _same(_fit(ctx, S, launches, single=False), _fit(ctx, S, launches, single=True))


@pytest.mark.parametrize('S', [1, 3, 8, 12])
def test_constant_learning_rate(ctx, S):
    _same(_fit(ctx, S, (5, 4, 4), single=False, schedule=False), _fit(ctx, S, (5, 4, 4), single=True, schedule=False))
