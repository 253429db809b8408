"""The two-workgroup PSF fit at n = 32 with role 0's waits taken off its chain (csrc/psf_kernels.h, TRIM): role 0's half
stored straight behind the transposed row pass, with one barrier and a wave-level sync where there were three barriers, and
T of the next iteration written behind the pixel step so that the closing barrier opens the first group of stars.

None of it moves an operand or the order of a sum, so the one-workgroup form (LCMI_PSF_SINGLE_WG=1), which has none of it,
must give the same bits: loss history, grid and stars.  The cases are the smallest at which each item can go wrong:
S = 1 and 8 (one group of stars), S = 12 (two groups: the second still needs its opening barrier); a launch of 4 (the
shortest the library runs in two workgroups); launches of 5 + 4 and 7 + 33 with one more of 4 behind each (schedule entries
picked by t0 + it across launches, T written in front of the loop from the grid the launch before left, the moments carried
over); and a constant learning rate."""
import os

import numpy as np
import pytest

from tests.test_psf_handoff_order_gpu import _setup

pytestmark = pytest.mark.gpu

N_STAMP, F = 32, 3


def _fit(ctx, S, launches, single, schedule=True):
    if single:
        os.environ['LCMI_PSF_SINGLE_WG'] = '1'
    try:
        ds, plist, b = _setup(N_STAMP, 2, F, S, 2030 + S, ctx, jitter=0.1)
        b.propagate_noise()
        b.set_regularization(None, 1.0, 1.0)
        for k in launches:
            b.run_adabelief(k, init_learning_rate=1e-4, schedule_learning_rate=schedule)
        out = (b.loss_history(), b.get_grid(), b.get_stars())
        fallbacks = b.split_fallbacks
    finally:
        os.environ.pop('LCMI_PSF_SINGLE_WG', None)
    assert fallbacks == 0
    assert out[0].shape == (F, sum(launches) + 1) and np.all(np.isfinite(out[0]))
    return out


def _same(two, one):
    for name, x, y in zip(('loss history', 'grid', 'stars'), two, one):
        np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize('launches', [(4,), (5, 4, 4), (7, 33, 4)])
@pytest.mark.parametrize('S', [1, 8, 12])
def test_two_workgroups_equal_one(ctx, S, launches):
    _same(_fit(ctx, S, launches, single=False), _fit(ctx, S, launches, single=True))


def test_constant_learning_rate(ctx):
    _same(_fit(ctx, 8, (7, 33, 4), single=False, schedule=False), _fit(ctx, 8, (7, 33, 4), single=True, schedule=False))
