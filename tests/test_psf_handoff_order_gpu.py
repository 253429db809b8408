"""The hand-off of the two-workgroup PSF fit (csrc/psf_kernels.h, SPLIT) at the shapes the benchmark runs.

Role 0 (chi2 gradient) and role 1 (starlet l1 term) swap their halves of dL/dB and role 1's scalar l1 value once per
iteration through L2; both apply the same AdaBelief step.  Whatever the order of stores, flags and loads inside that
hand-off, the operands and the order of the arithmetic are those of the one-workgroup form, so every output must be equal
bit for bit: grid, stars and the whole loss history (whose l1 part reaches role 0 through the hand-off's loads).  The
AdaBelief moments have no accessor of their own; they are compared through what they produce - every case below ends
with a further launch that starts from the moments the launches before it left behind.

The library takes the two-workgroup form for launches of at least four iterations whose grid is resident at once
(csrc/psf_batch.hip); LCMI_PSF_SINGLE_WG=1 forces the one-workgroup form."""
import os

import numpy as np
import pytest

from lightcurver_amd.synthetic import make_psf_dataset
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _setup(n, ss, F, S, seed, ctx, jitter):
    from lightcurver_amd.psf_batch import PsfBatch
    ds = make_psf_dataset(F=F, S=S, n=n, ss=ss, seed=seed)
    rng = np.random.default_rng(seed + 1)
    plist = [H.psf_initial_params(ds, f, ss, rng, jitter) for f in range(F)]
    b = PsfBatch(ds['data'], H.weights_from(ds), ss, ctx)
    b.set_moffat(H.moffat_array(plist))
    b.set_stars(H.stars_array(plist))
    b.set_grid(np.stack([p['B'].numpy() for p in plist]))
    return ds, plist, b


def _fit(ctx, n, S, F, seed, launches, single):
    """Loss history, grid and stars after the given launches (iterations each), in the asked form; and the number of
    two-workgroup launches that gave up and were redone (must be none: a redone launch would hide the form under test)."""
    if single:
        os.environ['LCMI_PSF_SINGLE_WG'] = '1'
    try:
        ds, plist, b = _setup(n, 2, F, S, seed, ctx, jitter=0.1)
        b.propagate_noise()
        b.set_regularization(None, 1.0, 1.0)
        for k in launches:
            b.run_adabelief(k, init_learning_rate=1e-4, schedule_learning_rate=True)
        out = (b.loss_history(), b.get_grid(), b.get_stars())
        fallbacks = b.split_fallbacks
    finally:
        os.environ.pop('LCMI_PSF_SINGLE_WG', None)
    assert fallbacks == 0
    assert out[0].shape == (F, sum(launches) + 1) and np.all(np.isfinite(out[0]))
    return out


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_c2_shape_several_hundred_iterations_both_forms(ctx):
    """F = 100, S = 8, n = 32, ss = 2: 200 workgroups at once, 400 iterations and a further launch of 50."""
    two = _fit(ctx, 32, 8, 100, 2024, (400, 50), single=False)
    one = _fit(ctx, 32, 8, 100, 2024, (400, 50), single=True)
    _same(two, one)


@pytest.mark.parametrize('k1,k2', [(150, 150), (7, 293), (151, 149)])
def test_one_launch_equals_two_launches(ctx, k1, k2):
    """The flags restart at zero and the slab parity at iteration 0 of every launch, the iteration count t0 carries on:
    k1 + k2 iterations in two launches against the same total in one, both in the two-workgroup form, and a further
    launch behind each."""
    split = _fit(ctx, 32, 8, 100, 2025, (k1, k2, 20), single=False)
    whole = _fit(ctx, 32, 8, 100, 2025, (k1 + k2, 20), single=False)
    _same(split, whole)


@pytest.mark.parametrize('launches', [(1, 10), (4, 10), (5, 10), (301, 10)])
def test_odd_and_shortest_iteration_counts(ctx, launches):
    """One iteration (the library runs it in the one-workgroup form), the shortest two-workgroup launch (4), odd counts
    (the last hand-off leaves the slab parity at 1), each followed by a launch that continues from that state."""
    two = _fit(ctx, 32, 8, 100, 2026, launches, single=False)
    one = _fit(ctx, 32, 8, 100, 2026, launches, single=True)
    _same(two, one)


@pytest.mark.parametrize('launches', [(40, 11), (5, 20)])
def test_c3_shard_shape_both_forms(ctx, launches):
    """n = 64 (N = 128), 63 frames of 8 stars - one GPU's share of C3: the pixel state lives in global memory and role 1
    steps its own copy, through the same hand-off."""
    two = _fit(ctx, 64, 8, 63, 2027, launches, single=False)
    one = _fit(ctx, 64, 8, 63, 2027, launches, single=True)
    _same(two, one)
