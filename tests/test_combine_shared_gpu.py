"""The two users of the per-pixel robust combine (robust_combine of csrc/order_stats.h) against each other, bit for bit:
stack_kernel behind align_stack_batch (samples from global memory, weight 1 / noise per pixel) and coadd_combine_kernel
behind FrameSet.coadd (keys in LDS, weight per frame), on the same samples with the same weights.

The frames are E of 32 x 32 float32, a shape legal both as stamps and as frames, E = 1, 2, 5, 6: trivial, even, odd.  The
co-add runs with the identity transform at order 1 on the frames' own grid and flux scale 1; its samples are then the
frames themselves wherever the four bilinear taps are finite and inside (asserted below), NaN on the last row and column
(a tap outside) and next to a pixel that is not finite (0 x NaN).  The stack gets exactly those samples, from the float32
restatement of the warp (tests/_coadd.py), so every pixel of the grid is compared and none is left out.  The weights are
powers of two, so the stack's 1 / (1 / w_k) is w_k exactly.

A pixel without a finite sample is NaN in every output of both; there the two kernels need not write the same NaN
pattern (0 / 0 in the stack, a constant in the co-add), so such pixels are compared as NaN and all others on raw bits."""
import numpy as np
import pytest

from tests import _coadd as CO

pytestmark = pytest.mark.gpu

N = 32
COUNTS = (1, 2, 5, 6)
WEIGHTS = (0.5, 1.0, 2.0, 4.0)
NAN_ONE, INF_ONE, NAN_ALL = (5, 7), (12, 20), (20, 9)       # apart: what each spoils (itself, left, up, up-left) is disjoint


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    """NaN at the same pixels, the same bits at every other pixel."""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def _frames(E):
    rng = np.random.default_rng(300 + E)
    f = (3.0 * rng.standard_normal((E, N, N))).astype(np.float32)       # about half the pixels negative
    f[0][NAN_ONE] = np.nan
    f[min(1, E - 1)][INF_ONE] = np.inf
    f[(slice(None),) + NAN_ALL] = np.nan
    return f


@pytest.mark.parametrize('E', COUNTS)
def test_stack_and_coadd_combine_alike(ctx, E):
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.roi_modelling import align_stack_batch
    frames = _frames(E)
    assert (frames < 0).mean() > 0.3
    w = np.array([WEIGHTS[k % len(WEIGHTS)] for k in range(E)], np.float32)
    noise = np.broadcast_to((1.0 / w)[:, None, None], (E, N, N)).astype(np.float32)
    assert np.array_equal(np.float32(1.0) / noise[:, 0, 0], w)
    identity = np.eye(3)
    samples = np.stack([CO.warp(frames[k], identity, (N, N), (0, 0), 1, 1.0, np.float32)['sample'] for k in range(E)])
    taps = np.isfinite(frames)
    taps[:, :-1, :-1] = taps[:, :-1, :-1] & taps[:, 1:, :-1] & taps[:, :-1, 1:] & taps[:, 1:, 1:]
    taps[:, -1, :] = taps[:, :, -1] = False
    assert taps.mean() > 0.9 and np.array_equal(np.isfinite(samples), taps)
    assert np.array_equal(_bits(samples[taps]), _bits(frames[taps]))        # the identity warp copies the pixels
    nothing = ~taps.any(axis=0)
    assert nothing[NAN_ALL] and nothing[-1].all() and nothing[:, -1].all()

    with FrameSet(frames, ctx) as fs:
        co = {mode: fs.coadd(np.arange(E), [identity] * E, weights=w, order=1, combine=mode, n_sigma=CO.N_SIGMA)
              for mode in CO.COMBINES}
    cube = samples[None]
    clipped = align_stack_batch(cube, noise, n_sigma=CO.N_SIGMA, clip=True, want=('stack', 'median', 'n_rejected'), ctx=ctx)
    plain = align_stack_batch(cube, noise, n_sigma=CO.N_SIGMA, clip=False, want=('stack', 'n_rejected'), ctx=ctx)

    assert _same(clipped['median'][0], co['median']['image'])
    assert _same(clipped['stack'][0], co['sigma_clip']['image'])
    assert np.array_equal(clipped['n_rejected'][0], co['sigma_clip']['n_rejected'])
    assert _same(plain['stack'][0], co['mean']['image'])
    assert not plain['n_rejected'].any() and not co['mean']['n_rejected'].any() and not co['median']['n_rejected'].any()
    for image in (clipped['median'][0], clipped['stack'][0], plain['stack'][0], *(co[mode]['image'] for mode in CO.COMBINES)):
        assert np.array_equal(np.isnan(image), nothing)
    for mode in CO.COMBINES:
        assert np.array_equal(co[mode]['count'] + co[mode]['n_rejected'], taps.sum(axis=0))
    rejected = int((clipped['n_rejected'] > 0).sum())
    print(f'E={E}: {rejected} pixels reject something, {int(nothing.sum())} without a sample')
    if E >= 5:
        assert rejected > 0
