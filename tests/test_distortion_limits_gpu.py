"""The field-distortion kernels (csrc/psf_distort.h, csrc/distort.hip) at the limits the fit can reach, against the float64
restatement of tests/_distortion.py (pinned on the CPU by tests/test_distortion_cpu.py): matrices with entries up to 0.5 from
the identity (the 5 x 5 window of the adjoint and its clamp), grids whose largest values sit on the border (the clipping of
the window), 1 / 5 / 16 stars, three frames with different coefficients, N^2 that is no multiple of 256.

Tolerance of the comparisons with float64 (nothing in it comes from the device).  The device forms the sample positions in
float32; what that costs is measured on the CPU from the reference alone, as |position_rounding - float64| with NumPy's
float32.  NumPy's roundings and the device's are different draws of the same size (the compiler may contract a product into
a sum where NumPy rounds twice), so one pixel's NumPy figure does not bound that pixel on the device: the bound of a pixel is
4 x the largest figure of its image (one star's image for the forward kernel, one frame's gradient for the adjoint, one
position's PSF for lc_apply_distortion) plus 8 * 2^-24 * sum |w * value| of that pixel for the float32 products and sums.
Every pixel of every case is asserted.

Largest error seen on the MI355X and the bound at that pixel, per shape (n, ss), over all cases and S in {1, 5, 16} (absolute:
the resampled grids reach 8 / det A, about 150 in the near-singular case; the tests print the figures, pytest -s):

    (n, ss)   forward: error   bound      adjoint: error   bound      largest first term / max |value|   worst case
    (16, 1)   9.4e-4           3.8e-3     9.3e-4           3.8e-3     5.7e-5                             near-singular
    (16, 2)   2.8e-3           1.1e-2     2.7e-2           1.1e-1     1.2e-4                             near-singular
    (24, 2)   4.9e-3           2.0e-2     2.5e-2           1.0e-1     2.4e-4                             near-singular
    (32, 2)   1.0e-4           4.1e-4     2.5e-4           9.8e-4     8.7e-5                             corners, stars 1..15
    (64, 2)   2.4e-4           9.6e-4     9.8e-4           3.5e-3     2.1e-4                             corners, stars 1..15

The first term passes 1e-4 of max |value| in the near-singular case from N = 32 on (forward at S >= 5, adjoint at N = 48) and,
at N = 128, for the stars of the corner frames that do not sit in the corner of the field.  Neither sits on a cell border: in
the first A^-1 has entries near 10, so a float32 rounding of A^-1 moves a sample by 10 * 2^-24 * N / 2 pixels; in the second it
is the size of the grid, with noise of amplitude 8 and alternating sign on the outermost rows.  Where the positions are exact
in float32 (the identity, the corner matrices themselves: S = 1 at the two large shapes) the first term is zero and the whole
bound is the second term: the errors there are 2e-7 (forward) and 9e-7 (adjoint) under bounds of 1.1e-6 and 4.3e-6.
The device's largest error is within a few per cent of NumPy's largest float32 figure in every shape, a quarter of the bound.
No case inside the supported range failed.  A library built with hv and hu exchanged in the adjoint fails 27 of the 31
adjoint tests (per pixel, adjointness and padded stars).
"""
import numpy as np
import pytest

from oracle import model as om
from oracle import optim as oo
from tests import _distortion as D
from tests import helpers as H

pytestmark = pytest.mark.gpu

F = 3
SHAPES = [(16, 1), (16, 2), (24, 2)]            # every case
CORNER_SHAPES = [(32, 2), (64, 2)]              # the corners only
RUNS = [(n, ss, S) for n, ss in SHAPES + CORNER_SHAPES for S in (1, 5, 16)]
SENTINEL = np.float32(-7.25)


def _groups(n, ss):
    cases = D.CASES if (n, ss) in SHAPES else D.CORNERS
    return [[cases[(i + k) % len(cases)] for k in range(F)] for i in range(0, len(cases), F)]


_cache = {}


def _device(ctx, n, ss, S):
    """Everything the device computes for one (n, ss, S), once: per group of F frames (different coefficients and grids per
    frame) the resampled grids, the gradient g the star batch left on the device, the adjoint of g, and for 8 more random
    grids the two sides of <forward(B), g> = <B, adjoint(g)>."""
    key = (n, ss, S)
    if key in _cache:
        return _cache[key]
    from lightcurver_amd.psf_batch import PsfBatch
    N = n * ss
    rng = np.random.default_rng(1000 * n + 10 * ss + S)
    # noise stamps with unit weights: the gradient of the star batch is dense up to the border of the grid
    star_b = PsfBatch(rng.standard_normal((F * S, 1, n, n)), np.ones((F * S, 1, n, n)), ss, ctx)
    frame_b = PsfBatch(np.zeros((F, 1, n, n)), np.zeros((F, 1, n, n)), ss, ctx)
    star_b.set_moffat_q(np.tile([0.1, 0.02, 0.15, 2.5], (F * S, 1)))
    st = np.zeros((F * S, 1, 4))
    st[..., 0] = rng.uniform(0.5, 2.0, (F * S, 1))
    st[..., 1:3] = rng.uniform(-1.0, 1.0, (F * S, 1, 2))
    star_b.set_stars(st)
    star_b.set_regularization(None, 0.0, 0.0)
    out = []
    for group in _groups(n, ss):
        coef = np.stack([c for _, c, _ in group])
        xy = np.stack([p[:S] for _, _, p in group])
        B = np.stack([D.noise_grid(rng, N) for _ in range(F)])
        frame_b.set_grid(B)
        frame_b.set_distortion(S, coef, xy)
        frame_b.distortion_forward(star_b)
        fwd = star_b.get_grid().reshape(F, S, N, N)
        # grad_grid is lc_psf_batch's o_ggrid, the buffer lc_psf_distortion_backward hands to the adjoint kernel
        g = star_b.evaluate()['grad_grid'].reshape(F, S, N, N)
        frame_b.distortion_backward(star_b)
        eg = frame_b.get_ext_grad()
        pairs = []
        for _ in range(8):
            Bk = rng.standard_normal((F, N, N)).astype(np.float32)
            frame_b.set_grid(Bk)
            frame_b.distortion_forward(star_b)
            fk = star_b.get_grid().reshape(F, S, N, N).astype(np.float64)
            for f in range(F):
                t = fk[f] * g[f].astype(np.float64)
                pairs.append((group[f][0], t.sum(), (Bk[f].astype(np.float64) * eg[f]).sum(), np.abs(t).sum()))
        out.append(dict(names=[c[0] for c in group], coef=coef, xy=xy, B=B, fwd=fwd, g=g, eg=eg, pairs=pairs))
    star_b.close()
    frame_b.close()
    _cache[key] = out
    return out


def _operators(N, coef, xy):
    """(float64 operator, the same with float32 positions) of every (frame, star)."""
    a = D.matrices(coef, xy)
    a32 = D.matrices(np.float32(coef), np.float32(xy), np.float32)
    Fr, S = a[0].shape
    return [[(D.warp_operator(N, a[0][f, s], a[1][f, s], a[2][f, s]),
              D.position_rounding(N, a32[0][f, s], a32[1][f, s], a32[2][f, s])) for s in range(S)] for f in range(Fr)]


def _group_operators(grp, N):
    if 'ops' not in grp:
        grp['ops'] = _operators(N, grp['coef'], grp['xy'])
    return grp['ops']


def _report(what, n, ss, S, worst, above):
    err, bound, rounding, name = worst
    print(f'{what} (n, ss, S) = ({n}, {ss}, {S}): largest error {err:.3e} (bound there {bound:.3e}) in {name}; '
          f'largest rounding term {rounding:.2e} of max |value|; above 1e-4 in: {sorted(above) or "none"}')


@pytest.mark.parametrize('n,ss,S', RUNS)
def test_forward_matches_float64(ctx, n, ss, S):
    N = n * ss
    worst, rounding, above = (0.0, 0.0, 0.0, ''), 0.0, set()
    for grp in _device(ctx, n, ss, S):
        ops = _group_operators(grp, N)
        for f in range(F):
            for s in range(S):
                op, opr = ops[f][s]
                ref = op.warp(grp['B'][f])
                first = 4.0 * np.abs(opr.warp(grp['B'][f]) - ref).max()
                bound = first + 8.0 * D.EPS32 * op.warp_abs(grp['B'][f])
                err = np.abs(grp['fwd'][f, s] - ref)
                rounding = max(rounding, first / np.abs(ref).max())
                if first > 1e-4 * np.abs(ref).max():
                    above.add(grp['names'][f])
                i = np.argmax(err)
                if err.flat[i] >= worst[0]:
                    worst = (err.flat[i], bound.flat[i], rounding, grp['names'][f])
                assert np.all(err <= bound), (grp['names'][f], s, float(err.flat[i]), float(bound.flat[i]))
    _report('forward', n, ss, S, worst[:2] + (rounding,) + worst[3:], above)


@pytest.mark.parametrize('n,ss,S', RUNS)
def test_adjoint_matches_float64_per_pixel(ctx, n, ss, S):
    """The reference gets the device's own g: only psf_warp_adjoint_kernel is under test.  N^2 = 2304 is no multiple of 256,
    N = 128 gives 64 blocks along grid.y, S = 16 fills the shared array of matrices."""
    N = n * ss
    worst, rounding, above = (0.0, 0.0, 0.0, ''), 0.0, set()
    for grp in _device(ctx, n, ss, S):
        ops = _group_operators(grp, N)
        for f in range(F):
            g = grp['g'][f]
            assert np.all(np.isfinite(g)) and (g != 0).mean() > 0.99          # dense up to the border
            ref = D.adjoint([o[0] for o in ops[f]], g)
            first = 4.0 * np.abs(D.adjoint([o[1] for o in ops[f]], g) - ref).max()
            bound = first + 8.0 * D.EPS32 * sum(o[0].adjoint_abs(gs) for o, gs in zip(ops[f], g))
            err = np.abs(grp['eg'][f] - ref)
            rounding = max(rounding, first / np.abs(ref).max())
            if first > 1e-4 * np.abs(ref).max():
                above.add(grp['names'][f])
            i = np.argmax(err)
            if err.flat[i] >= worst[0]:
                worst = (err.flat[i], bound.flat[i], rounding, grp['names'][f])
            assert np.all(err <= bound), (grp['names'][f], float(err.flat[i]), float(bound.flat[i]))
    _report('adjoint', n, ss, S, worst[:2] + (rounding,) + worst[3:], above)


@pytest.mark.parametrize('n,ss,S', RUNS)
def test_the_two_kernels_are_adjoint_to_each_other(ctx, n, ss, S):
    """<forward(B), g> = <B, adjoint(g)>, both sides summed in float64 on the host from what the device returned.  Both
    kernels take the positions from the same float32 warp_sample, so their rounding cancels: a window candidate that the
    adjoint leaves out shows here at its full weight."""
    worst = 0.0
    for grp in _device(ctx, n, ss, S):
        for name, lhs, rhs, size in grp['pairs']:
            worst = max(worst, abs(lhs - rhs) / size)
            assert abs(lhs - rhs) <= 1e-5 * size, (name, lhs, rhs, size)
    print(f'adjointness (n, ss, S) = ({n}, {ss}, {S}): largest |lhs - rhs| / sum |terms| = {worst:.2e}')


def test_padded_stars_do_not_reach_the_gradient(ctx):
    """A frame with fewer stars than S: the unused slots carry zero weight and xy = 0 (as the facade leaves them).  The
    adjoint must be the same, bit for bit, when those slots hold other coordinates."""
    from lightcurver_amd.psf_batch import PsfBatch
    n, ss, S = 16, 2, 5
    N = n * ss
    used = [3, 5, 1]
    rng = np.random.default_rng(77)
    data, wgt = rng.standard_normal((F, S, n, n)), np.ones((F, S, n, n))
    st = np.zeros((F, S, 4))
    st[..., 0] = rng.uniform(0.5, 2.0, (F, S))
    st[..., 1:3] = rng.uniform(-1.0, 1.0, (F, S, 2))
    xy = np.stack([D.CASES[i][2][:S] for i in (-1, 3, 14)])
    coef = np.stack([D.CASES[i][1] for i in (-1, 3, 14)])
    for f in range(F):
        data[f, used[f]:], wgt[f, used[f]:], st[f, used[f]:], xy[f, used[f]:] = 0.0, 0.0, 0.0, 0.0
    other = xy.copy()
    for f in range(F):
        other[f, used[f]:] = rng.uniform(-0.5, 0.5, (S - used[f], 2))
    B = np.stack([D.noise_grid(rng, N) for _ in range(F)])
    got = []
    for coords in (xy, other):
        star_b = PsfBatch(data.reshape(F * S, 1, n, n), wgt.reshape(F * S, 1, n, n), ss, ctx)
        frame_b = PsfBatch(np.zeros((F, 1, n, n)), np.zeros((F, 1, n, n)), ss, ctx)
        star_b.set_moffat_q(np.tile([0.1, 0.02, 0.15, 2.5], (F * S, 1)))
        star_b.set_stars(st.reshape(F * S, 1, 4))
        star_b.set_regularization(None, 0.0, 0.0)
        frame_b.set_grid(B)
        frame_b.set_distortion(S, coef, coords)
        frame_b.distortion_forward(star_b)
        g = star_b.evaluate()['grad_grid'].reshape(F, S, N, N)
        frame_b.distortion_backward(star_b)
        got.append((g, frame_b.get_ext_grad()))
        star_b.close()
        frame_b.close()
    for f in range(F):
        assert not got[0][0][f, used[f]:].any() and np.all(got[0][0][f, :used[f]].reshape(used[f], -1).any(axis=1))
    assert np.all(np.abs(got[0][1]).max(axis=(1, 2)) > 0)
    assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))
    # and it is the adjoint of the used stars alone
    for f in range(F):
        ops = _operators(N, coef[f:f + 1], xy[f:f + 1, :used[f]])[0]
        ref = D.adjoint([o[0] for o in ops], got[0][0][f, :used[f]])
        assert H.rel_err(got[0][1][f], ref) < 1e-4


# ---- Moffat by its quadratic form ---------------------------------------------------------------------------------------------
def _moffat_cases(n, ss):
    """theta of every frame: beta in {1.1, 2.5, 50}, axis ratios 1 and 4, both signs of q12, the FWHM at the facade's bounds."""
    lo, hi = 0.5 / ss, n / 2.0
    return np.array([(fx, fy, phi, beta) for fx, fy in ((lo, lo), (hi, hi), (lo, 4 * lo), (hi, hi / 4), (3.0, 3.0), (2.0, 8.0))
                     for phi in (0.5, -0.5) for beta in (1.1, 2.5, 50.0)])


@pytest.mark.parametrize('n,ss', [(16, 1), (16, 2), (64, 2)])
def test_moffat_by_quadratic_form_matches_float64(ctx, n, ss):
    """moffat_q_raster_kernel and moffat_q_grad_kernel work in double on float32 inputs.  Raster: read back as the narrow PSF
    of a batch with a zero grid, (float)(Tm / sum Tm) - three float32 roundings, so 4 * 2^-24 relative (and the smallest
    normal float32 where the value underflows).  Gradient: the reference takes the gT the device produced (grad_grid, which
    is o_gT when the regularisation is off); the result is one float32 rounding (2^-23 allowed) of a difference of sums in
    double, whose error is bounded by N^2 * 2^-53 ~ 2e-12 of the terms that cancel (1e-10 allowed)."""
    from lightcurver_amd.psf_batch import PsfBatch
    from lightcurver_amd.starred.procedures.psf_routines import quadratic_forms
    N = n * ss
    theta = _moffat_cases(n, ss)
    Fm = len(theta)
    rng = np.random.default_rng(n * ss)
    q = np.float32(quadratic_forms(np.concatenate([theta, np.zeros((Fm, 9))], axis=1), np.zeros((Fm, 1, 2)), ss)[:, 0])
    assert (q[:, 1] > 0).any() and (q[:, 1] < 0).any()
    b = PsfBatch(rng.standard_normal((Fm, 1, n, n)), np.ones((Fm, 1, n, n)), ss, ctx)
    b.set_moffat_q(q)
    st = np.zeros((Fm, 1, 4))
    st[..., 0] = 1.0
    st[..., 1:3] = rng.uniform(-1.0, 1.0, (Fm, 1, 2))
    b.set_stars(st)
    b.set_grid(None)
    b.set_regularization(None, 0.0, 0.0)
    out = b.evaluate(model=True)
    narrow = b.results()['narrow_psf']
    b.close()
    worst_r = worst_g = 0.0
    for f in range(Fm):
        ref = D.moffat_q(N, q[f].astype(np.float64))
        err = np.abs(narrow[f] - ref)
        tol = 4.0 * D.EPS32 * ref + 1.2e-38
        worst_r = max(worst_r, float((err / tol).max()))
        assert np.all(err <= tol), (theta[f], float((err / tol).max()))
        gT = out['grad_grid'][f]
        assert np.all(np.isfinite(gT)) and gT.any()
        gref, size = D.moffat_q_grad(N, q[f].astype(np.float64), gT, scale=True)
        gerr = np.abs(out['grad_moffat'][f] - gref)
        gtol = 2.0 * D.EPS32 * np.abs(gref) + 1e-10 * size + 1.2e-38
        worst_g = max(worst_g, float((gerr / gtol).max()))
        assert np.all(gerr <= gtol), (theta[f], out['grad_moffat'][f], gref, gtol)
    print(f'moffat_q N = {N}: largest error / tolerance: raster {worst_r:.2f}, gradient {worst_g:.2f}')


# ---- the optimiser steps of the two-batch scheme ----------------------------------------------------------------------------
def _problem(Fr, S, n, ss, seed, span=0.15):
    from lightcurver_amd.synthetic import make_psf_dataset
    ds = make_psf_dataset(F=Fr, S=S, n=n, ss=ss, seed=seed)
    rng = np.random.default_rng(seed + 1)
    plist = [H.psf_initial_params(ds, f, ss, rng, 0.2) for f in range(Fr)]
    xy = rng.uniform(-0.5, 0.5, (Fr, S, 2))
    dist = rng.uniform(-span, span, (Fr, 9))
    for f in range(Fr):
        plist[f]['dist'] = om.T(dist[f])
        plist[f]['B'] = om.T(2e-4 * rng.standard_normal(plist[f]['B'].shape))
    return ds, plist, xy, dist


def _two_batches(ctx, ds, plist, xy, dist, W, ss):
    from lightcurver_amd.psf_batch import PsfBatch
    from lightcurver_amd.starred.procedures.psf_routines import quadratic_forms
    Fr, S, n = ds['data'].shape[:3]
    star_b = PsfBatch(ds['data'].reshape(Fr * S, 1, n, n), H.weights_from(ds).reshape(Fr * S, 1, n, n), ss, ctx)
    frame_b = PsfBatch(np.zeros((Fr, 1, n, n)), np.zeros((Fr, 1, n, n)), ss, ctx)
    theta = np.concatenate([[[float(p[k]) for k in ('fwhm_x', 'fwhm_y', 'phi', 'beta')] for p in plist], dist], axis=1)
    star_b.set_moffat_q(quadratic_forms(theta, xy, ss).reshape(Fr * S, 4))
    star_b.set_grid(None)
    frame_b.set_grid(None)
    star_b.set_stars(H.stars_array(plist).reshape(Fr * S, 1, 4))
    star_b.set_regularization(None, 0.0, 0.0)
    frame_b.set_grid(np.stack([p['B'].numpy() for p in plist]))
    frame_b.set_regularization(W, 1.0, 1.0)
    frame_b.set_distortion(S, dist, xy)
    return star_b, frame_b


def test_frame_step_with_the_external_gradient_matches_oracle(ctx):
    """One frame_b.step_adabelief(use_ext_grad=True) after a backward against one iteration of oracle.optim.adabelief on
    psf_loss_distorted with B alone free (starlet term with the weights handed to set_regularization).  Tolerances of the
    AdaBelief trajectory test of tests/test_psf_gpu.py at T = 1: the first step is sign-like, so the worst pixel is bounded
    by 2 % of the travel T * lr, the typical pixel agrees to 1e-7 and under 1 % of the pixels are off by more than 1e-6."""
    Fr, S, n, ss, lr = 2, 3, 16, 2, 1e-4
    N = n * ss
    J = om.n_scales(N)
    ds, plist, xy, dist = _problem(Fr, S, n, ss, 41)
    Ws = [om.propagate_noise_psf(plist[f], *H.psf_oracle_inputs(ds, f, ss)[1:], ss) for f in range(Fr)]
    star_b, frame_b = _two_batches(ctx, ds, plist, xy, dist, np.stack([w[:J].numpy() for w in Ws]), ss)
    frame_b.distortion_forward(star_b)
    out = star_b.evaluate()
    frame_b.distortion_backward(star_b)
    frame_b.step_adabelief(use_ext_grad=True, init_learning_rate=lr, schedule_learning_rate=True)
    grid = frame_b.get_grid()
    hist = frame_b.loss_history()
    moved = np.abs(grid - np.stack([p['B'].numpy().reshape(N, N) for p in plist]))
    assert moved.max() > 0.5 * lr
    for f in range(Fr):
        data, sig2, mask = H.psf_oracle_inputs(ds, f, ss)
        fn = lambda q: om.psf_loss_distorted(q, xy[f], data, sig2, mask, ss, W=Ws[f], lam_scales=1.0, lam_hf=1.0)
        pf, lh, l0 = oo.adabelief(fn, plist[f], ['B'], lr, 1, schedule=True)
        total = hist[f, 0] + out['loss'].reshape(Fr, S)[f].sum()
        assert abs(total - l0) / abs(l0) < 1e-4
        dB = np.abs(grid[f].ravel() - pf['B'].numpy())
        print(f'frame step, frame {f}: max |dB| {dB.max():.2e}, median {np.median(dB):.2e}, '
              f'share above 1e-6 {(dB > 1e-6).mean():.4f}')
        assert dB.max() < 0.02 * 1 * lr
        assert np.median(dB) < 1e-7
        assert (dB > 1e-6).mean() < 0.01
    star_b.close()
    frame_b.close()


def test_distortion_run_equals_the_calls_it_replaces(ctx):
    """lc_psf_distortion_run(3) against three rounds of forward / star step with export_grad / backward / frame step with
    use_ext_grad and a final forward: grids, stars and both loss histories bit for bit."""
    Fr, S, n, ss = 2, 3, 16, 2
    N = n * ss
    J = om.n_scales(N)
    ds, plist, xy, dist = _problem(Fr, S, n, ss, 43)
    W = np.random.default_rng(3).uniform(0.5, 1.5, (Fr, J, N, N)) * 1e-3
    cfg = dict(init_learning_rate=1e-4, schedule_learning_rate=True)
    got = []
    for one_call in (True, False):
        star_b, frame_b = _two_batches(ctx, ds, plist, xy, dist, W, ss)
        if one_call:
            frame_b.distortion_run(star_b, 3, **cfg)
        else:
            for _ in range(3):
                frame_b.distortion_forward(star_b)
                star_b.step_adabelief(export_grad=True, **cfg)
                frame_b.distortion_backward(star_b)
                frame_b.step_adabelief(use_ext_grad=True, **cfg)
            frame_b.distortion_forward(star_b)
        assert frame_b.iterations_done == 3 and star_b.iterations_done == 3
        got.append([frame_b.get_grid(), star_b.get_grid(), star_b.get_stars(), frame_b.loss_history(), star_b.loss_history()])
        star_b.close()
        frame_b.close()
    start = np.stack([p['B'].numpy().reshape(N, N) for p in plist]).astype(np.float32)
    assert np.abs(got[0][0] - start).max() > 1e-4 and got[0][2].shape == (Fr * S, 1, 4)
    assert np.abs(got[0][2] - H.stars_array(plist).reshape(Fr * S, 1, 4)).max() > 0
    for a, b in zip(*got):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- lc_apply_distortion ------------------------------------------------------------------------------------------------------
def _asymmetric_psf(N, seed=0):
    """Positive, unit sum, off centre, three times as wide along x as along y, with a ramp along x."""
    rng = np.random.default_rng(seed)
    c = (N - 1) // 2
    v, u = np.meshgrid(np.arange(N) - c, np.arange(N) - c)
    w = max(N / 10.0, 1.0)
    psf = np.exp(-0.5 * ((v - 0.3 * w) / (1.5 * w)) ** 2 - 0.5 * ((u + 0.2 * w) / (0.5 * w)) ** 2) * (1.0 + 0.4 * np.tanh(v / w))
    psf = psf + 0.02 * psf.max() * rng.uniform(0.0, 1.0, (N, N))
    return np.float32(psf / psf.sum())


def _check_apply(got, psf, coef, xy):
    """Every position of one call against oracle.model.apply_distortion; returns the largest error / bound."""
    N = psf.shape[0]
    p64 = psf.astype(np.float64)
    a = D.matrices(coef[None], xy[None])
    a32 = D.matrices(np.float32(coef[None]), np.float32(xy[None]), np.float32)
    worst = 0.0
    for k in range(len(xy)):
        ref = om.apply_distortion(p64, coef, xy[k, 0], xy[k, 1]).numpy()
        op = D.warp_operator(N, a[0][0, k], a[1][0, k], a[2][0, k], flux=False)
        w = op.warp(p64)
        assert np.abs(w / w.sum() - ref).max() <= 1e-12 * ref.max()
        wr = D.position_rounding(N, a32[0][0, k], a32[1][0, k], a32[2][0, k], flux=False, divide=True).warp(p64)
        bound = 4.0 * np.abs(wr / wr.sum() - ref).max() + 8.0 * D.EPS32 * op.warp_abs(p64) / w.sum()
        err = np.abs(got[k] - ref)
        assert np.all(err <= bound), (k, xy[k], float(err.max()), float(bound[np.unravel_index(np.argmax(err), err.shape)]))
        assert abs(float(got[k].astype(np.float64).sum()) - 1.0) < 1e-5
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


@pytest.mark.parametrize('N', [1, 2, 31, 32, 128])
def test_apply_distortion_on_the_matrix_set(ctx, N):
    """The matrix set through lc_apply_distortion (one call per case: the frame's positions with its position-dependent
    coefficients; at N = 128 the first four positions), and K = 300 positions in one call."""
    from lightcurver_amd.starred.psf.psf import apply_distortion
    psf = _asymmetric_psf(N, N)
    assert N < 3 or np.abs(psf - psf.T).max() > 0.1 * psf.max()
    worst = 0.0
    for name, coef, xy in D.CASES:
        pos = xy[:4] if N == 128 else xy
        kw = {'dilation_x': coef[0:3], 'dilation_y': coef[3:6], 'shear': coef[6:9]}
        got = apply_distortion(psf, kw, pos, ctx=ctx)
        assert got.shape == (len(pos), N, N), name
        worst = max(worst, _check_apply(got, psf, coef, pos))
    name, coef, _ = D.CASES[-1]
    xy = np.float32(np.random.default_rng(N).uniform(-0.5, 0.5, (300, 2))).astype(np.float64)
    got = apply_distortion(psf, {'dilation_x': coef[0:3], 'dilation_y': coef[3:6], 'shear': coef[6:9]}, xy, ctx=ctx)
    assert got.shape == (300, N, N)
    worst = max(worst, _check_apply(got, psf, coef, xy))
    print(f'lc_apply_distortion N = {N}: largest error / bound {worst:.3f}')


def test_apply_distortion_pure_dilation_and_pure_shear(ctx):
    """One non-zero coefficient at a time on a PSF that is asymmetric in x and y: a transposed matrix or image cannot pass."""
    from lightcurver_amd.starred.psf.psf import apply_distortion
    N = 32
    psf = _asymmetric_psf(N, 5)
    xy = np.array([[0.25, -0.5]])
    for i in range(9):
        coef = np.zeros(9)
        coef[i] = 0.25
        kw = {'dilation_x': coef[0:3], 'dilation_y': coef[3:6], 'shear': coef[6:9]}
        got = apply_distortion(psf, kw, xy, ctx=ctx)[None]
        _check_apply(got, psf, coef, xy)
        if i in (0, 3):      # what a transposition would give is far outside the bound (a pure shear is its own transpose)
            swapped = om.apply_distortion(psf.T.astype(np.float64), coef, xy[0, 0], xy[0, 1]).numpy().T
            assert np.abs(got[0] - swapped).max() > 1e-3 * got.max()


def test_apply_distortion_keeps_unit_sum_when_flux_leaves_the_grid(ctx):
    """A dilation of 1.5 in both axes pushes a tenth of a broad PSF's flux off the grid: the output is still of unit sum
    and equal to the reference."""
    from lightcurver_amd.starred.psf.psf import apply_distortion
    N = 32
    c = (N - 1) // 2
    v, u = np.meshgrid(np.arange(N) - c, np.arange(N) - c)
    psf = (1.0 + (v * v + 1.3 * u * u + 0.4 * u * v) / 10.0) ** -1.5
    psf = np.float32(psf / psf.sum())
    coef = np.array([0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.0, 0.0, 0.0])
    xy = np.array([[0.5, 0.5]])
    a00, a01, a11, det = D.matrices(coef[None], xy[None])
    assert (a00[0, 0], a01[0, 0], a11[0, 0]) == (1.5, 0.0, 1.5)
    kept = D.warp_operator(N, 1.5, 0.0, 1.5).warp(psf.astype(np.float64)).sum()
    assert 0.88 < kept < 0.92, kept
    got = apply_distortion(psf, {'dilation_x': coef[0:3], 'dilation_y': coef[3:6]}, xy, ctx=ctx)[None]
    _check_apply(got, psf, coef, xy)


def _raw_apply(ctx, N, K, psf, coef, xy, k_arg=None):
    from lightcurver_amd import _lib
    from lightcurver_amd._lib import f32, ptr
    out = np.full((max(K, 1), N, N), SENTINEL, np.float32)
    p, c, q = f32(psf), f32(coef), f32(np.asarray(xy).reshape(-1, 2))
    rc = _lib.lib().lc_apply_distortion(ctx.h, N, K if k_arg is None else k_arg, ptr(p), ptr(c), ptr(q), ptr(out))
    return rc, out, _lib.lib().lc_last_error(ctx.h).decode()


def test_apply_distortion_refusals_leave_the_output_untouched(ctx):
    N = 16
    psf = _asymmetric_psf(N, 2)
    ok = [[0.1, 0.2], [-0.3, 0.4], [0.5, -0.5]]
    zero = np.zeros(9)

    def coef(**kw):
        c = np.zeros(9)
        for k, v in kw.items():
            c[int(k[1:])] = v
        return c

    small = float(np.sqrt(1.0 - 5e-4))                       # det = 1 - shear^2 = 5e-4, inside (0, 1e-3]
    refused = {
        'det in (0, 1e-3]': (coef(c6=small), ok),
        'det < 0': (coef(c0=-2.0), ok),
        'det = 0': (coef(c0=-0.5, c3=-0.5, c6=0.5), ok),
        'singular at the last position only': (coef(c0=-0.25, c1=-0.25, c2=-0.25, c3=-0.25, c4=-0.25, c5=-0.25, c6=0.25,
                                                    c7=0.25, c8=0.25), [[0.0, 0.0], [0.1, 0.1], [0.5, 0.5]]),
        'nan coefficient': (coef(c4=np.nan), ok),
        'inf coefficient': (coef(c8=np.inf), ok),
        'nan position': (zero, [[0.1, 0.2], [np.nan, 0.4], [0.5, -0.5]]),
        'inf position': (coef(c0=0.1), [[0.1, 0.2], [-0.3, 0.4], [0.5, -np.inf]]),
    }
    for what, (c, xy) in refused.items():
        rc, out, msg = _raw_apply(ctx, N, 3, psf, c, xy)
        assert rc == -1 and 'lc_apply_distortion' in msg, (what, rc, msg)
        assert np.all(out == SENTINEL), what
    assert 'position 1 is not finite' in _raw_apply(ctx, N, 3, psf, zero, refused['nan position'][1])[2]
    assert 'position 2' in _raw_apply(ctx, N, 3, psf, *refused['singular at the last position only'])[2]
    for k in (0, -1):
        rc, out, msg = _raw_apply(ctx, N, 3, psf, zero, ok, k_arg=k)
        assert rc == -1 and np.all(out == SENTINEL)
    # just outside the refused range, and after the refusals, the call works
    rc, out, msg = _raw_apply(ctx, N, 3, psf, coef(c6=float(np.sqrt(1.0 - 2e-3))), ok)
    assert rc == 0 and np.all(np.isfinite(out)) and np.all(np.abs(out.sum(axis=(1, 2)) - 1.0) < 1e-5)


# ---- lc_psf_batch_set_distortion: what the kernels do not hold for is refused on the host -----------------------------------
SINGULAR = np.array([-0.25, -0.25, -0.25, -0.25, -0.25, -0.25, 0.25, 0.25, 0.25])     # a00 = a11 = a01 = 0.5 at (0.5, 0.5)


def test_set_distortion_refusals_name_the_star_and_change_nothing(ctx):
    from lightcurver_amd import _lib
    from lightcurver_amd._lib import f32, ptr
    from lightcurver_amd.psf_batch import PsfBatch
    n, ss, S = 16, 1, 4
    N = n * ss
    rng = np.random.default_rng(12)
    star_b = PsfBatch(rng.standard_normal((F * S, 1, n, n)), np.ones((F * S, 1, n, n)), ss, ctx)
    frame_b = PsfBatch(np.zeros((F, 1, n, n)), np.zeros((F, 1, n, n)), ss, ctx)
    lib = _lib.lib()

    def raw(coef, xy):
        c, p = f32(coef).reshape(F, 9), f32(xy).reshape(F, S, 2)
        return lib.lc_psf_batch_set_distortion(frame_b.h, S, ptr(c), ptr(p)), lib.lc_last_error(ctx.h).decode()

    good_coef = np.stack([D.CASES[i][1] for i in (2, -1, 9)])
    good_xy = np.stack([D.CASES[i][2][:S] for i in (2, -1, 9)])
    bad = {}
    c, p = good_coef.copy(), good_xy.copy()
    c[1], p[1, 2] = SINGULAR, (0.5, 0.5)
    bad['singular'] = (c, p, 'singular')
    c, p = good_coef.copy(), good_xy.copy()
    c[1], p[1, 2] = [-0.25, -0.25, -0.2482, -0.25, -0.25, -0.2482, 0.25, 0.25, 0.25], (0.5, 0.5)     # det = 9e-4
    bad['det in (0, 1e-3]'] = (c, p, 'singular')
    p = good_xy.copy()
    p[1, 2] = (40.0, 40.0)
    bad['pixel coordinates'] = (good_coef, p, 'further than 0.5')
    c, p = good_coef.copy(), good_xy.copy()
    c[1], p[1, 2] = [0.25, 0.25, 0.25, 0, 0, 0, 0, 0, 0], (0.5, 0.52)
    bad['entry just past 0.5'] = (c, p, 'further than 0.5')
    for v in (np.nan, np.inf, -np.inf):
        p = good_xy.copy()
        p[1, 2, 1] = v
        bad[f'{v} coordinate'] = (good_coef, p, 'not finite')
    # a batch that was never given a distortion stays without one
    for what, (c, p, word) in bad.items():
        rc, msg = raw(c, p)
        assert rc == -1 and 'frame 1, star 2' in msg and word in msg, (what, rc, msg)
    with pytest.raises(_lib.LcError):
        frame_b.distortion_forward(star_b)
    c = good_coef.copy()
    c[2, 4] = 0.2501
    assert raw(c, good_xy)[0] == -1
    with pytest.raises(_lib.LcError):
        frame_b.distortion_forward(star_b)
    # a batch that has one keeps it: the same resampled grids and the same adjoint, bit for bit, after every refusal
    B = np.stack([D.noise_grid(rng, N) for _ in range(F)])
    star_b.set_moffat_q(np.tile([0.1, 0.02, 0.15, 2.5], (F * S, 1)))
    star_b.set_stars(np.tile([1.0, 0.2, -0.3, 0.0], (F * S, 1, 1)))
    star_b.set_regularization(None, 0.0, 0.0)
    frame_b.set_grid(B)
    frame_b.set_distortion(S, good_coef, good_xy)

    def state():
        frame_b.distortion_forward(star_b)
        fwd = star_b.get_grid()
        star_b.evaluate()
        frame_b.distortion_backward(star_b)
        return fwd, frame_b.get_ext_grad()

    before = state()
    assert np.abs(before[0]).max() > 1 and np.abs(before[1]).max() > 0
    for what, (c, p, word) in bad.items():
        with pytest.raises(_lib.LcError, match='frame 1, star 2'):
            frame_b.set_distortion(S, c, p)
        after = state()
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what
    # the corner itself (entries exactly 0.5 from the identity) is inside
    frame_b.set_distortion(S, np.stack([D.CORNERS[i][1] for i in range(F)]), np.stack([D.CORNERS[i][2][:S] for i in range(F)]))
    star_b.close()
    frame_b.close()


@pytest.mark.parametrize('bad', [(40.0, 40.0), (np.nan, 0.1), (0.2, np.inf), (1.0, -0.6)])
def test_build_psf_refuses_coordinates_that_are_not_rescaled(ctx, bad):
    from lightcurver_amd.starred.procedures.psf_routines import build_psf
    S, n, ss = 4, 16, 2
    rng = np.random.default_rng(3)
    data = rng.standard_normal((S, n, n)) + 50.0 * np.exp(-0.5 * ((np.arange(n) - 7.5) ** 2)[:, None] / 4
                                                           - 0.5 * ((np.arange(n) - 7.5) ** 2)[None, :] / 4)
    xy = rng.uniform(-0.5, 0.5, (S, 2))
    xy[2] = bad
    with pytest.raises(ValueError, match='stamp_coordinates'):
        build_psf(image=data, noisemap=np.ones_like(data), subsampling_factor=ss, masks=np.ones_like(data), n_iter_analytic=5,
                  n_iter_adabelief=5, field_distortion=True, stamp_coordinates=xy)
