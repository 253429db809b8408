"""PSF-fit kernels with stars at offsets up to the quarter-stamp limit (through the C ABI) against the float64 oracle.

The other PSF tests keep their stars within half a data pixel of the stamp centre, where the rounded offset
o = nearbyint(delta) of tap_entry (csrc/psf_kernels.h) only takes the values -1, 0, 1.  build_psf's default barycentre guess
and the bounds of stage A reach +-n/4 data pixels; the window base bq, the zero aprons of the one-wave layout, the
clamped-index reads of the other layouts, the shift / zero-fill of the noise tables and the host noise path all depend on o.
The stamps are drawn from the oracle's own forward model (tests/_psf_geometry.py), the offsets are the corners and edges of
the allowed square, both sides of a rounding tie of delta next to the limit, the same figure at half the limit and a
negative-only frame; fluxes span two decades inside every frame.

Tolerances are those of tests/test_psf_gpu.py (2e-5 loss / model, 5e-5 gradients, 1e-4 Moffat gradient and loss history)
and hold in two finer norms as well: per star (model against the star's own peak, star gradients element by element) and
on the border ring of dL/dB (outer 8 high-resolution pixels against the largest element there), because the global
max-norm hides a faint star next to a bright one and a border that carries 2 % of the largest gradient element.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import model as om, optim as oo
from tests import helpers as H
from tests import _psf_geometry as G

pytestmark = pytest.mark.gpu

# every layout of the PSF kernels at either subsampling: the one-wave layout (N = 16 ... 64) and the block-synchronised one
# (N = 128) at subsampling 2; at subsampling 1 the one-wave layout (n = 16, 32) and the block-synchronised one of n = 64
SIZES = [(16, 1, 8), (16, 2, 8), (24, 2, 8), (32, 2, 8), (64, 2, 8), (32, 1, 8), (64, 1, 8)]


def _batch(ds, plist, ss, ctx, grid=True):
    from lightcurver_amd.psf_batch import PsfBatch
    b = PsfBatch(ds['data'], H.weights_from(ds), ss, ctx)
    b.set_moffat(H.moffat_array(plist))
    b.set_stars(H.stars_array(plist))
    b.set_grid(np.stack([p['B'].numpy() for p in plist]) if grid else None)
    return b


def _oracle_weights(ds, plist, ss):
    return [om.propagate_noise_psf(plist[f], *H.psf_oracle_inputs(ds, f, ss)[1:], ss) for f in range(len(plist))]


def _check_eval(out, f, L, g, model, N, tag, star_element_bounds=(5e-5, 5e-5, 5e-5, 5e-5)):
    """Every figure is printed before it is judged (run with -s to see them).  star_element_bounds: one bound per column
    (a, x0, y0, sky) of the star gradients judged element by element."""
    gs = np.stack([g['a'].numpy(), g['x0'].numpy(), g['y0'].numpy(), g['sky'].numpy()], axis=-1)
    gB = g['B'].numpy().reshape(N, N)
    gm = np.array([float(g[k]) for k in ['fwhm_x', 'fwhm_y', 'phi', 'beta']])
    fig = dict(loss=abs(out['loss'][f] - L) / abs(L), model=H.rel_err(out['model'][f], model),
               stars=[H.rel_err(out['grad_stars'][f][:, q], gs[:, q]) for q in range(4)],
               grid=H.rel_err(out['grad_grid'][f], gB), moffat=H.rel_err(out['grad_moffat'][f], gm),
               model_per_star=G.per_star_model_err(out['model'][f], model).max(),
               stars_per_element=[G.per_element_err(out['grad_stars'][f][:, q], gs[:, q]).max() for q in range(4)],
               ring=G.ring_err(out['grad_grid'][f], gB))
    print(tag, 'frame', f, {k: (['%.2e' % x for x in v] if isinstance(v, list) else '%.2e' % v) for k, v in fig.items()})
    assert fig['loss'] < 2e-5
    assert fig['model'] < 2e-5
    assert max(fig['stars']) < 5e-5, fig['stars']
    assert fig['grid'] < 5e-5
    assert fig['moffat'] < 1e-4
    assert fig['model_per_star'] < 2e-5
    for q in range(4):
        assert fig['stars_per_element'][q] < star_element_bounds[q], (q, fig['stars_per_element'])
    assert fig['ring'] < 5e-5
    return fig


# ---- a. single evaluation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,ss,S', SIZES + [(32, 2, 16)])
def test_eval_at_the_offset_limit_matches_oracle(ctx, n, ss, S):
    """Bounds: 2e-5 / 5e-5 / 1e-4 in every norm, with one exception: dL/da judged element by
    element in frame 1 of the (n, ss) = (64, 2) case gets 6.4e-4.  There a faint star's dL/da sums 4096 pixels of which the noise
    outweighs the 20 % flux deficit; the independent fp32 C port (oracle/psf_cpu.c) is 1.64e-4 from the float64 oracle in
    that element on these very inputs (tests/test_psf_cpu_port_cpu.py runs it on them and guards the figure), and four
    times that is allowed as fp32 reassociation headroom.  dL/dx0, dL/dy0 and dL/dsky of that frame, every column of the
    other frames and every other size keep 5e-5: the C port stays below 1.4e-5 there."""
    F = 3
    N = n * ss
    J = om.n_scales(N)
    ds, plist, xy = G.case(n, ss, S, F, G.eval_seed(n, ss, S))
    Ws = _oracle_weights(ds, plist, ss)
    b = _batch(ds, plist, ss, ctx)
    b.set_regularization(np.stack([w[:J].numpy() for w in Ws]), lam_scales=1.3, lam_hf=0.7)
    out = b.evaluate(model=True)
    free = ['fwhm_x', 'fwhm_y', 'phi', 'beta', 'a', 'x0', 'y0', 'sky', 'B']
    for f in range(F):
        data, sig2, mask = H.psf_oracle_inputs(ds, f, ss)
        fn = lambda q: om.psf_loss(q, data, sig2, mask, ss, W=Ws[f], lam_scales=1.3, lam_hf=0.7)
        L, g = oo.value_and_grad(fn, plist[f], free)
        _check_eval(out, f, L, g, om.psf_model(plist[f], ss, n).numpy(), N, f'eval n={n} ss={ss} S={S}',
                    star_element_bounds=(6.4e-4 if (n, ss, f) == (64, 2, 1) else 5e-5, 5e-5, 5e-5, 5e-5))
    b.close()


# ---- b. noise propagation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,ss,S', SIZES)
def test_noise_propagation_at_the_offset_limit_matches_oracle(ctx, n, ss, S):
    """Device tables (csrc/psf_noise.h: the response enters shifted by ss * (n / 2) - c with zero fill, which cuts it at
    large offsets) and the host path (LCMI_NOISE_HOST=1), each against the oracle's direct formula; the finest scale also on
    its border ring, where the cut response of a star at the limit lands."""
    F = 3 if n < 64 else 2
    J = om.n_scales(n * ss)
    ds, plist, xy = G.case(n, ss, S, F, 400 + n + ss)
    b = _batch(ds, plist, ss, ctx)
    Wo = np.stack([w[:J].numpy() for w in _oracle_weights(ds, plist, ss)])
    for env in (None, '1'):
        if env:
            os.environ['LCMI_NOISE_HOST'] = env
        try:
            b.propagate_noise()
        finally:
            os.environ.pop('LCMI_NOISE_HOST', None)
        W = b.get_weights()
        for f in range(F):
            e, r = H.rel_err(W[f], Wo[f]), G.ring_err(W[f][0], Wo[f][0])
            print(f'noise n={n} ss={ss} host={env} frame {f}: all scales {e:.2e} finest-scale ring {r:.2e}')
            assert e < 2e-5
            assert r < 2e-5
    b.close()


# ---- c. AdaBelief trajectory -----------------------------------------------------------------------------------------------
def _trajectory_problem(n, ss, seed, gap=6e-4):
    """Two frames of 8 stars for a run of the optimiser: the limit set and the half-limit set of G.offset_frames.  The
    stars of the limit set start 0.01 data pixels inside +-n/4: a run moves a position by a few 1e-3 pixels, and a star
    that leaves the allowed square is pinned by the kernel where the oracle, which knows no limit,
    goes on - the pin has its own test below.  In frame 1, star 0 - given the brightest flux of its frame - starts `gap`
    pixels inside the last rounding tie of delta in x while its stamp has the star 0.3 pixels past the tie: AdaBelief's
    first steps move a parameter by about the learning rate (1e-4) each, so x0 passes the tie within the first ten
    iterations and o, bq and the tap table change between two iterations."""
    lim = n / 4.0
    xy = np.clip(G.offsets_for(n, ss, 8, 2), -(lim - 0.01), lim - 0.01)
    t = G.tie_offset(n, ss)
    xy[1, 0] = (t - gap, 0.31)
    true = G.displaced(xy, seed + 1)
    true[1, 0, 0] = t + 0.3
    ds = G.draw_dataset(n, ss, true, seed, brightest={1: 0})
    return ds, G.params_at(ds, xy, seed + 2), t


@pytest.mark.parametrize('n,ss', [(16, 2), (32, 2), (64, 2), (32, 1), (64, 1)])
def test_adabelief_trajectory_from_the_offset_limit_matches_oracle(ctx, n, ss):
    """T = 25 iterations started at the limit offsets, with the bounds of test_psf_gpu.py's trajectory test.  In frame 1 a
    star crosses a rounding tie of delta during the run (see _trajectory_problem): the crossing is asserted on the ORACLE's
    x0 history, so the test cannot stop exercising the rebuilt tap table without failing."""
    F, T, S = 2, 25, 8
    N = n * ss
    J = om.n_scales(N)
    ds, plist, tie = _trajectory_problem(n, ss, 500 + n)
    Ws = _oracle_weights(ds, plist, ss)
    b = _batch(ds, plist, ss, ctx)
    b.set_regularization(np.stack([w[:J].numpy() for w in Ws]), lam_scales=1.0, lam_hf=1.0)
    b.run_adabelief(T, init_learning_rate=1e-4, schedule_learning_rate=True)
    hist, stars, grid = b.loss_history(), b.get_stars(), b.get_grid()
    assert hist.shape == (F, T + 1)
    for f in range(F):
        data, sig2, mask = H.psf_oracle_inputs(ds, f, ss)
        x0_hist = []

        def fn(q):
            x0_hist.append(float(q['x0'][0].detach()))
            return om.psf_loss(q, data, sig2, mask, ss, W=Ws[f], lam_scales=1.0, lam_hf=1.0)
        pf, lh, l0 = oo.adabelief(fn, plist[f], ['B', 'a', 'x0', 'y0'], 1e-4, T, schedule=True)
        if f == 1:
            x0h = np.array(x0_hist[:T + 1])      # x0 of the crossing star at every evaluation of the run
            side = x0h > tie
            print(f'crossing n={n}: tie {tie}, x0 - tie from {x0h[0] - tie:.2e} to {x0h[-1] - tie:.2e}, '
                  f'{int((~side).sum())} evaluations before, {int(side.sum())} after')
            assert not side[0] and side[-1] and 2 <= side.sum() <= T - 1   # both sides are evaluated at least twice
        ref = np.array([l0] + lh)
        dB = np.abs(grid[f].ravel() - pf['B'].numpy())
        fig = dict(hist=np.abs(hist[f] - ref).max() / np.abs(ref).max(), dBmax=dB.max(), dBmed=np.median(dB),
                   moved=(dB > 1e-6).mean(), a=H.rel_err(stars[f][:, 0], pf['a'].numpy()),
                   x0=np.abs(stars[f][:, 1] - pf['x0'].numpy()).max(), y0=np.abs(stars[f][:, 2] - pf['y0'].numpy()).max())
        print(f'trajectory n={n} frame {f}', {k: '%.2e' % v for k, v in fig.items()})
        assert fig['hist'] < 1e-4
        assert fig['dBmax'] < 0.02 * T * 1e-4 and fig['dBmed'] < 1e-7 and fig['moved'] < 0.01
        assert fig['a'] < 1e-5
        assert fig['x0'] < 2e-5 and fig['y0'] < 2e-5
    b.close()


# ---- d. the forms of the optimisation loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n,F', [(32, 100), (64, 63)])
def test_forms_are_bit_identical_at_the_offset_limit(ctx, n, F):
    """The two-workgroup form (same-XCD hand-off and write-through hand-off) and the one-workgroup form, as
    test_psf_gpu.py::test_two_workgroup_form_is_bit_identical, on the offset set: three frames of G.offset_frames and the
    frame with the tie-crossing star, repeated to F frames (the forms rebuild the tap tables at different places of the
    iteration - behind role 0's hand-off stores or behind the star update).  That the star does cross is read off the
    result."""
    ss, S, T = 2, 8, (60 if n < 64 else 20)
    ds2, pl2, tie = _trajectory_problem(n, ss, 600 + n, gap=3e-4)
    ds3, pl3, _ = G.case(n, ss, S, 3, 610 + n)
    reps = (F + 3) // 4
    pick = lambda a3, a2: np.concatenate([np.concatenate([a3, a2[1:2]])] * reps)[:F]
    ds = dict(data=pick(ds3['data'], ds2['data']), noisemap=pick(ds3['noisemap'], ds2['noisemap']),
              masks=pick(ds3['masks'], ds2['masks']), ss=ss)
    plist = ((pl3 + [pl2[1]]) * reps)[:F]
    out = []
    for env in ({}, {'LCMI_PSF_XCD_FAST': '0'}, {'LCMI_PSF_SINGLE_WG': '1'}):
        os.environ.update(env)
        try:
            b = _batch(ds, plist, ss, ctx)
            b.propagate_noise()
            b.set_regularization(None, 1.0, 1.0)
            b.run_adabelief(T, init_learning_rate=1e-4, schedule_learning_rate=True)
            b.run_adabelief(T // 2, init_learning_rate=1e-4, schedule_learning_rate=True)
            out.append((b.loss_history(), b.get_grid(), b.get_stars()))
            b.close()
        finally:
            for k in env:
                os.environ.pop(k, None)
    for other in out[1:]:
        for a, c in zip(out[0], other):
            np.testing.assert_array_equal(a, c)
    assert np.all(np.isfinite(out[0][0]))
    x_start, x_end = float(plist[3]['x0'][0]), out[0][2][3, 0, 1]
    print(f'forms n={n}: crossing star x0 - tie from {x_start - tie:.2e} to {x_end - tie:.2e}')
    assert x_start < tie < x_end


# ---- e. past the limit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,ss,S', SIZES)
def test_past_the_limit_is_pinned_to_the_limit(ctx, n, ss, S):
    """A star parameter past +-n/4 (a broken fit) is pinned there: DESIGN.md section 3.  With x0, y0 = +-(n/4 + 1.5) the
    evaluation returns model, loss and dL/dB bit-equal to those at +-n/4, the noise maps of both paths are bit-equal too
    (they pin in the same way), and ten AdaBelief iterations stay finite.

    Why nothing reads or writes outside its buffers, whatever the star parameters hold (from the code, csrc/psf_kernels.h):
    * compute_taps clamps ss * x0 to [-N/4, N/4] with fminf / fmaxf before anything is derived from it (a NaN comes out of
      fmaxf / fminf as the bound), so |o| <= N/4 (N/4 is even at every size, N/4 + 0.5 rounds to N/4) and
      bq = floor((o - kRg - (SS - 1)) / SS) lies in [-(N/4 + 6) / SS, (N/4 - 6) / SS] for SS = 2, [-N/4 - 5, N/4 - 5] for
      SS = 1.  Every window index below is an affine function of bq and of a tile index with compile-time range.
    * One-wave layout (N = 16 .. 64).  Row pass: the window of T starts at ws = SS * (jd0 - bq) - (NT - 1) with
      jd0 in [0, n - JB] and is SS * (JB - 1) + NT (+ 1, paired form) samples long: at N = 64 that is [-22, 85] around a row
      of 64 samples with aprons AP = N/4 + 10 = 26 on either side ([-26, 89]); the bounds scale with N/4 like AP does.
      Column pass: same expression with a0 in [0, n - LC] on the R2 rows of the per-wave scratch, same apron.  Transposed
      column pass: residual rows bq + a0 + i, i < WI = 10, i.e. [-11, 42] at N = 64 inside [-APR, n - 1 + APR] = [-15, 46].
      Transposed row pass: reads V through min(max(jd, -1), n) into the two zero columns.  The aprons are LDS of the same
      workgroup, zeroed once and never written.
    * Other layout (N = 128): every window sample is read through min(max(idx, 0), N - 1) (or n - 1) and replaced by zero
      when idx was outside; all stores go to tile indices that do not depend on bq.
    * Noise tables (csrc/psf_noise.h): delta only enters comparisons and the exponent; every index is threadIdx / loop
      bound.  Host path: pinned with fmin / fmax in the same way, and up, vp are range-checked before r is written.
    The test does not try to leave the buffers; it checks the pin that this argument rests on."""
    lim, F = n / 4.0, 2
    N = n * ss
    ds, plist, xy = G.case(n, ss, S, F, 700 + n + ss)
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    # frame 0: x0 past the limit (alternating sign), y0 inside; frame 1: both past it, opposite signs
    past = np.stack([np.stack([sign * (lim + 1.5), xy[0, :, 1]], axis=-1),
                     np.stack([sign * (lim + 1.5), -sign * (lim + 1.5)], axis=-1)])
    at = np.clip(past, -lim, lim)
    res = []
    for pos in (at, past):
        pl = [dict(p, x0=om.T(pos[f, :, 0]), y0=om.T(pos[f, :, 1])) for f, p in enumerate(plist)]
        b = _batch(ds, pl, ss, ctx)
        b.propagate_noise()
        Wd = b.get_weights().copy()
        os.environ['LCMI_NOISE_HOST'] = '1'
        try:
            b.propagate_noise()
        finally:
            os.environ.pop('LCMI_NOISE_HOST', None)
        Wh = b.get_weights().copy()
        b.set_regularization(None, 1.3, 0.7)
        out = b.evaluate(model=True)
        ev = {k: np.array(out[k]) for k in ('model', 'loss', 'grad_grid')}
        b.run_adabelief(10, init_learning_rate=1e-4, schedule_learning_rate=True)
        res.append((ev, Wd, Wh, b.loss_history(), b.get_grid(), b.get_stars()))
        b.close()
    (ev0, Wd0, Wh0, *_), (ev1, Wd1, Wh1, hist, grid, stars) = res
    for k in ('model', 'loss', 'grad_grid'):
        np.testing.assert_array_equal(ev0[k], ev1[k], err_msg=k)
    assert np.all(np.isfinite(ev1['loss'])) and np.all(ev1['loss'] > 0)
    np.testing.assert_array_equal(Wd0, Wd1)
    np.testing.assert_array_equal(Wh0, Wh1)
    assert np.all(np.isfinite(Wd1)) and np.all(np.isfinite(Wh1)) and Wd1.max() > 0 and Wh1.max() > 0
    assert H.rel_err(Wd1, Wh1) < 2e-5
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(grid)) and np.all(np.isfinite(stars))


# ---- f. stage A and build_psf at real offsets ------------------------------------------------------------------------------
def _real_offset_stamps(n, ss, S, seed):
    """One frame of S stars at true offsets up to 0.8 * n/4 (the corners of that square among them), drawn from the oracle's
    forward model; flux over one decade so that every star constrains its position."""
    rng = np.random.default_rng(seed)
    r = 0.8 * n / 4.0
    xy = rng.uniform(-r, r, (1, S, 2))
    xy[0, :4] = [(r, r), (-r, r), (r, -r), (-r, -r)]
    return G.draw_dataset(n, ss, xy, seed + 1, flux_decades=1.0), xy


def _stage_a_optimum(ds, ss, n, S, x0, y0):
    """scipy L-BFGS-B on the oracle loss from the clipped barycentre guess, as test_moffat_stage_reaches_oracle_optimum."""
    data, sig2, mask = H.psf_oracle_inputs(ds, 0, ss)
    a = (ds['data'][0] * ds['masks'][0]).sum(axis=(-1, -2)).astype(np.float64)
    p0 = {k: om.T(v) for k, v in dict(fwhm_x=3.0, fwhm_y=3.0, phi=0.0, beta=2.5, B=np.zeros(n * ss * n * ss), a=a, x0=x0,
                                      y0=y0, sky=np.zeros(S)).items()}
    free = ['fwhm_x', 'fwhm_y', 'phi', 'beta', 'a', 'x0', 'y0']
    bounds = dict(fwhm_x=(0.5 / ss, n / 2), fwhm_y=(0.5 / ss, n / 2), phi=(-math.pi, math.pi), beta=(1.1, 50.),
                  a=(0, np.inf), x0=(-n / 4, n / 4), y0=(-n / 4, n / 4))
    po, hist, res = oo.lbfgsb(lambda q: om.psf_loss(q, data, sig2, mask, ss), p0, free, 200, bounds)
    return p0, po, res


def test_moffat_stage_and_build_psf_at_real_offsets(ctx):
    """Stage A from the clipped barycentre guess on stamps whose stars sit up to 0.8 * n/4 from the centre: fit_moffat(200)
    against scipy L-BFGS-B on the oracle loss (tolerances of test_psf_gpu.py::test_moffat_stage_reaches_oracle_optimum), then
    build_psf(guess_method_star_position='barycenter') end to end on the same stamps: reduced chi2 < 1.5 (the bound
    test_distortion_gpu.py uses for model-drawn data) and x0, y0 within the stage-A tolerance of the scipy optimum."""
    from lightcurver_amd.starred.procedures.psf_routines import build_psf, _initial_positions
    n, ss, S = 16, 2, 8
    ds, xy = _real_offset_stamps(n, ss, S, 801)
    x0, y0 = _initial_positions(ds['data'][0].astype(np.float64), ds['masks'][0], 'barycenter')
    print('barycentre guess - truth', np.abs(x0 - xy[0, :, 0]).max(), np.abs(y0 - xy[0, :, 1]).max())
    p0, po, res = _stage_a_optimum(ds, ss, n, S, x0, y0)
    b = _batch(ds, [p0], ss, ctx, grid=False)
    final = b.fit_moffat(200)
    mof, st = b.get_moffat(), b.get_stars()
    b.close()
    print('stage A', final[0], res.fun, np.abs(st[0][:, 1] - po['x0'].numpy()).max(), np.abs(st[0][:, 2] - po['y0'].numpy()).max())
    assert final[0] <= res.fun * (1 + 2e-4) + 1e-6, (final[0], res.fun)
    assert abs(final[0] - res.fun) / res.fun < 2e-3
    assert H.rel_err(st[0][:, 0], po['a'].numpy()) < 5e-3
    assert np.abs(st[0][:, 1] - po['x0'].numpy()).max() < 5e-3
    assert np.abs(st[0][:, 2] - po['y0'].numpy()).max() < 5e-3
    fw_gpu, fw_or = 0.5 * (mof[0, 0] + mof[0, 1]), 0.5 * (float(po['fwhm_x']) + float(po['fwhm_y']))
    assert abs(fw_gpu - fw_or) / fw_or < 2e-2
    r = build_psf(image=ds['data'][0].astype(np.float64), noisemap=ds['noisemap'][0].astype(np.float64),
                  subsampling_factor=ss, masks=ds['masks'][0].astype(np.float64), n_iter_analytic=200, n_iter_adabelief=300,
                  guess_method_star_position='barycenter', guess_fwhm_pixels=3.5)
    kg = r['kwargs_psf']['kwargs_gaussian']
    print('build_psf chi2', r['chi2'], np.abs(kg['x0'] - po['x0'].numpy()).max(), np.abs(kg['y0'] - po['y0'].numpy()).max())
    assert r['chi2'] < 1.5
    assert np.abs(kg['x0'] - po['x0'].numpy()).max() < 5e-3
    assert np.abs(kg['y0'] - po['y0'].numpy()).max() < 5e-3


def test_build_psf_embedded_size_at_real_offsets(ctx):
    """20 x 20 stamps have no kernel of their own and are fitted embedded in 24 x 24 frames; the barycentre guess and the
    stars' offsets (up to 0.8 * 20/4 = 4 data pixels) are in the caller's frame.  Reduced chi2 < 1.5 as above; positions
    against the truth the stamps were drawn from: the faintest star has 1e4 counts over a noise floor of 5 per pixel, a
    centroid error of FWHM / (2.355 * SNR) < 0.02 pixels, so 0.1 pixels is more than five sigma for every star."""
    from lightcurver_amd.starred.procedures.psf_routines import build_psf
    n, ss, S = 20, 2, 8
    ds, xy = _real_offset_stamps(n, ss, S, 811)
    r = build_psf(image=ds['data'][0].astype(np.float64), noisemap=ds['noisemap'][0].astype(np.float64),
                  subsampling_factor=ss, masks=ds['masks'][0].astype(np.float64), n_iter_analytic=200, n_iter_adabelief=300,
                  guess_method_star_position='barycenter', guess_fwhm_pixels=3.5)
    kg = r['kwargs_psf']['kwargs_gaussian']
    print('embedded build_psf chi2', r['chi2'], np.abs(kg['x0'] - xy[0, :, 0]).max(), np.abs(kg['y0'] - xy[0, :, 1]).max())
    assert r['residuals'].shape == (S, n, n) and r['narrow_psf'].shape == (n * ss, n * ss)
    assert r['chi2'] < 1.5
    assert np.abs(kg['x0'] - xy[0, :, 0]).max() < 0.1 and np.abs(kg['y0'] - xy[0, :, 1]).max() < 0.1


# ---- Moffat parameters away from the one starting point of the parity tests -----------------------------------------------
MOFFATS = {'beta1.2': (3.0, 2.7, 0.3, 1.2), 'beta8': (3.0, 2.7, 0.3, 8.0), 'beta40': (3.0, 2.7, 0.3, 40.0),
           'ratio0.4': (4.0, 1.6, 0.3, 2.5), 'phi-3.1': (3.0, 2.4, -3.1, 2.5), 'phi_pi/2': (3.0, 2.4, math.pi / 2, 2.5),
           'phi3.1': (3.0, 2.4, 3.1, 2.5), 'fwhm_min': (None, None, 0.3, 2.5)}


@pytest.mark.parametrize('which', list(MOFFATS))
@pytest.mark.parametrize('n,ss', [(16, 2), (32, 2), (32, 1), (64, 1)])
def test_moffat_gradient_away_from_the_starting_point(ctx, n, ss, which):
    """grad_moffat (and the rasterised Moffat behind loss and model) at beta 1.2 / 8 / 40, axis ratio 0.4, phi next to +-pi
    and at pi/2, and fwhm at 1.2 x its lower bound 0.5 / ss, against the oracle with the tolerances of test_eval_matches_oracle;
    the other parity tests evaluate it at (phi 0.3, beta 2.5) only.  Stars at the half-limit set."""
    N = n * ss
    J = om.n_scales(N)
    m = MOFFATS[which]
    if m[0] is None:
        m = (1.2 * 0.5 / ss, 1.2 * 0.5 / ss * 1.1, m[2], m[3])
    xy = G.offsets_for(n, ss, 8, 2)[1:2]
    ds = G.draw_dataset(n, ss, xy, 900 + n)
    plist = G.params_at(ds, xy, 901 + n, moffat=np.array(m, dtype=np.float32).astype(np.float64))
    Ws = _oracle_weights(ds, plist, ss)
    b = _batch(ds, plist, ss, ctx)
    b.set_regularization(np.stack([w[:J].numpy() for w in Ws]), lam_scales=1.3, lam_hf=0.7)
    out = b.evaluate(model=True)
    b.close()
    data, sig2, mask = H.psf_oracle_inputs(ds, 0, ss)
    fn = lambda q: om.psf_loss(q, data, sig2, mask, ss, W=Ws[0], lam_scales=1.3, lam_hf=0.7)
    free = ['fwhm_x', 'fwhm_y', 'phi', 'beta', 'a', 'x0', 'y0', 'sky', 'B']
    L, g = oo.value_and_grad(fn, plist[0], free)
    gm = np.array([float(g[k]) for k in free[:4]])
    # the same evaluation by the oracle in float32: what rounding alone does to this gradient (printed for DESIGN.md)
    p32 = {k: om.T(v, dtype=torch.float32) for k, v in plist[0].items()}
    fn32 = lambda q: om.psf_loss(q, om.T(data, torch.float32), om.T(sig2, torch.float32), om.T(mask, torch.float32), ss,
                                 W=om.T(Ws[0], torch.float32), lam_scales=1.3, lam_hf=0.7)
    L32, g32 = oo.value_and_grad(fn32, p32, free[:4])
    e32 = H.rel_err(np.array([float(g32[k]) for k in free[:4]]), gm)
    e = H.rel_err(out['grad_moffat'][0], gm)
    print(f'moffat {which} n={n}: grad_moffat {e:.2e} (float32 oracle {e32:.2e}) loss {abs(out["loss"][0] - L) / abs(L):.2e} '
          f'model {H.rel_err(out["model"][0], om.psf_model(plist[0], ss, n).numpy()):.2e}', gm, out['grad_moffat'][0])
    assert abs(out['loss'][0] - L) / abs(L) < 2e-5
    assert H.rel_err(out['model'][0], om.psf_model(plist[0], ss, n).numpy()) < 2e-5
    assert H.rel_err(out['grad_grid'][0], g['B'].numpy().reshape(N, N)) < 5e-5
    assert e < 1e-4
