"""Every term of the joint loss on its own, on every device path that has it, at the active points of tests/_joint_terms.py
(tests/test_joint_terms_cpu.py proves on the oracle that each term carries at least a tenth of its block's gradient there
and moves every loop's trajectory by ten tolerances).

Evaluations - the method of test_flux_uniformity_with_small_scatter: the same object at the same parameters with the term's
strength on and off (two evaluations with it off are bit-equal), the differences against the float64 oracle's:

    |dg_dev - dg_ref| <= r   * max|dg_ref| + 8 * 2^-24 * max|g_dev_off|     per block, r   = 1e-4
    |dL_dev - dL_ref| <= r_L * |dL_ref|    + 4 * 2^-24 * |L_dev_off|               r_L = 3e-5

(second summands: the float32 rounding of adding the term to the rest), and the control: the device's difference for a term
is NOT within that bound of the oracle's difference for any other term of the same block (a swap of the two l1 strengths or
of the two prior coordinates).  Loops - T = 20 AdaBelief iterations with the term alone beside chi2 against oo.adabelief on
the same loss, at the tolerances of test_adabelief_trajectory."""
import numpy as np
import pytest

from tests import _joint_terms as JT
from tests import helpers as H

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
CFG = dict(init_learning_rate=JT.LR_LOOP, schedule_learning_rate=True)


def _fit(ctx, pt, free):
    from lightcurver_amd.joint import JointFit
    ds = pt['ds']
    j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], pt['ss'], pt['M'], ctx)
    j.set_params(**pt['p'])
    j.set_free(list(free))
    return j


def _evaluate(j, pt, on, free, how):
    j.set_loss(**JT.settings(pt, on)[0])
    if how == 'step':
        j.step_local()
        L, g = j.step_grad(free)
    else:
        L, g = j.loss_grad(free)
    return float(L), {k: np.asarray(v, np.float64) for k, v in g.items()}


def _check_terms(j, pt, case, base, terms, free, how='loss_grad'):
    L1, g1 = _evaluate(j, pt, base, free, how)
    refs = {t: JT.oracle_term(pt, t, free, base=base) for t in terms}
    seen = {}
    for t in terms:
        off = tuple(u for u in base if u != t)
        L0, g0 = _evaluate(j, pt, off, free, how)
        L0b, g0b = _evaluate(j, pt, off, free, how)
        assert L0 == L0b and all(np.array_equal(g0[b], g0b[b]) for b in free), t
        dL, dg = L1 - L0, {b: g1[b] - g0[b] for b in free}
        seen[t] = (dg, {b: 8 * EPS * np.abs(g0[b]).max() for b in free})
        dL_ref, dg_ref = refs[t]
        tol_L = JT.r_loss(t, case) * abs(dL_ref) + 4 * EPS * abs(L0)
        print(f'{case} {how} {t}: value off by {abs(dL - dL_ref):.2e} of {abs(dL_ref):.2e} (bound {tol_L:.2e})')
        bad = []
        if not abs(dL - dL_ref) <= tol_L:
            bad.append((t, 'value', abs(dL - dL_ref), tol_L))
        for b in free:
            err, scale = np.abs(dg[b] - dg_ref[b]).max(), np.abs(dg_ref[b]).max()
            tol = JT.r_grad(t, case) * scale + seen[t][1][b]
            if b in JT.BLOCKS[t]:
                print(f'{case} {how} {t} {b}: off by {err:.2e} = {err / scale:.1e} of the term (bound {tol:.2e}, floor {seen[t][1][b]:.1e})')
            if not err <= tol:
                bad.append((t, b, err, tol))
        assert not bad, bad
    for t in terms:                       # the control: no other term's difference would have passed in this one's place
        for u in terms:
            for b in set(JT.BLOCKS[t]) & set(JT.BLOCKS[u]):
                if u != t:
                    ref_u = refs[u][1][b]
                    tol = JT.r_grad(u, case) * np.abs(ref_u).max() + seen[t][1][b]
                    assert np.abs(seen[t][0][b] - ref_u).max() > tol, (t, u, b)


@pytest.mark.parametrize('case', JT.CASES_ONE_WG, ids=str)
def test_one_workgroup_update(ctx, case, monkeypatch):
    monkeypatch.delenv('LCMI_N128_SPLIT', raising=False)
    pt = JT.point_of(case)
    j = _fit(ctx, pt, JT.FREE_H)
    try:
        _check_terms(j, pt, case, JT.ALL, JT.ALL, JT.FREE_H)
    finally:
        j.close()


@pytest.mark.parametrize('case,forced', [(JT.CASE_MULTI_BLOCK, False), (JT.CASE_N128, False)] + [(c, True) for c in JT.CASES_FORCED_GLOBAL] +
                         [(c, False) for c in JT.CASES_MULTI_BLOCK_SS1 + [JT.CASE_N128_SS1]], ids=str)
def test_multi_block_update(ctx, case, forced):
    """n = 40 and 64 take the multi-block update by themselves (through loss_grad the regulariser comes from the
    multi-block cascade kernels at n = 40 and from the matrix-core chain at N = 128); n = 16 and 32 under
    lc_joint_set_debug_global.  At subsampling 1: n = 24, 40, 56 (run-time-N regulariser and update behind the epoch kernel
    with 8-lane transforms) and n = 128 (the chain)."""
    from lightcurver_amd import _lib
    lib = _lib.lib()
    pt = JT.point_of(case)
    if forced:
        lib.lc_joint_set_debug_global(1)
    try:
        j = _fit(ctx, pt, JT.FREE_H)
        try:
            _check_terms(j, pt, case, JT.ALL, JT.ALL, JT.FREE_H)
        finally:
            j.close()
    finally:
        if forced:
            lib.lc_joint_set_debug_global(0)


CHAIN_ENVS = dict(argvalues=[{}, {'LCMI_REG_FUSED': '0'}, {'LCMI_REG_CASCADE': '1'}], ids=['default', 'eight-launch', 'cascade'])
CHAIN_BASES = dict(argvalues=[JT.ALL, ('pos', 'pts')], ids=['all-terms', 'no-l1'])


@pytest.mark.parametrize('base', **CHAIN_BASES)
@pytest.mark.parametrize('env', **CHAIN_ENVS)
def test_large_grid_regulariser_chains(ctx, monkeypatch, env, base):
    """N = 128: the regulariser through the four-launch matrix-core chain, the eight-launch one, the cascade; with both l1
    strengths zero the eight-launch form is the production path.  Evaluated as an iteration does it: step_local (the chain
    on the second stream) + step_grad."""
    _check_chains(ctx, monkeypatch, env, base, JT.CASE_N128)


@pytest.mark.parametrize('base', **CHAIN_BASES)
@pytest.mark.parametrize('env', **CHAIN_ENVS)
def test_large_grid_regulariser_chains_at_subsampling_1(ctx, monkeypatch, env, base):
    """The same chains behind the N = 128 epoch kernel of subsampling 1 (n = 128)."""
    _check_chains(ctx, monkeypatch, env, base, JT.CASE_N128_SS1)


def _check_chains(ctx, monkeypatch, env, base, case):
    for k in ('LCMI_REG_FUSED', 'LCMI_REG_CASCADE', 'LCMI_REG_DENSE', 'LCMI_PTS_TAIL', 'LCMI_PTS_CHAIN'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pt = JT.point_of(case)
    terms = tuple(t for t in JT.N128_TERMS if t in base)
    j = _fit(ctx, pt, JT.FREE_H)
    try:
        _check_terms(j, pt, case, base, terms, JT.FREE_H, how='step')
    finally:
        j.close()


@pytest.mark.parametrize('fft_only', [False, True], ids=['separable', 'fft-only'])
@pytest.mark.parametrize('case', JT.CASES_PS, ids=str)
def test_point_source_only_kernel(ctx, monkeypatch, case, fft_only):
    """h zero and fixed: csrc/joint_ps.h, and the library's FFT pipeline on the same problem (LCMI_JOINT_FFT_ONLY=1)."""
    if fft_only:
        monkeypatch.setenv('LCMI_JOINT_FFT_ONLY', '1')
    else:
        monkeypatch.delenv('LCMI_JOINT_FFT_ONLY', raising=False)
    pt = JT.point_of(case, False)
    j = _fit(ctx, pt, JT.FREE_PS)
    try:
        _check_terms(j, pt, case, JT.PS_TERMS, JT.PS_TERMS, JT.FREE_PS)
    finally:
        j.close()


@pytest.mark.parametrize('case', JT.CASES_STEP, ids=str)
def test_step_entry_points_on_one_rank(ctx, case):
    """step_local + step_grad (the sharded fit's evaluation; one rank, nothing to all-reduce): every term as above."""
    pt = JT.point_of(case)
    j = _fit(ctx, pt, JT.FREE_H)
    try:
        _check_terms(j, pt, case, JT.ALL, JT.ALL, JT.FREE_H, how='step')
    finally:
        j.close()


@pytest.mark.parametrize('case', JT.CASES_STEP, ids=str)
def test_step_grad_equals_loss_grad_within_the_rounding_floor(ctx, case):
    """All terms on: step_local + step_grad against loss_grad of the same object, within 4 * 2^-24 of the loss and
    8 * 2^-24 of each block's largest gradient element.

    At (2, 2, 64, 2, 0.3) this test found loss_grad and an iteration evaluating the regulariser of h with different kernels
    (the multi-block cascade inline against the matrix-core chain): one pixel of dL/dh 8.13 units of 2^-24 of the largest
    element apart.  lc_joint_loss_grad takes the chain there now, as an iteration does."""
    pt = JT.point_of(case)
    j = _fit(ctx, pt, JT.FREE_H)
    try:
        L1, g1 = _evaluate(j, pt, JT.ALL, JT.FREE_H, 'loss_grad')
        L2, g2 = _evaluate(j, pt, JT.ALL, JT.FREE_H, 'step')
        print(f'{case} step_grad against loss_grad, in units of 2^-24: value {abs(L2 - L1) / abs(L1) / EPS:.2f}',
              {b: f'{H.rel_err(g2[b], g1[b]) / EPS:.2f}' for b in JT.FREE_H})
        assert abs(L2 - L1) <= 4 * EPS * abs(L1)
        for b in JT.FREE_H:
            assert np.abs(g2[b] - g1[b]).max() <= 8 * EPS * np.abs(g1[b]).max(), b
    finally:
        j.close()


# ------------------------------------------------------------------------------------------------------------------ loops
def _run(ctx, pt, on, free, T=JT.T_LOOP):
    j = _fit(ctx, pt, free)
    try:
        j.set_loss(**JT.settings(pt, on)[0])
        j.run_adabelief(T, **CFG)
        return np.asarray(j.loss_history(), np.float64), {k: np.asarray(v) for k, v in j.get_params().items()}
    finally:
        j.close()


def _against_the_oracle(label, got, ref, free, T=JT.T_LOOP):
    (hist, p), (rh, rp) = got, ref
    assert hist.shape == (T + 1,)
    d = JT.trajectory_distance(ref, (hist, {k: np.asarray(v, np.float64) for k, v in p.items()}), free)
    print(label, {k: f'{v:.2f}' for k, v in d.items()}, '(1 = the bound)')
    assert np.abs(hist - rh).max() / np.abs(rh).max() < 2e-4
    assert H.rel_err(p['a'], rp['a']) < 2e-4
    for k in ('c_x', 'c_y', 'dx', 'dy'):
        if k in free:
            assert np.abs(p[k] - rp[k]).max() < 5e-4, k
    if 'h' in free:
        dh = np.abs(p['h'] - rp['h'])
        assert dh.max() < 0.05 * T * JT.LR_LOOP and np.median(dh) < 1e-5


@pytest.mark.parametrize('term', JT.ALL)
@pytest.mark.parametrize('case', [c for c, _ in JT.LOOP_SECOND_STREAM], ids=str)
def test_loop_with_second_stream_regulariser(ctx, case, term):
    """n = 16, 32 (and n = 32, 48 at subsampling 1): inside lc_joint_run_adabelief the regulariser and the point-source term
    run on the second stream ahead of the single-workgroup update (reg_mode 1 / 2, pts_early)."""
    pt = JT.point_of(case)
    got = _run(ctx, pt, (term,), JT.FREE_H)
    _against_the_oracle(f'{case} {term}', got, JT.oracle_trajectory(pt, (term,), JT.FREE_H), JT.FREE_H)


@pytest.mark.parametrize('case,term', [(c, t) for c, terms in JT.LOOP_FUSED for t in terms], ids=str)
def test_loop_with_fused_reduction_and_update(ctx, monkeypatch, case, term):
    """n = 40, 64 (and n = 24, 40, 56 at subsampling 1, every term): reduction over the epochs and update in one launch; as two
    kernels (LCMI_SPLIT_UPDATE=1) the same bits."""
    monkeypatch.delenv('LCMI_SPLIT_UPDATE', raising=False)
    pt = JT.point_of(case)
    got = _run(ctx, pt, (term,), JT.FREE_H)
    _against_the_oracle(f'{case} {term}', got, JT.oracle_trajectory(pt, (term,), JT.FREE_H), JT.FREE_H)
    monkeypatch.setenv('LCMI_SPLIT_UPDATE', '1')
    split = _run(ctx, pt, (term,), JT.FREE_H)
    np.testing.assert_array_equal(got[0], split[0])
    for k in JT.FREE_H:
        np.testing.assert_array_equal(got[1][k], split[1][k], err_msg=k)


def test_persistent_point_source_loop(ctx, monkeypatch):
    """Photometry at fixed positions: the whole loop inside one launch (default) or a kernel pair per iteration
    (LCMI_PS_LOOP=1), with positivity(a) acting on one flux in three."""
    monkeypatch.delenv('LCMI_PS_LOOP', raising=False)
    pt = JT.point_of(JT.LOOP_PERSISTENT, False)
    free = JT.FREE_PERSISTENT
    got = _run(ctx, pt, ('pos_ps',), free)
    _against_the_oracle(f'{JT.LOOP_PERSISTENT} pos_ps', got, JT.oracle_trajectory(pt, ('pos_ps',), free), free)
    monkeypatch.setenv('LCMI_PS_LOOP', '1')
    pair = _run(ctx, pt, ('pos_ps',), free)
    for k in free:
        np.testing.assert_array_equal(got[1][k], pair[1][k], err_msg=k)


def _batch(ctx, stars, background):
    from lightcurver_amd.joint import StarPhotometryBatch
    b = StarPhotometryBatch([(pt['ds']['data'], pt['ds']['noisemap'].astype(np.float64) ** 2, pt['ds']['psf']) for pt in stars],
                            2, 1, ctx, background=background)
    names = ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha', 'mean') + (('h',) if background else ())
    b.set_params(**{k: np.concatenate([pt['p'][k] for pt in stars]) for k in names})
    return b


def _batch_settings(stars, on, background):
    dev = JT.settings(stars[0], on)[0]
    if background:
        dev['W'] = np.stack([pt['W'] for pt in stars])
    return dev


def _check_batch(ctx, stars, term, free, background):
    from lightcurver_amd import _lib
    on = (term,) + (JT.bg_carrier(term) if background else ())
    b = _batch(ctx, stars, background)
    try:
        for refused in ('pts', 'prior_cx', 'prior_cy'):
            with pytest.raises(_lib.LcError):
                b.set_loss(**_batch_settings(stars, on + (refused,), background))
        if background and JT.bg_carrier(term):      # the flux terms alone leave h unregularised: refused, not run
            b.set_loss(**_batch_settings(stars, (term,), background))
            b.set_free(list(free))
            with pytest.raises(_lib.LcError):
                b.run_adabelief(1, **CFG)
        b.set_loss(**_batch_settings(stars, on, background))
        b.set_free(list(free))
        b.run_adabelief(JT.T_LOOP, **CFG)
        got, hist = b.get_params(), np.asarray(b.loss_history(), np.float64)
        for g, pt in enumerate(stars):
            mine = (hist[g], {k: np.asarray(b.split(got[k], k)[g]) for k in free})
            _against_the_oracle(f'star {g} ({pt["E"]} epochs) {term}', mine, JT.oracle_trajectory(pt, on, free), free)
            alone = _run(ctx, pt, on, free)
            np.testing.assert_array_equal(np.float32(hist[g]), np.float32(alone[0]))
            for k in free:
                np.testing.assert_array_equal(mine[1][k], alone[1][k], err_msg=f'{g} {k}')
    finally:
        b.close()


@pytest.mark.parametrize('term', JT.BATCH_PS['terms'])
def test_star_batch_without_background(ctx, term):
    """Stars of 3, 5 and 4 epochs in one object: each against the oracle and bit for bit its own JointFit; the point-source
    starlet term and the priors are refused."""
    stars = JT.star_points(JT.BATCH_PS['epochs'], JT.BATCH_PS['n'], False)
    _check_batch(ctx, stars, term, JT.FREE_STAR, False)


@pytest.mark.parametrize('term', JT.BATCH_BG_TERMS)
@pytest.mark.parametrize('b', JT.BATCH_BG, ids=lambda b: f'n{b["n"]}')
def test_star_batch_with_backgrounds(ctx, b, term):
    """A background per star, each with its own negative patch.  The object runs only with h free and regularised, so the two
    flux terms run beside positivity(h) (and the oracle with the same two terms)."""
    stars = JT.star_points(b['epochs'], b['n'], True)
    _check_batch(ctx, stars, term, JT.FREE_STAR + ('h',), True)
