"""The active points of tests/_joint_terms.py, on the float64 oracle alone: at every case of the GPU lists every term of the
joint loss has a value > 0 and, in every block it touches, a gradient of at least a tenth of the block's full gradient that
differs from every other term's; the term-on trajectory of every loop case lies ten tolerances from the term-off one.  Then
the C ports (oracle/joint_cpu.c in float64 at 1e-9, oracle/joint_ps_cpu.c for what it has) term by term, and the distance of
the float32 port from the oracle per term and case - the figure the device bounds of tests/test_joint_terms_gpu.py may fall
back on (R_GRAD / R_LOSS of tests/_joint_terms.py)."""
import numpy as np
import pytest

from oracle.joint_cpu import JointCpu
from tests import _joint_terms as JT

EVAL = JT.eval_list()
_ID = lambda v: f'{v[0]}-{"h" if v[1] else "ps"}-{len(v[2])}on'.replace(' ', '')
SHARE = 0.1


@pytest.mark.parametrize('case,with_h,base,terms,free', EVAL, ids=[_ID(v) for v in EVAL])
def test_every_term_acts_and_is_distinguishable(case, with_h, base, terms, free):
    pt = JT.point_of(case, with_h)
    a = pt['p']['a'].reshape(pt['E'], pt['M'])
    assert np.abs(a).min() > 10 * JT.T_LOOP * JT.LR_LOOP          # no flux comes near zero during a run
    assert (a < 0).any() and ((a > 0).any(axis=0) & ((a < 0).any(axis=0) | (pt['E'] < 3))).all()
    _, g_full = JT.oracle_eval(pt, base, free)
    term_g = {}
    for t in terms:
        dL, dg = JT.oracle_term(pt, t, free, base=base)
        term_g[t] = dg
        assert dL > 0, t
        for b in JT.BLOCKS[t]:
            share = np.abs(dg[b]).max() / np.abs(g_full[b]).max()
            print(f'{case} {t} {b}: share {share:.3f}')
            assert share >= SHARE, (t, b, share)
        for b in free:                                             # and nothing outside its blocks
            if b not in JT.BLOCKS[t]:
                assert np.abs(dg[b]).max() <= 1e-9 * np.abs(g_full[b]).max(), (t, b)
    for t in terms:
        for u in terms:
            for b in set(JT.BLOCKS[t]) & set(JT.BLOCKS[u]):
                if t < u:
                    # further apart than the loosest bound the device test may apply to either (2 R_CAP of the larger one)
                    d = np.abs(term_g[t][b] - term_g[u][b]).max()
                    assert d > 0.1 * max(np.abs(term_g[t][b]).max(), np.abs(term_g[u][b]).max()), (t, u, b)


LOOPS = JT.loop_list()


@pytest.mark.parametrize('label,pt,term,free,carrier', LOOPS, ids=[f'{v[0]}-{v[2]}'.replace(' ', '') for v in LOOPS])
def test_term_moves_the_trajectory_by_ten_tolerances(label, pt, term, free, carrier):
    if pt['E'] >= 3:
        a = pt['p']['a'].reshape(pt['E'], pt['M'])
        assert ((a < 0).any(axis=0) & (a > 0).any(axis=0)).all()     # per star: flux uniformity and positivity act
    _, g_on = JT.oracle_eval(pt, (term,) + carrier, free)
    dL, dg = JT.oracle_term(pt, term, free, base=(term,) + carrier)
    assert dL > 0
    for b in JT.BLOCKS[term]:
        if b in free:
            assert np.abs(dg[b]).max() >= SHARE * np.abs(g_on[b]).max(), b
    on = JT.oracle_trajectory(pt, (term,) + carrier, free)
    off = JT.oracle_trajectory(pt, carrier, free)
    dist = JT.trajectory_distance(on, off, free)
    print(label, term, 'max|a| %.1f' % np.abs(pt['p']['a']).max(), {k: round(float(v), 1) for k, v in dist.items()})
    assert dist['hist'] >= 10.0
    assert max(v for k, v in dist.items() if k != 'hist') >= 10.0
    # no flux crosses zero during the run
    assert (np.sign(on[1]['a']) == np.sign(pt['p']['a'])).all() and np.abs(on[1]['a']).min() > 5 * JT.T_LOOP * JT.LR_LOOP


def _port(pt, double):
    ds = pt['ds']
    c = JointCpu(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], pt['ss'], pt['M'], double=double, threads=2)
    c.set_params(**pt['p'])
    return c


def _port_eval(c, pt, on):
    dev = {k: v for k, v in JT.settings(pt, on)[0].items() if k != 'prior'}
    c.set_loss(**dev)
    L, g = c.eval(threads=2)
    return L, {k: np.asarray(v, np.float64) for k, v in g.items()}


PORT_TERMS = ('scales', 'hf', 'pos', 'pos_ps', 'pts', 'fu')      # oracle/joint_cpu.c has no prior


@pytest.mark.parametrize('case,with_h,base,terms,free', EVAL, ids=[_ID(v) for v in EVAL])
def test_c_port_equals_the_oracle_term_by_term(case, with_h, base, terms, free):
    pt = JT.point_of(case, with_h)
    base = tuple(t for t in base if t in PORT_TERMS)
    c = _port(pt, True)
    try:
        L1, g1 = _port_eval(c, pt, base)
        for t in terms:
            if t not in PORT_TERMS:
                continue
            L0, g0 = _port_eval(c, pt, tuple(u for u in base if u != t))
            dL, dg = JT.oracle_term(pt, t, free, base=base)
            assert abs((L1 - L0) - dL) <= 1e-9 * abs(dL), t
            for b in free:
                ref = np.abs(dg[b]).max()
                assert np.abs((g1[b] - g0[b]) - dg[b]).max() <= 1e-9 * max(ref, 1e-3 * np.abs(g1[b]).max()), (t, b)
    finally:
        c.close()


@pytest.mark.parametrize('case', JT.CASES_PS + [JT.LOOP_PERSISTENT], ids=str)
def test_point_source_port_at_negative_fluxes(case):
    """oracle/joint_ps_cpu.c has chi2 alone of the seven terms: value and gradient at the active point (fluxes of both signs)."""
    from oracle.joint_ps_cpu import JointPsCpu
    pt = JT.point_of(case, False)
    if np.any(pt['p']['alpha'] != 0):
        pytest.fail('the point-source port has no rotation: list cases with alpha = 0')
    ds = pt['ds']
    c = JointPsCpu(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], pt['ss'], pt['M'], double=True)
    c.set_params(**{k: pt['p'][k] for k in JT.FREE_PS})
    L, g = c.eval(threads=2)
    Lo, go = JT.oracle_eval(pt, (), JT.FREE_PS)
    assert abs(L - Lo) <= 1e-9 * abs(Lo)
    for b in JT.FREE_PS:
        assert np.abs(g[b] - go[b]).max() <= 1e-9 * np.abs(go[b]).max(), b


@pytest.mark.parametrize('case,with_h,base,terms,free', EVAL, ids=[_ID(v) for v in EVAL])
def test_float32_port_distance_per_term(case, with_h, base, terms, free):
    """float32 arithmetic of the same SPEC on the CPU: its distance from the float64 oracle on each term's own value and
    gradient (printed; DESIGN.md holds the table).  A device bound other than the project's 1e-4 / 3e-5 must be at most four
    times this figure and at most 2e-3."""
    pt = JT.point_of(case, with_h)
    base = tuple(t for t in base if t in PORT_TERMS)
    c = _port(pt, False)
    try:
        L1, g1 = _port_eval(c, pt, base)
        for t in terms:
            if t not in PORT_TERMS:
                assert JT.r_key(t, case) not in JT.R_GRAD and JT.r_key(t, case) not in JT.R_LOSS
                continue
            L0, g0 = _port_eval(c, pt, tuple(u for u in base if u != t))
            dL, dg = JT.oracle_term(pt, t, free, base=base)
            dist_L = abs((L1 - L0) - dL) / abs(dL)
            dist_g = max(np.abs((g1[b] - g0[b]) - dg[b]).max() / np.abs(dg[b]).max() for b in JT.BLOCKS[t])
            print(f'{case} {t}: float32 port value {dist_L:.1e} gradient {dist_g:.1e}')
            assert np.isfinite(dist_L) and np.isfinite(dist_g)
            assert JT.R_DEFAULT <= JT.r_grad(t, case) <= JT.R_CAP and JT.RL_DEFAULT <= JT.r_loss(t, case) <= JT.R_CAP
            if JT.r_key(t, case) in JT.R_GRAD:
                assert JT.R_GRAD[JT.r_key(t, case)] <= 4 * dist_g, (t, dist_g)
            if JT.r_key(t, case) in JT.R_LOSS:
                assert JT.R_LOSS[JT.r_key(t, case)] <= 4 * dist_L, (t, dist_L)
    finally:
        c.close()
