"""Active points of the joint-fit loss: parameters at which every one of its seven terms

    0.5 chi2 + l1_starlet(h) + positivity(h) + positivity(a) + pts_source + flux_uniformity + prior(c_x, c_y)

contributes a gradient of at least a tenth of its block's, the case lists of tests/test_joint_terms_gpu.py, and the float64
oracle's values at them (computed once per process and shared; callers must not modify what they get).
tests/test_joint_terms_cpu.py proves the activity on the oracle alone; DESIGN.md "Joint-loss terms, one at a time" holds
the figures."""
import functools

import numpy as np

from lightcurver_amd.synthetic import make_roi_dataset
from oracle import model as om, optim as oo
from tests.test_joint_gpu import _params

# The noise map is multiplied by QUIET: chi2 and its gradient shrink by QUIET^2, the starlet weights W by QUIET; positivity,
# flux uniformity and the prior do not shrink.  With these strengths every term clears the 0.1 share at every listed case.
QUIET = 30.0
# (the point-source starlet term is weighted by W[0]: the propagated one shrinks with QUIET, the default one does not)
LAMS = dict(scales=15.0, hf=60.0, pos=20.0, pos_ps=50.0, pts=3000.0, fu=50.0)     # with a background: W propagated
LAMS_PS = dict(LAMS, pts=100.0)                                                    # h zero and fixed: default W
PRIOR_OFFSET = dict(c_x=0.1, c_y=-0.07)
PRIOR_SIGMA = dict(c_x=0.02, c_y=0.03)
PRIOR_OFF_SIGMA = 1e6          # a prior this wide contributes (offset / 1e6)^2 / 2 ~ 1e-14: nothing measurable
T_LOOP, LR_LOOP = 20, 1e-3

FREE_H = ('a', 'c_x', 'c_y', 'dx', 'dy', 'h', 'mean')
FREE_PS = ('a', 'c_x', 'c_y', 'dx', 'dy', 'mean')

_DEV = dict(scales='lam_scales', hf='lam_hf', pos='lam_positivity', pos_ps='lam_positivity_ps', pts='lam_pts_source',
            fu='lam_flux_uniformity')
_ORA = dict(scales='lam_scales', hf='lam_hf', pos='lam_pos', pos_ps='lam_pos_ps', pts='lam_pts', fu='lam_fu')
# term -> (device keyword of JointFit.set_loss, oracle keyword of om.deconv_loss, parameter blocks the term touches);
# the two priors travel in `prior` on both sides (settings() below)
TERMS = {
    'scales': (_DEV['scales'], _ORA['scales'], ('h',)),
    'hf': (_DEV['hf'], _ORA['hf'], ('h',)),
    'pos': (_DEV['pos'], _ORA['pos'], ('h',)),
    'pos_ps': (_DEV['pos_ps'], _ORA['pos_ps'], ('a',)),
    'pts': (_DEV['pts'], _ORA['pts'], ('a', 'c_x', 'c_y')),
    'fu': (_DEV['fu'], _ORA['fu'], ('a',)),
    'prior_cx': ('prior', 'prior', ('c_x',)),
    'prior_cy': ('prior', 'prior', ('c_y',)),
}
ALL = tuple(TERMS)
H_TERMS = ('scales', 'hf', 'pos')
PS_TERMS = ('pos_ps', 'fu', 'pts', 'prior_cx', 'prior_cy')
BLOCKS = {t: v[2] for t, v in TERMS.items()}

# (E, M, n, ss, alpha_sigma) per evaluation path.  At subsampling 1 the path follows N = n (find_jv_ss1, DESIGN.md
# "Subsampling 1 at every stamp size"): 32, 48, 64 the single-workgroup update, 24, 40, 56 the run-time-N (multi-block) one,
# 128 the matrix-core chain.
CASES_ONE_WG = [(4, 2, 16, 2, 0.0), (3, 1, 16, 1, 0.0), (3, 3, 24, 2, 0.5), (3, 2, 32, 2, 0.3),
                (3, 2, 32, 1, 0.3), (3, 2, 48, 1, 0.3), (2, 3, 64, 1, 0.3)]
CASE_MULTI_BLOCK = (2, 2, 40, 2, 0.3)
CASES_MULTI_BLOCK_SS1 = [(3, 2, 24, 1, 0.5), (3, 2, 40, 1, 0.3), (2, 2, 56, 1, 0.3)]
CASES_FORCED_GLOBAL = [(4, 2, 16, 2, 0.0), (3, 2, 32, 2, 0.3)]
CASE_N128 = (2, 2, 64, 2, 0.3)
CASE_N128_SS1 = (3, 2, 128, 1, 0.0)
CASES_N128 = [CASE_N128, CASE_N128_SS1]
N128_TERMS = ('scales', 'hf', 'pos', 'pts')
CASES_PS = [(4, 2, 16, 2, 0.0), (3, 1, 32, 2, 0.0), (4, 1, 24, 1, 0.0), (4, 2, 40, 1, 0.0), (3, 1, 48, 1, 0.0), (2, 2, 128, 1, 0.0)]
CASES_STEP = [(4, 2, 16, 2, 0.0), (2, 2, 64, 2, 0.3)]
# loops: (E, M, n, ss, alpha_sigma) and the terms run one at a time beside chi2
LOOP_SECOND_STREAM = [((4, 2, 16, 2, 0.0), ALL), ((4, 2, 32, 2, 0.0), ALL),
                      ((4, 2, 32, 1, 0.0), ALL), ((4, 2, 48, 1, 0.0), ALL)]
LOOP_FUSED = [((4, 2, 40, 2, 0.0), ('pos', 'pos_ps', 'pts', 'prior_cx')), ((4, 2, 64, 2, 0.0), ('pos', 'pos_ps', 'pts', 'prior_cx')),
              ((4, 2, 24, 1, 0.0), ALL), ((4, 2, 40, 1, 0.0), ALL), ((4, 2, 56, 1, 0.0), ALL)]
LOOP_PERSISTENT = (7, 1, 32, 2, 0.0)
BATCH_PS = dict(epochs=(3, 5, 4), n=16, terms=('pos_ps', 'fu'))
BATCH_BG = [dict(epochs=(3, 4), n=16), dict(epochs=(4, 3), n=24)]
BATCH_BG_TERMS = ('pos_ps', 'fu', 'pos', 'scales', 'hf')


def seed_of(case):
    E, M, n, ss, alpha = case
    return 900 + 7 * n + 3 * M + E + ss


def negative_fluxes(E, M):
    """Every third entry of a (epoch-major); with M a multiple of 3 the pattern shifts by one per epoch, so that no
    source is negative (or positive) at every epoch."""
    e, i = np.divmod(np.arange(E * M), M)
    return (e * M + i + (e if M % 3 == 0 else 0)) % 3 == 2


@functools.lru_cache(maxsize=None)
def active_point(E, M, n, ss, seed, alpha_sigma=0.0, with_h=True, quiet=QUIET):
    """-> dict(ds, p, prior, W): make_roi_dataset + the jitter of tests/test_joint_gpu.py::_params, changed so that every
    term acts (module docstring).  ds['noisemap'] is already multiplied by `quiet`; W is the oracle's noise propagation
    (None without a background); prior: dict of c_x_mean, c_x_sigma, c_y_mean, c_y_sigma."""
    ds = dict(make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=seed, alpha_sigma=alpha_sigma, with_background=with_h))
    p = _params(ds, np.random.default_rng(seed + 7), with_h=with_h)
    neg = negative_fluxes(E, M)
    da = np.zeros_like(p['a'])
    da[neg] = -0.2 * np.abs(p['a'][neg]) - p['a'][neg]
    p['a'] = p['a'] + da
    # The data follow the negative fluxes (the model is linear in a), and a little further: they ask for 1.5 times the
    # negative flux, so chi2 pushes those entries down where positivity(a) and the flux uniformity push them up.  AdaBelief
    # steps do not depend on the gradient's size: a term that only lengthened the chi2 gradient would leave the trajectory
    # where it was, one that turns it round moves it by 2 lr per step.
    dp = {k: om.T(v) for k, v in dict(p, a=da * (1.0 + 0.1 * neg / 1.2), h=np.zeros_like(p['h']), mean=np.zeros(E)).items()}
    ds['data'] = (ds['data'].astype(np.float64) + om.deconv_model(dp, om.T(ds['psf']), ss, n).numpy()).astype(np.float32)
    if with_h:
        N = n * ss
        h = p['h'].reshape(N, N)
        h[:N // 2, :N // 2] -= 0.3 * h.max()
    ds['noisemap'] = (ds['noisemap'].astype(np.float64) * quiet).astype(np.float32)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}    # the values the device holds
    prior = dict(c_x_mean=p['c_x'] + PRIOR_OFFSET['c_x'], c_x_sigma=np.full(M, PRIOR_SIGMA['c_x']),
                 c_y_mean=p['c_y'] + PRIOR_OFFSET['c_y'], c_y_sigma=np.full(M, PRIOR_SIGMA['c_y']))
    prior = {k: v.astype(np.float32).astype(np.float64) for k, v in prior.items()}
    W = None
    if with_h:
        W = om.propagate_noise_deconv(om.T(ds['noisemap']) ** 2, om.T(ds['psf']), ss).numpy()
    return dict(ds=ds, p=p, prior=prior, W=W, E=E, M=M, n=n, ss=ss, with_h=with_h)


def point_of(case, with_h=True):
    E, M, n, ss, alpha = case
    return active_point(E, M, n, ss, seed_of(case), alpha, with_h)


def lams_of(pt):
    return LAMS if pt['with_h'] else LAMS_PS


def settings(pt, on, lams=None):
    """-> (keywords of JointFit.set_loss, keywords of om.deconv_loss) with exactly the terms `on` switched on."""
    lams = lams or lams_of(pt)
    M = pt['M']
    dev = {_DEV[t]: (lams[t] if t in on else 0.0) for t in _DEV}
    ora = {_ORA[t]: (lams[t] if t in on else 0.0) for t in _ORA}
    if pt['W'] is not None:
        dev['W'] = pt['W']
        ora['W'] = om.T(pt['W'])
    if 'prior_cx' in on or 'prior_cy' in on:
        pr = dict(pt['prior'])
        if 'prior_cx' not in on:
            pr['c_x_sigma'] = np.full(M, PRIOR_OFF_SIGMA)
        if 'prior_cy' not in on:
            pr['c_y_sigma'] = np.full(M, PRIOR_OFF_SIGMA)
        dev['prior'] = pr
        ora['prior'] = [('c_x', pr['c_x_mean'], pr['c_x_sigma']), ('c_y', pr['c_y_mean'], pr['c_y_sigma'])]
    return dev, ora


def oracle_fn(pt, on, lams=None):
    ds = pt['ds']
    d, s2, ps = om.T(ds['data']), om.T(ds['noisemap']) ** 2, om.T(ds['psf'])
    ora = settings(pt, on, lams)[1]
    return lambda q: om.deconv_loss(q, d, s2, ps, pt['ss'], **ora)


def _key(pt):
    return (pt['E'], pt['M'], pt['n'], pt['ss'], pt['with_h'], pt['p']['a'].tobytes()[:64])


_EVAL, _TRAJ = {}, {}


def oracle_eval(pt, on, free, lams=None):
    """-> (loss, {block: gradient}) of the float64 oracle with the terms `on`; cached."""
    k = (_key(pt), tuple(sorted(on)), tuple(free), None if lams is None else tuple(sorted(lams.items())))
    if k not in _EVAL:
        po = {q: om.T(v) for q, v in pt['p'].items()}
        L, g = oo.value_and_grad(oracle_fn(pt, on, lams), po, list(free))
        _EVAL[k] = (float(L), {q: v.numpy() for q, v in g.items()})
    return _EVAL[k]


def oracle_term(pt, term, free, base=ALL, lams=None):
    """The term alone, as the difference of two oracle evaluations: (dL, {block: dg}) with `base` on / `base` minus term."""
    on = tuple(t for t in ALL if t in base or t == term)
    off = tuple(t for t in on if t != term)
    L1, g1 = oracle_eval(pt, on, free, lams)
    L0, g0 = oracle_eval(pt, off, free, lams)
    return L1 - L0, {q: g1[q] - g0[q] for q in free}


def oracle_trajectory(pt, on, free, lams=None, T=T_LOOP, lr=LR_LOOP):
    """-> (history (T + 1,), final parameters) of oo.adabelief with the schedule; cached."""
    k = (_key(pt), tuple(sorted(on)), tuple(free), None if lams is None else tuple(sorted(lams.items())), T, lr)
    if k not in _TRAJ:
        po = {q: om.T(v) for q, v in pt['p'].items()}
        pf, lh, l0 = oo.adabelief(oracle_fn(pt, on, lams), po, list(free), lr, T, schedule=True)
        _TRAJ[k] = (np.array([l0] + lh), {q: v.numpy() for q, v in pf.items()})
    return _TRAJ[k]


def trajectory_distance(ref, other, free, T=T_LOOP, lr=LR_LOOP):
    """The quantities the GPU trajectory tests bound (2e-4 on the history and a, 5e-4 px on positions and shifts, the h
    rule of test_adabelief_trajectory), each divided by its bound: {'hist': ..., block: ...}."""
    (h0, p0), (h1, p1) = ref, other
    out = {'hist': np.abs(h1 - h0).max() / np.abs(h0).max() / 2e-4}
    for q in free:
        d = np.abs(p1[q] - p0[q])
        if q == 'a':
            out[q] = d.max() / np.abs(p0[q]).max() / 2e-4
        elif q == 'h':
            out[q] = max(d.max() / (0.05 * T * lr), np.median(d) / 1e-5)
        elif q != 'mean':
            out[q] = d.max() / 5e-4
    return out


# Where the device cannot meet r = 1e-4 (gradient) / r_L = 3e-5 (value) on a term alone, the bound is four times the
# distance of the float32 C port (oracle/joint_cpu.c, same SPEC in float32 on the CPU) from the float64 oracle for that term
# and case, at most 2e-3; tests/test_joint_terms_cpu.py checks every entry against the port.  (term, E, M, n, ss) -> r: an entry holds
# for its own case and no other of the same size (the point-source-only case at n = 128 keeps 1e-4)
R_DEFAULT, RL_DEFAULT, R_CAP = 1e-4, 3e-5, 2e-3
# pts at (3, 2, 128, 1, 0): the c_y gradient of the point-source starlet term sums the signs of 16384 coefficients per scale,
# and the float32 port is 1.87e-4 of the term's largest element from the oracle there (c_x 8.7e-6, a 2.1e-7); the device
# measures 1.8e-4 in c_y, 8.9e-6 in c_x - the same arithmetic.  4 x 1.87e-4 = 7.47e-4.
R_GRAD = {('pts', 3, 2, 128, 1): 7.4e-4}
R_LOSS = {}


def r_key(term, case):
    return (term,) + tuple(case[:4])


def r_grad(term, case):
    return R_GRAD.get(r_key(term, case), R_DEFAULT)


def r_loss(term, case):
    return R_LOSS.get(r_key(term, case), RL_DEFAULT)


def star_points(epochs, n, with_h, seed=700):
    """One active point per star of a batch (M = 1)."""
    return [active_point(E, 1, n, 2, seed + 11 * g + n, 0.0, with_h) for g, E in enumerate(epochs)]


FREE_STAR = ('a', 'c_x', 'c_y', 'dx', 'dy')
FREE_PERSISTENT = ('a', 'dx', 'dy', 'mean')


def eval_list():
    """Every (case, with_h, base, terms, free) the evaluation tests of the device take: `terms` one at a time, switched on and
    off beside the other terms of `base`."""
    out = []
    for c in dict.fromkeys(CASES_ONE_WG + [CASE_MULTI_BLOCK] + CASES_MULTI_BLOCK_SS1 + CASES_FORCED_GLOBAL + CASES_STEP + CASES_N128):
        out.append((c, True, ALL, ALL, FREE_H))
    for c in CASES_N128:
        out.append((c, True, ALL, N128_TERMS, FREE_H))
        out.append((c, True, ('pos', 'pts'), ('pos', 'pts'), FREE_H))
    for c in CASES_PS:
        out.append((c, False, PS_TERMS, PS_TERMS, FREE_PS))
    return out


def loop_list():
    """Every (label, point, term, free, carrier) of the loop tests: the term alone beside chi2 - and beside `carrier`, the
    terms the path cannot run without (bg_carrier)."""
    out = []
    for c, terms in LOOP_SECOND_STREAM + LOOP_FUSED:
        out += [(str(c), point_of(c), t, FREE_H, ()) for t in terms]
    out.append((str(LOOP_PERSISTENT), point_of(LOOP_PERSISTENT, False), 'pos_ps', FREE_PERSISTENT, ()))
    for g, pt in enumerate(star_points(BATCH_PS['epochs'], BATCH_PS['n'], False)):
        out += [(f'star {g} of {BATCH_PS}', pt, t, FREE_STAR, ()) for t in BATCH_PS['terms']]
    for b in BATCH_BG:
        for g, pt in enumerate(star_points(b['epochs'], b['n'], True)):
            out += [(f'star {g} of {b}', pt, t, FREE_STAR + ('h',), bg_carrier(t)) for t in BATCH_BG_TERMS]
    return out


def bg_carrier(term):
    """The batch with a background per star runs only with h free and regularised (LC_ERR_UNSUPPORTED otherwise): the two
    flux terms run there beside positivity(h), on and off against that."""
    return () if term in H_TERMS else ('pos',)
