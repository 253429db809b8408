"""The two device forms of the bounded L-BFGS held to the restatement of tests/_lbfgs.py step by step.

PSF form (csrc/psf_lbfgs.h, and csrc/lbfgs_host.h under LCMI_LBFGS_HOST=1): fit_moffat(k) for a ladder of k against the
restatement at maxiter k, the restatement driven by set_moffat / set_stars / evaluate(), i.e. by the very evaluation the
fit uses (asserted first).  Both sides hold their state in double and differ only in the order, and possibly the fusing,
of sums of at most 52 terms, so the float32 read-backs are expected to be bit-equal; allowed per parameter is the larger
of one float32 ulp and 4 x the restatement's own difference between its sequential and butterfly orders.

Joint form (csrc/joint_lbfgs.h, driver lc_joint_run_lbfgs): one step ahead.  run_lbfgs(k) for k = 1 .. K gives the device's
own iterates x_k; its own pairs are rebuilt from them and from loss_grad at them, and every step x_k -> x_k+1 is compared
with the restatement's direction from those pairs, so no error is carried from one step into the next."""
import numpy as np
import pytest

from tests import _lbfgs as L
from tests import helpers as H

pytestmark = pytest.mark.gpu


# ---- PSF form ------------------------------------------------------------------------------------------------------------
class _PsfCase:
    """One (S, ss): the batch, its start, and the restatement in both orders at the longest ladder rung.  A problem's
    iterates do not depend on maxiter before it is reached, so rung k is the prefix of length k."""

    def __init__(self, ctx, S, ss):
        from lightcurver_amd.psf_batch import PsfBatch
        self.S, self.ss, self.F, self.n = S, ss, L.PSF_F, L.PSF_N
        self.ds, self.mof0, self.st0 = L.psf_problem(S, ss)
        self.batch = PsfBatch(self.ds['data'], H.weights_from(self.ds), ss, ctx)
        self.batch.set_grid(None)
        self.batch.set_regularization(None, 0, 0)
        self.lo, self.hi = L.psf_bounds(self.F, S, self.n, ss)
        self.x0 = L.psf_pack(self.mof0, self.st0)
        ev = L.psf_eval(self.batch, self.st0[..., 3])
        kmax = max(L.PSF_K)
        self.ref = {o: L.restate(ev, self.x0, self.lo, self.hi, kmax, order=o) for o in ('sequential', 'butterfly')}
        self.reset()

    def reset(self):
        self.batch.set_moffat(self.mof0)
        self.batch.set_stars(self.st0)

    def at(self, order, k):
        """Restatement at maxiter k: x [F][D], f [F], iterations [F]."""
        r = self.ref[order]
        it = [min(k, len(r['iterates'][f]) - 1) for f in range(self.F)]
        return (np.stack([r['iterates'][f][i] for f, i in enumerate(it)]),
                np.array([r['losses'][f][i] for f, i in enumerate(it)]), it)

    def rounds(self, order, k):
        """Evaluations after the first that maxiter k costs: the slowest frame's trials, failed line search included."""
        r = self.ref[order]
        out = 0
        for f in range(self.F):
            n = sum(r['trials'][f][:k])
            if r['ls_failed'][f] and len(r['trials'][f]) < k:
                n += L.MAX_LS
            out = max(out, n)
        return out

    def fit(self, k):
        """Reset, fit_moffat(k) -> (x [F][D] of the float32 read-backs, final loss float32, stars)."""
        self.reset()
        final = self.batch.fit_moffat(k)
        st = self.batch.get_stars()
        return L.psf_pack(self.batch.get_moffat(), st), final, st


_cases = {}


@pytest.fixture
def psf_case(ctx, request):
    key = request.param
    if key not in _cases:
        _cases[key] = _PsfCase(ctx, *key)
    return _cases[key]


PSF_CASES = [(S, ss) for ss in L.PSF_SS for S in L.PSF_S]


@pytest.mark.parametrize('psf_case', PSF_CASES, indirect=True, ids=lambda c: f'S{c[0]}-ss{c[1]}')
def test_psf_problem_is_what_it_says(psf_case):
    """The properties the comparison below relies on, asserted in the restatement on the device's own evaluation."""
    c = psf_case
    for order in ('sequential', 'butterfly'):
        r = c.ref[order]
        for k in L.PSF_K:
            assert c.rounds(order, k) <= L.psf_round_budget(k), (order, k)   # the device form's round budget is not met
        x, f, it = c.at(order, max(L.PSF_K))
        assert not any(r['ls_failed'])
        # the frames finish in different rounds at some rung of the ladder
        assert any(len({sum(r['trials'][fr][:k]) for fr in range(c.F)}) > 1 for k in L.PSF_K)
        assert x[2, 0] == c.hi[2, 0] and x[2, 1] == c.hi[2, 1]               # frame 2: the FWHM bound ends active
    clipped = np.clip(c.x0, c.lo, c.hi)
    assert c.x0[1, 3] > c.hi[1, 3] and c.x0[1, 4 + c.S] > c.hi[1, 4 + c.S]   # frame 1: beta and one x0 start outside
    assert np.array_equal(c.ref['sequential']['iterates'][1][0], clipped[1])
    a, b = c.ref['sequential'], c.ref['butterfly']
    assert np.array_equal(a['iters'], b['iters'])


@pytest.mark.parametrize('host', (False, True), ids=('device', 'host'))
@pytest.mark.parametrize('psf_case', PSF_CASES, indirect=True, ids=lambda c: f'S{c[0]}-ss{c[1]}')
def test_psf_fit_follows_the_restatement(psf_case, host, monkeypatch):
    c = psf_case
    F, S = c.F, c.S
    if host:
        monkeypatch.setenv('LCMI_LBFGS_HOST', '1')
    order = 'sequential' if host else 'butterfly'
    # the fit's evaluation is the test's: fit_moffat(0) returns the bits of evaluate()['loss'] at the clipped start
    x, final0, st = c.fit(0)
    clipped = np.clip(c.x0, c.lo, c.hi)
    mof, stc = L.psf_unpack(clipped, c.st0[..., 3])
    assert np.array_equal(L.bits(x.astype(np.float32)), L.bits(clipped.astype(np.float32)))
    c.batch.set_moffat(mof)
    c.batch.set_stars(stc)
    assert np.array_equal(L.bits(final0), L.bits(c.batch.evaluate()['loss']))
    assert np.array_equal(L.bits(final0.astype(np.float64)), L.bits(np.array([c.ref[order]['losses'][f][0] for f in range(F)])))
    worst, unequal, total = 0.0, 0, 0
    for k in L.PSF_K:
        x, final, st = c.fit(k)
        xs, fs, its = c.at('sequential', k)
        xb, fb, itb = c.at('butterfly', k)
        # Iteration counts: the fit does not return them, so two checks stand in for the direct comparison.  The
        # restatement's counts agree between its two orders (here), and the parameters the fit returns are those of
        # iterate k of the restatement and of neither neighbour (below): a fit one iteration short or long fails there.
        assert its == itb
        xr, fr = (xs, fs) if host else (xb, fb)
        want = xr.astype(np.float32)
        tol = np.maximum(L.ulp32(want), L.REASSOCIATION_MARGIN * np.abs(xs - xb))
        diff = np.abs(x - want.astype(np.float64))
        ne = L.bits(x.astype(np.float32)) != L.bits(want)
        worst = max(worst, float((diff / tol).max()))
        unequal += int(ne.sum())
        total += ne.size
        assert np.all(diff <= tol), (k, np.argwhere(diff > tol)[:5], (diff / tol).max())
        # the fit stopped at iterate k of every frame and at no other: k is the nearest iterate of the restatement
        ref = c.ref[order]
        for f in range(F):
            for other in (its[f] - 1, its[f] + 1):
                if 0 <= other < len(ref['iterates'][f]):
                    assert np.abs(x[f] - ref['iterates'][f][other]).max() > diff[f].max(), (k, f, other)
        # the sky column is untouched, and the loss returned is the loss of the parameters returned
        assert np.array_equal(L.bits(st[..., 3]), L.bits(c.st0[..., 3]))
        now = c.batch.evaluate()['loss']
        assert np.array_equal(L.bits(final), L.bits(now))
        same = ~ne.any(axis=1)
        assert np.array_equal(L.bits(final[same].astype(np.float64)), L.bits(fr[same]))
        # A frame with a parameter off by rounding (none is expected) needs a bound for its loss derived from that
        # difference before it can pass: until then it fails here.
        assert same.all(), ('frames with parameters not bit-equal', k, np.flatnonzero(~same))
    print(f'PSF form ({"host" if host else "device"}), S = {S}, ss = {c.ss}: worst ratio {worst:.3g}, {unequal} of {total} '
          'parameters not bit-equal')


@pytest.mark.parametrize('host', (False, True), ids=('device', 'host'))
@pytest.mark.parametrize('psf_case', PSF_CASES, indirect=True, ids=lambda c: f'S{c[0]}-ss{c[1]}')
def test_psf_frame_alone_equals_frame_in_the_batch(psf_case, host, ctx, monkeypatch):
    from lightcurver_amd.psf_batch import PsfBatch
    c = psf_case
    if host:
        monkeypatch.setenv('LCMI_LBFGS_HOST', '1')
    k = 12
    x, final, st = c.fit(k)
    mof = c.batch.get_moffat()
    w = H.weights_from(c.ds)
    for f in range(c.F):
        one = PsfBatch(c.ds['data'][f:f + 1], w[f:f + 1], c.ss, ctx)
        one.set_grid(None)
        one.set_regularization(None, 0, 0)
        one.set_moffat(c.mof0[f:f + 1])
        one.set_stars(c.st0[f:f + 1])
        f1 = one.fit_moffat(k)
        assert np.array_equal(L.bits(one.get_moffat()), L.bits(mof[f:f + 1])), f
        assert np.array_equal(L.bits(one.get_stars()), L.bits(st[f:f + 1])), f
        assert np.array_equal(L.bits(f1), L.bits(final[f:f + 1])), f
        one.close()


# ---- joint form, one step ahead ------------------------------------------------------------------------------------------
class _JointTrace:
    """run_lbfgs(k) for k = 0 .. K from one start: the device's iterates, gradients, histories and evaluation counts."""

    def __init__(self, ctx, config, seed=None, off=None, K=None):
        self.config = config
        self.K = K or L.JOINT_K[config]
        self.setup = su = L.joint_setup(config, seed, off)
        self.j = j = L.joint_fit(ctx, su)
        self.lo, self.hi, self.blocks, self.free = su['lo'], su['hi'], su['blocks'], su['free']
        self.x, self.g, self.f, self.hist, self.nit, self.nev = [], [], [], [], [], []
        for k in range(self.K + 1):
            j.set_params(**su['start'])
            hist, nit, nev = j.run_lbfgs(k, su['lower'], su['upper'])
            self.x.append(self.pack(j.get_params(self.free)))
            loss, grads = j.loss_grad(self.free)
            self.g.append(self.pack(grads))
            self.f.append(np.float32(loss))
            self.hist.append(hist)
            self.nit.append(nit)
            self.nev.append(nev)

    def pack(self, d):
        return np.concatenate([np.asarray(d[k], np.float32).ravel() for k in self.free])

    def loss_at(self, x):
        self.j.set_params(**{k: x[sl] for k, sl in self.blocks.items()})
        return np.float32(self.j.loss_grad(self.free)[0])


_traces = {}


@pytest.fixture
def trace(ctx, request):
    if request.param not in _traces:
        _traces[request.param] = _JointTrace(ctx, request.param)
    return _traces[request.param]


@pytest.mark.parametrize('trace', ('bounded', 'full', 'spare'), indirect=True)
def test_joint_histories_are_prefixes_and_losses_are_the_iterates(trace):
    t = trace
    D = len(t.lo)
    assert D == (1049 if t.config == 'full' else 20)
    assert t.nit[0] == 0 and t.nev[0] == 1
    assert np.array_equal(L.bits(t.x[0]), L.bits(np.minimum(np.maximum(t.setup['x0'], t.lo), t.hi)))   # the clip of the start
    assert np.array_equal(L.bits(t.hist[0]), L.bits(np.array([t.f[0]])))
    last = t.nit[t.K]
    assert last >= min(t.K, 11), 'the fit stopped before the memory of 10 pairs was full'
    for k in range(1, t.K + 1):
        assert t.nit[k] == min(k, last) and len(t.hist[k]) == t.nit[k]
        assert np.array_equal(L.bits(t.hist[k][:t.nit[k - 1]]), L.bits(t.hist[k - 1][:t.nit[k - 1]]))
        # the loss recorded for iterate k is loss_grad at the parameters the fit left behind
        assert np.array_equal(L.bits(t.hist[k][-1:]), L.bits(np.array([t.f[k]]))), (k, t.hist[k][-1], t.f[k])
        assert t.nev[k] > t.nev[k - 1] or t.nit[k] == t.nit[k - 1]
        assert np.all(t.x[k] >= t.lo) and np.all(t.x[k] <= t.hi)


@pytest.mark.parametrize('trace', ('bounded', 'full', 'spare'), indirect=True)
def test_joint_steps_one_ahead(trace):
    t = trace
    last = t.nit[t.K]
    out = L.check_steps(L.StepTrace(t.x, t.g, t.f, t.nev, last, t.K, t.lo, t.hi, t.blocks, t.loss_at))
    print(f'joint form ({t.config}):', out)
    assert out['left_out'] <= L.ARMIJO_LEFT_OUT_MAX * out['decisions']
    if t.config == 'bounded':
        sl = t.blocks['a']
        assert (t.x[last][sl] == t.hi[sl]).sum() >= 8                             # the cap on the fluxes ends active
        assert out['held'] > 0
    if t.config == 'spare':
        # a pair failed the curvature guard while the memory was full, and the steps after it (checked above) are those of
        # the host form, which keeps its 10 pairs: the accept kernel writes into a spare slot of the ring
        assert out['lost_pairs'] >= 1 and out['steps'] == t.K
        assert out['power'] > 100      # with the oldest pair gone the steps after it would be this many tolerances away


@pytest.mark.parametrize('trace', ('stops',), indirect=True)
def test_joint_fit_that_ends_before_maxiter(trace):
    """A start so near the optimum that the fit ends on its own: the reason is one of the restatement's, the fit did not run
    on past an ftol or gtol stop, and every run with a larger maxiter leaves the same parameters and history."""
    t = trace
    last = t.nit[t.K]
    assert 0 < last < t.K
    stop = L.check_stops(L.StepTrace(t.x, t.g, t.f, t.nev, last, t.K, t.lo, t.hi, t.blocks, t.loss_at))
    print('joint form (stops):', last, 'iterations of', t.K, 'ended on', stop)
    assert stop in ('ftol', 'gtol', 'line search')
    for k in range(1, t.K + 1):
        assert t.nit[k] == min(k, last)
        assert np.array_equal(L.bits(t.hist[k]), L.bits(t.hist[min(k, last)]))
        assert np.array_equal(L.bits(t.hist[k][-1:]), L.bits(np.array([t.f[k]])))
