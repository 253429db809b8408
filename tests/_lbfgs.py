"""The bounded L-BFGS of csrc/lbfgs_host.h restated line for line in plain Python / NumPy, the analytic objectives and the
problem builders of tests/test_lbfgs_cpu.py and tests/test_lbfgs_steps_gpu.py, and every constant those tests use.

The three forms of the optimiser (csrc/lbfgs_host.h on the host in double, csrc/psf_lbfgs.h one wave per frame in double,
csrc/joint_lbfgs.h float32 vectors on the device with the decisions on the host) are one state machine; `restate` is that
state machine once more, for nb problems in lock step, with two switches: the order of the sums of its dot products
(sequential as the host loops have it, or the xor butterfly over 64 lanes of lb_wave_sum) and the type of its vector
arithmetic (float64, or float32 as the joint form has it).  No sum here goes through np.sum or np.dot: their pairwise
order is neither of the two."""
import numpy as np

# ---- constants of the algorithm (csrc/lbfgs_host.h; the joint driver in csrc/joint_fit.hip has its own stops) ------------
MEM = 10
C1 = 1e-4
MAX_LS = 25
HOST_STOPS = dict(gtol=1e-7, ftol=1e-12, tiny=1e-300)            # lbfgs_host.h, psf_lbfgs.h
JOINT_STOPS = dict(gtol=1e-6, ftol=2.2e-9, tiny=1e-30)           # lc_joint_run_lbfgs, float32

# ---- bounds of the comparisons, none fitted to the code under test ------------------------------------------------------
REASSOCIATION_MARGIN = 4.0        # the project's margin for a sum taken in another order
SCIPY_F_TOL = 1e-8                # independence of the restatement: optimum against scipy's L-BFGS-B, absolute in f
F32_EPS = 2.0 ** -24              # half a float32 ulp of 1: relative rounding error of one float32 operation
ARMIJO_NEAR = 8 * F32_EPS         # an Armijo decision closer to its threshold than this times |f| is left out
ARMIJO_LEFT_OUT_MAX = 0.05        # at most this share of the decisions may be left out
JOINT_X_ULPS = 2                  # float32 ulps of x allowed on one joint step besides the direction's own error

# cases of the host form
ROSEN_DIMS = (2, 7, 40)
ROSEN_MAXITER = (0, 1, 2, 13, 300)
# cases of the PSF form
PSF_N, PSF_F = 16, 6
PSF_SS = (1, 2)
PSF_S = (1, 5, 16)
PSF_K = (1, 2, 3, 5, 8, 11, 12, 20)
# cases of the joint form
JOINT_E, JOINT_M, JOINT_N, JOINT_SS = 5, 2, 16, 2
JOINT_K = dict(bounded=14, full=12, spare=20, stops=14)


def psf_round_budget(n_iter):
    """Rounds after which lc_psf_batch_fit_moffat's device form stops whatever the frames' states (the host form has no
    such budget)."""
    return 4 * max(1, n_iter) + 32


# ---- the two summation orders --------------------------------------------------------------------------------------------
def sum_sequential(v):
    s = v.dtype.type(0)
    for t in v:
        s = s + t
    return s


_LANES = np.arange(64)


def sum_butterfly(v):
    """lb_wave_sum: lane i holds term i (0 beyond the vector; a longer vector is folded onto the lanes in order first), then
    v += shfl_xor(v, off) for off = 32 .. 1.  Every lane ends with the same bits: the sum of two numbers commutes."""
    w = np.zeros(64, v.dtype)
    for k in range(0, len(v), 64):
        c = v[k:k + 64]
        w[:len(c)] = w[:len(c)] + c
    off = 32
    while off:
        w = w + w[_LANES ^ off]
        off >>= 1
    return w[0]


SUMS = dict(sequential=sum_sequential, butterfly=sum_butterfly)


# ---- the pieces of one iteration, usable on their own --------------------------------------------------------------------
def active_set(x, g, lo, hi):
    return ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))


def curvature_ok(sy, ss, yy):
    """The guard of the history update: sy > 1e-10 sqrt(ss yy) and sy > 0, in the type of its arguments."""
    t = type(sy)
    return bool(sy > t(1e-10) * np.sqrt(ss * yy) and sy > 0)


def _fma(a, b, c, fused):
    """a * b + c elementwise; fused: with one rounding, as a compiler may contract it.  A float32 product is exact in
    float64, so the fused float32 result is the float64 one rounded (float64 operands are left unfused)."""
    if fused and np.result_type(a, b, c) == np.float32:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return a * b + c


def direction(x, g, lo, hi, S, Y, rho, order='sequential', dtype=np.float64, fused=False):
    """-H g on the variables not held by a bound: the two-loop recursion over the pairs S[k], Y[k] (oldest first) with
    gamma from the newest pair.  Returns (d, g . d, max |projected gradient|, active set).  fused: the multiply-adds of a
    float32 run take one rounding (q -= a y, q += s c, c = a - rho dot), as the device compiler contracts them."""
    tsum = SUMS[order]
    t = np.dtype(dtype).type
    x, g, lo, hi = (np.asarray(v, dtype) for v in (x, g, lo, hi))
    act = active_set(x, g, lo, hi)
    q = np.where(act, t(0), g)
    pgmax = np.abs(q).max() if len(q) else t(0)
    m = len(S)
    S = [np.asarray(s, dtype) for s in S]
    Y = [np.asarray(y, dtype) for y in Y]
    rho = [t(r) for r in rho]
    a = [t(0)] * m
    for k in range(m - 1, -1, -1):
        a[k] = rho[k] * tsum(S[k] * q)
        q = _fma(-a[k], Y[k], q, fused)
    if m > 0:
        gamma = tsum(S[m - 1] * Y[m - 1]) / tsum(Y[m - 1] * Y[m - 1])
        q = q * gamma
    for k in range(m):
        c = _fma(-rho[k], tsum(Y[k] * q), a[k], fused)
        q = _fma(S[k], c, q, fused)
    d = np.where(act, t(0), -q)
    return d, tsum(d * g), pgmax, act


def steepest(x, g, lo, hi, order='sequential', dtype=np.float64):
    tsum = SUMS[order]
    t = np.dtype(dtype).type
    x, g, lo, hi = (np.asarray(v, dtype) for v in (x, g, lo, hi))
    d = np.where(active_set(x, g, lo, hi), t(0), -g)
    return d, tsum(d * g)


def first_alpha(d, order='sequential', tiny=1e-300):
    t = d.dtype.type
    nrm = SUMS[order](d * d)
    return min(t(1), t(1) / np.sqrt(max(nrm, t(tiny))))


# ---- the restatement -----------------------------------------------------------------------------------------------------
def restate(evalfn, x0, lo, hi, maxiter, order='sequential', dtype=np.float64, mem=MEM, gtol=1e-7, ftol=1e-12,
            tiny=1e-300):
    """lc::batched_lbfgs for nb problems in lock step.  evalfn(X [nb, D] float64) -> (F [nb], G [nb, D]).

    Returns a dict: x, f, iters, evaluations as the library returns them, and per problem the accepted iterates
    (`iterates`: the clipped start first) with their losses and gradients (`losses`, `grads`), the trials of every accepted
    iteration (`trials`), the number of pairs that failed the curvature guard (`rejected`; `rejected_full`: while the
    memory was full), of pairs dropped from a full memory (`dropped`), of steepest-descent restarts (`restarts`) and
    whether the line search failed (`ls_failed`), and the reason each problem stopped (`stop`)."""
    tsum = SUMS[order]
    t = np.dtype(dtype).type
    x = np.array(x0, dtype=dtype)
    nb, D = x.shape
    lo = np.broadcast_to(np.asarray(lo, dtype), x.shape)
    hi = np.broadcast_to(np.asarray(hi, dtype), x.shape)
    c1 = t(C1)
    x = np.minimum(np.maximum(x, lo), hi)                        # the clip of the start
    F, G = evalfn(x.astype(np.float64))
    f = np.array(F, dtype=dtype)
    g = np.array(G, dtype=dtype)
    evaluations = 1
    state = [0 if np.isfinite(f[b]) else 2 for b in range(nb)]   # 0 = needs a direction, 1 = in line search, 2 = done
    stop = ['' if s == 0 else 'nonfinite start' for s in state]
    alpha = [t(1)] * nb
    ls_count = [0] * nb
    iters = [0] * nb
    d = np.zeros_like(x)
    xt = x.copy()
    S = [[] for _ in range(nb)]
    Y = [[] for _ in range(nb)]
    RHO = [[] for _ in range(nb)]
    iterates = [[x[b].copy()] for b in range(nb)]
    losses = [[f[b]] for b in range(nb)]
    grads = [[g[b].copy()] for b in range(nb)]
    trials = [[] for _ in range(nb)]
    rejected = [0] * nb
    rejected_full = [0] * nb
    dropped = [0] * nb
    restarts = [0] * nb
    ls_failed = [False] * nb
    while True:
        anyone = False
        for b in range(nb):
            if state[b] == 2:
                continue
            if state[b] == 0:
                if iters[b] >= maxiter:
                    state[b], stop[b] = 2, 'maxiter'
                    continue
                db, gdot, pgmax, act = direction(x[b], g[b], lo[b], hi[b], S[b], Y[b], RHO[b], order, dtype)
                if pgmax < t(gtol) * max(t(1), abs(f[b])):        # the projected-gradient test
                    state[b], stop[b] = 2, 'gtol'
                    continue
                if not gdot < 0:                                  # not a descent direction: steepest-descent restart
                    S[b], Y[b], RHO[b] = [], [], []
                    restarts[b] += 1
                    db, gdot = steepest(x[b], g[b], lo[b], hi[b], order, dtype)
                d[b] = db
                alpha[b] = first_alpha(db, order, tiny) if not S[b] else t(1)
                ls_count[b] = 0
                state[b] = 1
            xt[b] = np.minimum(np.maximum(x[b] + alpha[b] * d[b], lo[b]), hi[b])
            anyone = True
        if not anyone:
            break
        for b in range(nb):
            if state[b] == 2:
                xt[b] = x[b]                                      # a finished problem is evaluated where it stopped
        FT, GT = evalfn(xt.astype(np.float64))
        ft = np.array(FT, dtype=dtype)
        gt = np.array(GT, dtype=dtype)
        evaluations += 1
        for b in range(nb):
            if state[b] != 1:
                continue
            dec = tsum(g[b] * (xt[b] - x[b]))                     # g . (projected step)
            if np.isfinite(ft[b]) and ft[b] <= f[b] + c1 * dec:
                s = xt[b] - x[b]
                y = gt[b] - g[b]
                sy, ss, yy = tsum(s * y), tsum(s * s), tsum(y * y)
                fold = f[b]
                x[b] = xt[b]
                g[b] = gt[b]
                f[b] = ft[b]
                iters[b] += 1
                iterates[b].append(x[b].copy())
                losses[b].append(f[b])
                grads[b].append(g[b].copy())
                trials[b].append(ls_count[b] + 1)
                if curvature_ok(sy, ss, yy):
                    if len(S[b]) == mem:                          # the memory is full: the oldest pair goes
                        del S[b][0], Y[b][0], RHO[b][0]
                        dropped[b] += 1
                    S[b].append(s)
                    Y[b].append(y)
                    RHO[b].append(t(1) / sy)
                else:
                    rejected[b] += 1
                    rejected_full[b] += len(S[b]) == mem
                state[b] = 0
                if abs(fold - f[b]) <= t(ftol) * max(abs(fold), abs(f[b]), t(1)):
                    state[b], stop[b] = 2, 'ftol'
            else:
                alpha[b] = alpha[b] * t(0.5)
                ls_count[b] += 1
                if ls_count[b] >= MAX_LS:                         # line search failed: the last accepted point stays
                    state[b], stop[b] = 2, 'line search'
                    ls_failed[b] = True
    return dict(x=x, f=f, iters=np.array(iters), evaluations=evaluations, iterates=iterates, losses=losses, grads=grads,
                trials=trials, rejected=rejected, rejected_full=rejected_full, dropped=dropped, restarts=restarts,
                ls_failed=ls_failed, stop=stop)


def order_difference(evalfn, x0, lo, hi, maxiter, **kw):
    """The restatement's own difference between its two summation orders on one problem: (sequential result, butterfly
    result, |x_seq - x_but| per variable, |f_seq - f_but| per problem)."""
    a = restate(evalfn, x0, lo, hi, maxiter, order='sequential', **kw)
    b = restate(evalfn, x0, lo, hi, maxiter, order='butterfly', **kw)
    return a, b, np.abs(a['x'] - b['x']), np.abs(a['f'] - b['f'])


def bits(a):
    """Raw bits of a float array, for comparisons that a NaN or a signed zero must not pass by accident."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def ulp32(v):
    """One float32 ulp at |v|, as float64."""
    v = np.abs(np.asarray(v, np.float32))
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


# ---- analytic objectives: batch_eval(fn) turns fn(x [D]) -> (f, g [D]) into the lock-step callback ------------------------
def batch_eval(fns):
    """One objective per problem (or one for all); every problem is evaluated on its own, so its bits cannot depend on its
    company."""
    def ev(X):
        X = np.asarray(X, np.float64)
        F = np.empty(len(X))
        G = np.empty_like(X)
        for b in range(len(X)):
            fn = fns[b] if isinstance(fns, (list, tuple)) else fns
            F[b], G[b] = fn(X[b])
        return F, G
    return ev


def rosenbrock(x):
    """Chained Rosenbrock, sum_i 100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2, summed in index order."""
    D = len(x)
    f = 0.0
    g = np.zeros(D)
    for i in range(D - 1):
        u = x[i + 1] - x[i] * x[i]
        v = 1.0 - x[i]
        f += 100.0 * u * u + v * v
        g[i] += -400.0 * x[i] * u - 2.0 * v
        g[i + 1] += 200.0 * u
    return f, g


def double_well(x):
    """sum_i x_i^4 / 4 - x_i^2 / 2 + 0.1 x_i x_{i+1}: concave around the origin, so a step taken there gives s . y < 0."""
    D = len(x)
    f = 0.0
    g = np.zeros(D)
    for i in range(D):
        f += 0.25 * x[i] ** 4 - 0.5 * x[i] * x[i]
        g[i] += x[i] ** 3 - x[i]
    for i in range(D - 1):
        f += 0.1 * x[i] * x[i + 1]
        g[i] += 0.1 * x[i + 1]
        g[i + 1] += 0.1 * x[i]
    return f, g


def lying_bowl(x, below=1.0):
    """sum_i (i + 1) x_i^2 whose gradient is right while the loss is above `below` and has the wrong sign under it: from
    there every trial point along -g raises the loss and all 25 halvings fail."""
    f = 0.0
    g = np.empty(len(x))
    for i, v in enumerate(x):
        f += (i + 1) * v * v
        g[i] = 2.0 * (i + 1) * v
    return f, (g if f > below else -g)


def walled(fn, wall=10.0):
    """fn with an infinite loss where x_0 > wall (the gradient there is NaN: nothing may read it)."""
    def w(x):
        if x[0] > wall:
            return np.inf, np.full(len(x), np.nan)
        return fn(x)
    return w


# ---- problem builders ----------------------------------------------------------------------------------------------------
def rosenbrock_problems(D):
    """Four Rosenbrock problems in lock step: 0 ends on an upper bound, 1 on a lower bound, 2 is unbounded, 3 starts outside
    its box.  Returns x0, lo, hi [4, D]."""
    rng = np.random.default_rng(100 + D)
    x0 = rng.uniform(-1.2, 1.2, (4, D))
    lo = np.full((4, D), -np.inf)
    hi = np.full((4, D), np.inf)
    hi[0, 0] = 0.5                       # the optimum has x_0 = 1: this bound ends active
    x0[0, 0] = min(x0[0, 0], 0.3)
    lo[1, D - 1] = 1.5                   # the optimum has x_{D-1} = 1
    x0[1, D - 1] = 2.0
    lo[3], hi[3] = -2.0, 2.0
    x0[3, 0], x0[3, D - 1] = 3.5, -4.0   # outside: the start is clipped
    return x0, lo, hi


def double_well_problem(D=6):
    x0 = np.full((1, D), 0.1) * (1 + 0.1 * np.arange(D))
    return x0, np.full((1, D), -np.inf), np.full((1, D), np.inf)


def lying_problem(D=5):
    x0 = np.linspace(1.5, 3.0, D)[None, :].copy()
    return x0, np.full((1, D), -np.inf), np.full((1, D), np.inf)


# ---- the PSF form: lc_psf_batch_fit_moffat driven through set_moffat / set_stars / evaluate -------------------------------
def psf_pack(moffat, stars):
    """[F][4], [F][S][4] -> x [F][D] in the optimiser's order: Moffat (4) | a (S) | x0 (S) | y0 (S)."""
    F, S = stars.shape[:2]
    return np.concatenate([np.asarray(moffat, np.float64).reshape(F, 4)] +
                          [np.asarray(stars[..., c], np.float64).reshape(F, S) for c in range(3)], axis=1)


def psf_unpack(X, sky):
    """x [F][D] -> float32 parameter blocks, rounded as the step kernel rounds them; the sky column is `sky`."""
    F, S = sky.shape
    X = np.asarray(X)
    mof = X[:, :4].astype(np.float32)
    st = np.empty((F, S, 4), np.float32)
    for c in range(3):
        st[..., c] = X[:, 4 + c * S:4 + (c + 1) * S].astype(np.float32)
    st[..., 3] = sky
    return mof, st


def psf_bounds(F, S, n, ss):
    D = 4 + 3 * S
    lo = np.empty((F, D))
    hi = np.empty((F, D))
    lo[:, 0:2], hi[:, 0:2] = 0.5 / ss, n / 2.0
    lo[:, 2], hi[:, 2] = -np.pi, np.pi
    lo[:, 3], hi[:, 3] = 1.1, 50.0
    lo[:, 4:4 + S], hi[:, 4:4 + S] = 0.0, np.inf
    lo[:, 4 + S:], hi[:, 4 + S:] = -n / 4.0, n / 4.0
    return lo, hi


def psf_eval(batch, sky):
    """The lock-step callback of a PsfBatch: the parameters go up rounded to float32, loss and gradients come back as the
    float32 the kernels wrote."""
    S = sky.shape[1]

    def ev(X):
        mof, st = psf_unpack(X, sky)
        batch.set_moffat(mof)
        batch.set_stars(st)
        out = batch.evaluate()
        G = np.concatenate([out['grad_moffat'].astype(np.float64)] +
                           [out['grad_stars'][..., c].astype(np.float64).reshape(-1, S) for c in range(3)], axis=1)
        return out['loss'].astype(np.float64), G
    return ev


def psf_problem(S, ss, seed=0):
    """make_psf_dataset at n = 16 with F = 6 frames, and a start per frame: the frames lie at different distances from the
    optimum (they finish in different rounds), frame 1 starts with beta and one x0 outside their bounds, and frame 2 has a
    seeing so wide that its FWHM bound n / 2 ends active.  Returns (dataset, moffat [F][4], stars [F][S][4])."""
    from lightcurver_amd.synthetic import make_psf_dataset
    from tests import helpers as H
    n, F = PSF_N, PSF_F
    ds = make_psf_dataset(F=F, S=S, n=n, ss=ss, seed=700 + 10 * S + ss + seed)
    v = np.arange(n) - (n - 1) / 2.0
    wide = np.exp(-0.5 * (v[:, None] ** 2 + v[None, :] ** 2) / 6.0 ** 2)   # FWHM 14 px: beyond the bound n / 2 of the Moffat's
    data = ds['data'].copy()
    data[2] = data[2].sum(axis=(-1, -2), keepdims=True) * (wide / wide.sum()).astype(data.dtype)
    ds['data'] = data
    plist = [H.psf_initial_params(ds, f, ss) for f in range(F)]
    mof = H.moffat_array(plist).astype(np.float32)
    st = H.stars_array(plist).astype(np.float32)
    st[..., 3] = np.float32(1e-4) * np.arange(1, S + 1, dtype=np.float32)   # a sky the fit must leave alone
    for f in range(F):
        st[f, :, 0] *= np.float32(1.0 - 0.06 * f)                # frame 0 starts nearest, frame 5 farthest
        mof[f, :2] *= np.float32(1.0 + 0.08 * f)
    mof[1, 3] = 60.0                                             # beta above its bound 50
    st[1, 0, 1] = 0.3 * n                                        # x0 beyond n / 4
    return ds, mof, st


# ---- the joint form: lc_joint_run_lbfgs one step ahead --------------------------------------------------------------------
JOINT_ORDER = ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha', 'h', 'mean')     # the order of the blocks in the optimiser's vector
# seeds and start offsets (px, 1 sigma) chosen on the oracle's float64 loss (tests/test_lbfgs_cpu.py): the whole ladder runs
# ('stops': ends on ftol) and no Armijo decision lies nearer its threshold than ARMIJO_NEAR |f|
JOINT_SEEDS = dict(bounded=76, full=73, spare=85, stops=71)
JOINT_OFF = dict(bounded=1.0, full=0.3, spare=2.0, stops=0.3)
JOINT_LAMBDAS = dict(lam_scales=1.0, lam_hf=1.0, lam_positivity=10.0)   # the regulariser of the configuration 'full'


def joint_setup(config, seed=None, off=None):
    """make_roi_dataset at E = 5, M = 2, n = 16, ss = 2 with a start `off` px (1 sigma) from the truth.  config 'bounded': a,
    dx, dy free (D = 20), a cap on the fluxes below their optimum and a lower bound on one dx; 'full': a, dx, dy, h, mean
    free (D = 1049), unbounded, the regulariser on with a propagated W; 'spare': 'bounded' from a start 2 px off, whose
    trajectory meets a pair that fails the curvature guard while the memory is full; 'stops': 'bounded' from a start so
    near that the fit ends on ftol before maxiter (only its stops are checked: its last steps are at the rounding floor).
    Returns a dict: ds, start, free, lower, upper, and
    the flat float32 vectors x0, lo, hi with the blocks {name: slice} they are made of."""
    from lightcurver_amd.synthetic import make_roi_dataset
    E, M, n, ss = JOINT_E, JOINT_M, JOINT_N, JOINT_SS
    seed = JOINT_SEEDS[config] if seed is None else seed
    off = JOINT_OFF[config] if off is None else off
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=seed)
    rng = np.random.default_rng(seed + 1)
    p = {k: np.array(v, dtype=np.float64).ravel() for k, v in ds['truth'].items()}
    p['a'] = p['a'] * rng.uniform(0.7, 1.3, p['a'].shape)
    p['dx'] = p['dx'] + rng.normal(0, off, E)
    p['dy'] = p['dy'] + rng.normal(0, off, E)
    if config in ('bounded', 'spare', 'stops'):
        free = ['a', 'dx', 'dy']
        lower = dict(a=np.zeros(E * M), dx=np.full(E, -n / 2.0))
        upper = dict(a=0.8 * np.asarray(ds['truth']['a'], np.float64).ravel())
        lower['dx'][1] = p['dx'][1] - 0.02
    else:
        free = ['a', 'dx', 'dy', 'h', 'mean']
        lower = upper = None
    free = [k for k in JOINT_ORDER if k in free]
    blocks, o = {}, 0
    for k in free:
        blocks[k] = slice(o, o + p[k].size)
        o += p[k].size
    x0 = np.concatenate([p[k].astype(np.float32) for k in free])
    lo = np.full(o, -np.inf, np.float32)
    hi = np.full(o, np.inf, np.float32)
    for k, sl in blocks.items():
        if lower and k in lower:
            lo[sl] = lower[k].astype(np.float32)
        if upper and k in upper:
            hi[sl] = upper[k].astype(np.float32)
    return dict(config=config, ds=ds, start=p, free=free, lower=lower, upper=upper, blocks=blocks, x0=x0, lo=lo, hi=hi)


def joint_fit(ctx, setup):
    """The JointFit of a joint_setup, at its start, loss and free blocks set."""
    from lightcurver_amd.joint import JointFit
    ds = setup['ds']
    j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], JOINT_SS, JOINT_M, ctx)
    j.set_params(**setup['start'])
    if setup['config'] == 'full':
        j.set_loss(W=j.propagate_noise(), **JOINT_LAMBDAS)
    else:
        j.set_loss()
    j.set_free(setup['free'])
    return j


def joint_oracle_eval(setup):
    """The lock-step callback (one problem) of a joint_setup on the oracle's float64 loss."""
    from oracle import model as om, optim as oo
    ds, blocks = setup['ds'], setup['blocks']
    data, sig2, psf = om.T(ds['data']), om.T(ds['noisemap']) ** 2, om.T(ds['psf'])
    kw = {}
    if setup['config'] == 'full':
        kw = dict(W=om.propagate_noise_deconv(sig2, psf, JOINT_SS), lam_scales=JOINT_LAMBDAS['lam_scales'],
                  lam_hf=JOINT_LAMBDAS['lam_hf'], lam_pos=JOINT_LAMBDAS['lam_positivity'])
    base = {k: om.T(np.asarray(v, np.float64)) for k, v in setup['start'].items()}

    def ev(X):
        p = dict(base)
        for k, sl in blocks.items():
            p[k] = om.T(np.asarray(X[0][sl], np.float64).reshape(tuple(base[k].shape)))
        f, g = oo.value_and_grad(lambda q: om.deconv_loss(q, data, sig2, psf, JOINT_SS, **kw), p, setup['free'])
        return np.array([f]), np.concatenate([g[k].numpy().ravel() for k in setup['free']])[None, :]
    return ev


def trace_of_restatement(evalfn, x0, lo, hi, K, blocks):
    """The StepTrace that a fit which IS the float32 restatement (with the joint driver's stops) leaves behind."""
    r = restate(evalfn, x0[None, :], lo[None, :], hi[None, :], K, order='butterfly', dtype=np.float32, **JOINT_STOPS)
    x, g, f = r['iterates'][0], r['grads'][0], r['losses'][0]
    last = len(x) - 1
    nev = list(np.cumsum([1] + r['trials'][0]))
    if r['ls_failed'][0]:
        nev.append(nev[-1] + MAX_LS)
    pad = K - last
    x, g, f = x + [x[-1]] * pad, g + [g[-1]] * pad, f + [f[-1]] * pad
    nev = nev[:last + 1] + [nev[-1]] * pad

    def loss_at(v):
        return np.float32(evalfn(np.asarray(v, np.float64)[None, :])[0][0])
    return StepTrace(x, g, f, nev, last, K, lo, hi, blocks, loss_at), r


class StepTrace:
    """What lc_joint_run_lbfgs leaves behind when it is run with maxiter 0 .. K from one start: iterates x[k] and gradients
    g[k] there (float32), losses f[k] (float32), evaluation counts nev[k], the iterations it did in all (`last`), bounds,
    the blocks {name: slice} of the variables, and loss_at(x) for the loss at any other point."""

    def __init__(self, x, g, f, nev, last, K, lo, hi, blocks, loss_at):
        self.x, self.g, self.f, self.nev, self.last, self.K = x, g, f, nev, last, K
        self.lo, self.hi, self.blocks, self.loss_at = lo, hi, blocks, loss_at


def check_stops(t):
    """The stops of a StepTrace are those of the restatement, in the float32 of the joint driver: the fit went on from
    iterate k only where neither gtol nor ftol stops it there, and where it ended before maxiter it ended on ftol, on gtol
    or on a line search that failed, the parameters then being those of the last accepted point.  Returns the reason."""
    gtol, ftol = np.float32(JOINT_STOPS['gtol']), np.float32(JOINT_STOPS['ftol'])
    one = np.float32(1)

    def by_gtol(k):
        pg = direction(t.x[k], t.g[k], t.lo, t.hi, [], [], [], 'sequential', np.float32)[2]
        return bool(pg < gtol * max(one, abs(np.float32(t.f[k]))))

    def by_ftol(k):
        f0, f1 = np.float32(t.f[k - 1]), np.float32(t.f[k])
        return k > 0 and bool(abs(f0 - f1) <= ftol * max(abs(f0), abs(f1), one))
    for k in range(t.last):
        assert not by_gtol(k), ('the fit went on where gtol stops it', k)
        assert not by_ftol(k), ('the fit went on where ftol stops it', k)
    if t.last == t.K:
        return 'maxiter'
    ls = t.nev[t.K] - t.nev[t.last] == MAX_LS
    assert t.nev[t.K] - t.nev[t.last] in (0, MAX_LS)
    stop = 'ftol' if by_ftol(t.last) else 'gtol' if by_gtol(t.last) else 'line search' if ls else None
    assert stop is not None, ('stopped early for no reason of the algorithm', t.last, t.f[t.last])
    # every longer run stops at the same iterate and leaves its parameters (after a failed line search: the last accepted point)
    for k in range(t.last, t.K + 1):
        assert np.array_equal(bits(t.x[k]), bits(t.x[t.last])), k
    return stop


def check_steps(t):
    """Every step x[k] -> x[k + 1] of a StepTrace against the restatement's direction from the trace's own pairs, so that no
    error is carried over from earlier steps; see tests/test_lbfgs_steps_gpu.py.  Returns the figures it measured."""
    S, Y, RHO, RHO32 = [], [], [], []        # rho = 1 / (s . y) is not left behind: each restatement sums its own
    decisions = left_out = lost_pairs = rejected_pairs = held = 0
    worst = worst_var = power = 0.0
    left_out_at, lost_at = [], []
    S9 = None                                # the pairs as a ring without the spare slot would hold them after a lost pair
    one = np.float32(1)
    for k in range(t.last):
        x, g, f = t.x[k], t.g[k], np.float64(t.f[k])
        d64, gd64, _, act = direction(x, g, t.lo, t.hi, S, Y, RHO, 'sequential', np.float64)
        d32, _, _, _ = direction(x, g, t.lo, t.hi, S, Y, RHO32, 'butterfly', np.float32)
        d32f = direction(x, g, t.lo, t.hi, S, Y, RHO32, 'butterfly', np.float32, fused=True)[0]
        m = len(S)
        if not gd64 < 0:
            d64, gd64 = steepest(x, g, t.lo, t.hi, 'sequential', np.float64)
            d32, _ = steepest(x, g, t.lo, t.hi, 'butterfly', np.float32)
            d32f = d32
            S, Y, RHO, RHO32, m = [], [], [], [], 0
        assert gd64 < 0, k
        alpha0 = 1.0 if m else float(first_alpha(d64, 'sequential', JOINT_STOPS['tiny']))
        alpha0_32 = one if m else first_alpha(d32, 'butterfly', JOINT_STOPS['tiny'])
        nb = t.nev[k + 1] - t.nev[k] - 1
        assert 0 <= nb < MAX_LS, (k, nb)
        alpha = alpha0 * 0.5 ** nb
        x64, xn = x.astype(np.float64), t.x[k + 1].astype(np.float64)
        want = np.minimum(np.maximum(x64 + alpha * d64, t.lo), t.hi)
        # The float32 step alpha d of the restatement against its float64 one (alpha is a float32 result too where it is
        # 1 / |d|).  Within a block the variables have one scale: one float32 realisation samples the rounding error per
        # variable and bounds it per block.  The ulps are those of x where it is largest on the step, x_k or x_k+1: the
        # sum x + alpha d is rounded at that size where the two nearly cancel.
        # The float32 restatement comes in the two forms a compiler may give it, multiply-adds fused or not.
        a32 = alpha0_32 * np.float32(0.5 ** nb)
        derr = np.zeros(len(x))
        for sl in t.blocks.values():
            derr[sl] = max(np.abs((a32 * d[sl]).astype(np.float64) - alpha * d64[sl]).max() for d in (d32, d32f))
        tol = np.maximum(JOINT_X_ULPS * ulp32(np.maximum(np.abs(x64), np.abs(xn))), REASSOCIATION_MARGIN * derr)
        diff = np.abs(xn - want)
        worst = max(worst, float((diff / tol).max()))
        # reported, not asserted: the bound read per variable, from the unfused float32 direction alone and the ulps of the
        # point aimed at (one float32 realisation is a sample of a variable's rounding error, not a bound on it).  MI355X:
        # 2.96, 12.1 and 1.44 for 'bounded', 'full' and 'spare', where the asserted ratio is 0.25, 0.55 and 0.37.
        tol_var = np.maximum(JOINT_X_ULPS * ulp32(want),
                             REASSOCIATION_MARGIN * np.abs((a32 * d32).astype(np.float64) - alpha * d64))
        worst_var = max(worst_var, float((diff / tol_var).max()))
        if S9 is not None and m:
            # what this step would be had the failed pair been written over the oldest one: the check must tell the two apart
            d9 = direction(x, g, t.lo, t.hi, S9[0], S9[1], S9[2], 'sequential', np.float64)[0]
            power = max(power, float((np.abs(np.minimum(np.maximum(x64 + alpha * d9, t.lo), t.hi) - want) / tol).max()))
        assert np.all(diff <= tol), ('step', k, 'alpha', alpha, 'variables', np.flatnonzero(diff > tol)[:8],
                                     'worst ratio', (diff / tol).max())
        # a variable held by its bound does not move
        held += int(act.sum())
        assert np.array_equal(bits(t.x[k + 1][act]), bits(x[act])), k
        # Armijo at the fit's own losses: the accepted trial satisfies it, every rejected one violates it
        near = ARMIJO_NEAR * abs(f)
        margin = f + C1 * float(sum_sequential(g.astype(np.float64) * (xn - x64))) - np.float64(t.f[k + 1])
        decisions += 1
        if abs(margin) < near:
            left_out += 1
            left_out_at.append(k)
        else:
            assert margin > 0, ('accepted step violates Armijo', k, margin)
        for b in range(nb):
            xt = np.minimum(np.maximum(x64 + alpha0 * 0.5 ** b * d64, t.lo), t.hi).astype(np.float32)
            ft = np.float64(t.loss_at(xt))
            margin = f + C1 * float(sum_sequential(g.astype(np.float64) * (xt.astype(np.float64) - x64))) - ft
            decisions += 1
            if np.isfinite(ft) and abs(margin) < near:
                left_out += 1
                left_out_at.append(k)
            else:
                assert not (np.isfinite(ft) and margin >= 0), ('rejected trial satisfies Armijo', k, b, margin)
        # the fit's own pair, in float32 as lb_accept_kernel forms it; the guard; the 10 newest
        s = t.x[k + 1] - x
        y = t.g[k + 1] - g
        s64, y64 = s.astype(np.float64), y.astype(np.float64)
        sy, ss, yy = (sum_sequential(v) for v in (s64 * y64, s64 * s64, y64 * y64))
        if curvature_ok(sy, ss, yy):
            if len(S) == MEM:
                del S[0], Y[0], RHO[0], RHO32[0]
            S.append(s)
            Y.append(y)
            RHO.append(1.0 / sy)
            RHO32.append(one / sum_butterfly(s * y))
            if S9 is not None:
                S9 = [S9[0][-(MEM - 1):] + [s], S9[1][-(MEM - 1):] + [y], S9[2][-(MEM - 1):] + [1.0 / sy]]
        else:
            rejected_pairs += 1
            if len(S) == MEM:                # the memory is full and stays as it is: the pair went into the ring's spare slot
                lost_pairs += 1
                lost_at.append(k)
                S9 = [S[1:], Y[1:], RHO[1:]] if S9 is None else [S9[0][1:], S9[1][1:], S9[2][1:]]
    stop = check_stops(t)
    return dict(steps=t.last, worst=worst, worst_per_variable=worst_var, decisions=decisions, left_out=left_out,
                lost_pairs=lost_pairs, rejected_pairs=rejected_pairs, held=held, stop=stop, left_out_at=left_out_at,
                lost_at=lost_at, power=power)
