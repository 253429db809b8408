"""NumPy restatement of the difference-imaging SPEC (DESIGN.md §5 "Difference imaging"), the scenes and the cases of
tests/test_diffim_cpu.py and tests/test_diffim_gpu.py.

``fit_region`` builds the design matrix of one region and solves it two ways in float64 (``numpy.linalg.lstsq`` and
Cholesky of the normal equations); ``gram`` sums the normal equations with exact products and long-double sums;
``difference`` evaluates D in float64 or in float32 in the SPEC's order; ``subtract`` runs the rounds of one frame."""
import functools

import numpy as np

STATUS_OK, STATUS_FEW, STATUS_PIVOT = 0, 1, 2
C_BOUND = 32.0   # diff: next power of two >= 4 x the float32 restatement's worst ratio (test_diffim_cpu.py measures it)


def n_background(bg_degree):
    return {0: 1, 1: 3, 2: 6}[bg_degree]


def regions_of(shape, regions):
    """[(i0, i1, j0, j1)] row-major over the gy x gx grid."""
    (H, W), (gy, gx) = shape, regions
    return [(i * H // gy, (i + 1) * H // gy, j * W // gx, (j + 1) * W // gx) for i in range(gy) for j in range(gx)]


def coordinate(i, i0, i1):
    """X or Y of the SPEC, in double."""
    return (2.0 * np.asarray(i, np.float64) - (i0 + i1 - 1)) / max(i1 - i0 - 1, 1)


def footprint_finite(R, r):
    """True where every reference pixel of the footprint is finite; False within r pixels of the border."""
    H, W = R.shape
    fin = np.isfinite(R)
    ok = np.zeros((H, W), bool)
    ok[r:H - r, r:W - r] = True
    for v in range(-r, r + 1):
        for u in range(-r, r + 1):
            ok[r:H - r, r:W - r] &= fin[r - v:H - r - v, r - u:W - r - u]
    return ok


def base_set(T, R, r, var=None, mask=None):
    """The fit set of round 0 over the whole image."""
    ok = footprint_finite(R, r) & np.isfinite(T)
    if var is not None:
        with np.errstate(invalid='ignore'):
            ok &= np.isfinite(var) & (var > 0)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    return ok


def design(R, r, bg_degree, region, rows, cols, dtype=np.float64):
    """The design vectors of the pixels (rows, cols) of ``region``: reference samples in the order m = (v + r)(2 r + 1) +
    (u + r), a_m = R(i - v, j - u), then the background terms 1, X, Y, X^2, XY, Y^2."""
    i0, i1, j0, j1 = region
    Rd = np.asarray(R, dtype)
    A = [Rd[rows - v, cols - u] for v in range(-r, r + 1) for u in range(-r, r + 1)]
    X, Y = coordinate(cols, j0, j1).astype(dtype), coordinate(rows, i0, i1).astype(dtype)
    A += [np.ones(len(rows), dtype), X, Y, X * X, X * Y, Y * Y][:n_background(bg_degree)]
    return np.stack(A, axis=1)


def cholesky_solve(U, b):
    """(x, status) by Cholesky in float64, no regularisation."""
    P = len(b)
    L = np.zeros((P, P))
    for i in range(P):
        s = U[i, i] - L[i, :i] @ L[i, :i]
        if not (s > 0 and np.isfinite(s)):
            return np.full(P, np.nan), STATUS_PIVOT
        L[i, i] = np.sqrt(s)
        L[i + 1:, i] = (U[i + 1:, i] - L[i + 1:, :i] @ L[i, :i]) / L[i, i]
    y = np.zeros(P)
    for i in range(P):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(P)
    for i in range(P - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return (x, STATUS_OK) if np.isfinite(x).all() else (np.full(P, np.nan), STATUS_PIVOT)


def fit_region(T, R, r, bg_degree, region, used, var=None):
    """The fit of one region over the pixels ``used`` (bool image): dict(A, t, w, n, status, x (Cholesky of the normal
    equations), x_lstsq, U, b), all float64."""
    i0, i1, j0, j1 = region
    sel = np.zeros_like(used)
    sel[i0:i1, j0:j1] = used[i0:i1, j0:j1]
    rows, cols = np.nonzero(sel)
    A = design(R, r, bg_degree, region, rows, cols)
    t = np.asarray(T, np.float64)[rows, cols]
    w = np.ones(len(rows)) if var is None else 1.0 / np.asarray(var, np.float64)[rows, cols]
    P = A.shape[1]
    out = dict(A=A, t=t, w=w, n=len(rows), rows=rows, cols=cols, U=(A * w[:, None]).T @ A, b=(A * w[:, None]).T @ t)
    if len(rows) < 2 * P:
        out.update(status=STATUS_FEW, x=np.full(P, np.nan), x_lstsq=np.full(P, np.nan))
        return out
    x, status = cholesky_solve(out['U'], out['b'])
    sw = np.sqrt(w)
    out.update(status=status, x=x, x_lstsq=np.linalg.lstsq(A * sw[:, None], t * sw, rcond=None)[0])
    return out


def gram(A, w, t):
    """(U, b, Uabs, babs): the normal equations with every product and sum in long double (the products of float32
    values are exact in double already), rounded to double at the end; and sum w |a_m| |a_n|, sum w |a_m| |t|."""
    Al = A.astype(np.longdouble)
    wa = Al * np.asarray(w, np.longdouble)[:, None]
    P = A.shape[1]
    U = np.empty((P, P))
    step = max(1, -(-P // 8))                       # the lower triangle in column blocks, mirrored: U is symmetric
    for c0 in range(0, P, step):
        U[c0:, c0:c0 + step] = (wa[:, c0:].T @ Al[:, c0:c0 + step]).astype(np.float64)
        U[c0:c0 + step, c0:] = U[c0:, c0:c0 + step].T
    b = (wa.T @ np.asarray(t, np.longdouble)).astype(np.float64)
    Aa = np.abs(A) * np.asarray(w)[:, None]
    return U, b, Aa.T @ np.abs(A), Aa.T @ np.abs(t)


def difference(T, R, r, bg_degree, region, x, dtype):
    """(D, magnitude) over the region's rectangle, NaN by the SPEC's rule.  float64: plain double arithmetic with the
    coefficients as they are.  float32: the coefficients rounded to float32 and the SPEC's order: m = 0; m += K[m] R in
    the order of m; bg = c0 (+ c1 X, + c2 Y (+ c3 (X X), + c4 (X Y), + c5 (Y Y))) with X, Y rounded from double; M = m +
    bg; D = T - M.  magnitude = sum |K_m| |R| + |bg| + |T|, in double."""
    i0, i1, j0, j1 = region
    H, W = R.shape
    D = np.full((i1 - i0, j1 - j0), np.nan, dtype)
    mag = np.full((i1 - i0, j1 - j0), np.nan)
    ok = (footprint_finite(R, r) & np.isfinite(T))[i0:i1, j0:j1]
    if not np.isfinite(x).all() or not ok.any():
        return D, mag
    rr, cc = np.nonzero(ok)
    rows, cols = rr + i0, cc + j0
    nk = (2 * r + 1) ** 2
    coef = np.asarray(x, np.float64).astype(dtype)
    Rd = np.asarray(R, dtype)
    m = np.zeros(len(rows), dtype)
    ma = np.zeros(len(rows))
    e = 0
    for v in range(-r, r + 1):
        for u in range(-r, r + 1):
            s = Rd[rows - v, cols - u]
            m = m + coef[e] * s
            ma += np.abs(float(coef[e])) * np.abs(s.astype(np.float64))
            e += 1
    X, Y = coordinate(cols, j0, j1).astype(dtype), coordinate(rows, i0, i1).astype(dtype)
    terms = [None, X, Y, X * X, X * Y, Y * Y][:n_background(bg_degree)]
    bg = np.full(len(rows), coef[nk], dtype)
    for c, term in zip(coef[nk + 1:], terms[1:]):
        bg = bg + c * term
    t = np.asarray(T, dtype)[rows, cols]
    D[rr, cc] = t - (m + bg)
    mag[rr, cc] = ma + np.abs(bg.astype(np.float64)) + np.abs(t.astype(np.float64))
    return D, mag


def subtract(T, R, r, bg_degree=1, regions=(1, 1), clip_iters=2, n_sigma=4.0, var=None, mask=None, sigma=None,
             check_margin=False):
    """The rounds of one frame.  Returns dict(diff64, diff32, magnitude (H, W); kernel (G, 2r+1, 2r+1), bg (G, 6), scale,
    n_used, chi2, chi2_slack, status (G,); fits: the last ``fit_region`` of every region; used: the last fit set; margins: per
    round > 0 the worst |D| / threshold among the kept and the least among the clipped pixels).  check_margin: asserts
    that no pixel of a clipping round lies between 0.5 and 20 thresholds."""
    T, R = np.asarray(T, np.float32), np.asarray(R, np.float32)
    H, W = T.shape
    regs = regions_of((H, W), regions)
    G, nk, nb = len(regs), (2 * r + 1) ** 2, n_background(bg_degree)
    P = nk + nb
    base = base_set(T, R, r, var, mask)
    status = np.zeros(G, np.int32)
    n_used = np.zeros(G, np.int32)
    D64 = np.full((H, W), np.nan)
    D32 = np.full((H, W), np.nan, np.float32)
    mag = np.full((H, W), np.nan)
    fits = [None] * G
    used = np.zeros((H, W), bool)
    rms = np.full(G, np.nan)
    xs = np.full((G, P), np.nan)
    margins = []
    for rnd in range(clip_iters + 1):
        for g, reg in enumerate(regs):
            if status[g] != 0:
                continue
            i0, i1, j0, j1 = reg
            sub = (slice(i0, i1), slice(j0, j1))
            take = base[sub].copy()
            if rnd > 0:
                if var is not None:
                    sg = np.sqrt(np.asarray(var, np.float32)[sub]).astype(np.float64)
                else:
                    sg = np.full(take.shape, float(np.float32(sigma)) if sigma is not None else float(np.float32(rms[g])))
                thr = float(np.float32(n_sigma)) * sg
                with np.errstate(invalid='ignore', divide='ignore'):
                    ratio = np.abs(D64[sub]) / thr
                    keep = ratio <= 1.0
                if check_margin:
                    rb = ratio[take]
                    assert not ((rb >= 0.5) & (rb < 20.0)).any(), (rnd, g, rb[(rb >= 0.5) & (rb < 20.0)])
                    margins.append((rnd, g, float(rb[rb < 0.5].max(initial=0.0)), float(rb[rb >= 20.0].min(initial=np.inf))))
                take &= keep
            used[sub] = take
            f = fit_region(T, R, r, bg_degree, reg, used, var)
            fits[g], n_used[g], status[g], xs[g] = f, f['n'], f['status'], f['x']
            D64[sub], mag[sub] = difference(T, R, r, bg_degree, reg, f['x'], np.float64)
            D32[sub] = difference(T, R, r, bg_degree, reg, f['x'], np.float32)[0]
            if f['status'] == 0:
                rms[g] = np.sqrt((D64[sub][take] ** 2).sum() / f['n'])
    chi2, slack = np.full(G, np.nan), np.zeros(G)
    for g, (i0, i1, j0, j1) in enumerate(regs):
        if status[g] != 0:
            continue
        sub = (slice(i0, i1), slice(j0, j1))
        d2 = D64[sub][used[sub]] ** 2
        s2 = np.asarray(var, np.float64)[sub][used[sub]] if var is not None else \
            (float(np.float32(sigma)) ** 2 if sigma is not None else d2.sum() / n_used[g])
        chi2[g] = (d2 / s2).sum() / (n_used[g] - P)
        # what errors of D within diff_bound can change of it: sum (2 |D| b + b^2) / sigma^2 over the same pixels
        b = diff_bound(mag[sub][used[sub]])
        slack[g] = 0.0 if var is None and sigma is None else ((2.0 * np.sqrt(d2) * b + b * b) / s2).sum() / (n_used[g] - P)
    bg = np.zeros((G, 6))
    bg[:, :nb] = xs[:, nk:]
    bg[status != 0] = np.nan
    kernel = xs[:, :nk].reshape(G, 2 * r + 1, 2 * r + 1)
    return dict(diff64=D64, diff32=D32, magnitude=mag, kernel=kernel, bg=bg, scale=kernel.reshape(G, -1).sum(axis=1),
                n_used=n_used, chi2=chi2, chi2_slack=slack, status=status, fits=fits, used=used, margins=margins)


def diff_bound(magnitude):
    return C_BOUND * 2.0 ** -24 * magnitude


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def true_kernel():
    """5 x 5, asymmetric: an off-centre elliptical Gaussian with one negative lobe, sum 0.8."""
    y, x = np.mgrid[-2:3, -2:3].astype(np.float64)
    k = np.exp(-0.5 * (((x - 0.3) / 0.9) ** 2 + ((y + 0.2) / 0.6) ** 2 + 0.5 * (x - 0.3) * (y + 0.2)))
    k[0, 3] -= 0.15 * k.max()
    return k * (0.8 / k.sum())


def star_field(shape, seed, n_stars=12, noise=0.0):
    """About n_stars Gaussian stars of different widths on a zero sky, float32; ``noise``: the rms of white noise."""
    H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros(shape)
    for _ in range(n_stars):
        cx, cy = rng.uniform(3, W - 4), rng.uniform(3, H - 4)
        s = rng.uniform(0.9, 2.2)
        img += rng.uniform(200.0, 2000.0) * np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / s ** 2)
    if noise:
        img += noise * rng.standard_normal(shape)
    return img.astype(np.float32)


def convolve_same(R, K):
    """scipy.signal.convolve2d(R, K, mode='same') for an odd kernel, in float64."""
    r = K.shape[0] // 2
    H, W = R.shape
    pad = np.zeros((H + 2 * r, W + 2 * r))
    pad[r:r + H, r:r + W] = R
    out = np.zeros((H, W))
    for v in range(-r, r + 1):
        for u in range(-r, r + 1):
            out += K[v + r, u + r] * pad[r - v:r - v + H, r - u:r - u + W]
    return out


def plane(shape, c0, cx, cy):
    H, W = shape
    return c0 + cx * coordinate(np.arange(W), 0, W)[None, :] + cy * coordinate(np.arange(H), 0, H)[:, None]


@functools.lru_cache(maxsize=None)
def known_kernel_scene():
    """Noise-free T = R (*) K_true + plane on 48 x 40: the well-conditioned known-kernel case."""
    shape = (48, 40)
    R = star_field(shape, 11, noise=2.0)
    K = true_kernel()
    T = (convolve_same(R.astype(np.float64), K) + plane(shape, 3.0, 1.5, -0.7)).astype(np.float32)
    return dict(R=R, T=T, K=K, plane=(3.0, 1.5, -0.7))


SIGMA = 1.0        # the declared pixel noise of the cases
NOISE = 0.1        # the injected noise: uniform in +- NOISE sigma, so that no kept pixel comes near a clipping threshold
OUTLIER = 85.0     # injected outliers, in sigma: >= 20 n_sigma sigma at n_sigma = 4

# shape, r, bg_degree, regions, K, var, sigma, mask, nan_T, nan_R, clip_iters, n_sigma
CASES = {
    'plain':        dict(shape=(40, 48), r=2, bg=1, regions=(1, 1), K=1, clip=0),
    'small':        dict(shape=(17, 19), r=1, bg=0, regions=(1, 1), K=3, clip=0, nan_T=True),
    'small_r3':     dict(shape=(17, 19), r=3, bg=0, regions=(1, 1), K=1, clip=0, sigma=True),
    'var_clip':     dict(shape=(40, 48), r=2, bg=2, regions=(1, 1), K=3, clip=2, var=True, mask=True, nan_R=True),
    'sigma_clip':   dict(shape=(40, 48), r=3, bg=1, regions=(1, 1), K=1, clip=2, sigma=True, nan_T=True),
    'regions':      dict(shape=(40, 48), r=1, bg=1, regions=(2, 3), K=3, clip=2, sigma=True, mask=True, nan_R=True),
    'regions_fail': dict(shape=(40, 48), r=3, bg=2, regions=(2, 3), K=1, clip=0, sigma=True, mask=True, fail=True),
    'prime':        dict(shape=(67, 131), r=3, bg=1, regions=(2, 3), K=1, clip=2, var=True, nan_T=True, nan_R=True),
    'prime_r7':     dict(shape=(67, 131), r=7, bg=1, regions=(1, 1), K=1, clip=0, mask=True),
    'rms_clip':     dict(shape=(67, 131), r=2, bg=0, regions=(1, 1), K=1, clip=2, n_sigma=3.0, rademacher=True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case: dict(R, T (K, H, W), var, mask, sigma (each None or an array), settings)."""
    c = CASES[name]
    shape, r, K = c['shape'], c['r'], c['K']
    H, W = shape
    rng = np.random.default_rng(sum(map(ord, name)))
    R = star_field(shape, 100 + len(name), n_stars=12 if H < 60 else 30, noise=3.0)
    n_out = 0 if not c['clip'] else (1 if c.get('rademacher') else 3)
    # the outliers sit where the reference is blank, footprint and all: such a pixel has no leverage on the kernel, so
    # an outlier there hardly moves the residuals of the other pixels
    oy = (np.arange(n_out) * 2 + 1) * H // (2 * max(n_out, 1)) if n_out else np.zeros(0, int)
    ox = rng.integers(2 * r + 2, W - 2 * r - 2, n_out)
    for y, x in zip(oy, ox):
        R[y - r:y + r + 1, x - r:x + r + 1] = 0.0
    if c.get('fail'):                    # region 5 sees a reference of zeros
        R[20 - r:, 32 - r:] = 0.0
    Rd = R.astype(np.float64)
    kt = true_kernel()
    T = np.empty((K, H, W), np.float32)
    var = np.empty((K, H, W), np.float32) if c.get('var') else None
    mask = np.zeros((K, H, W), np.uint8) if c.get('mask') else None
    for k in range(K):
        kk = np.roll(kt, k, axis=1) if r >= 2 else kt[1:4, 1:4]
        sg = SIGMA * (1.0 + 0.3 * np.sin(np.arange(W) / 5.0 + k)[None, :] * np.ones((H, 1))) if var is not None \
            else np.full(shape, SIGMA)
        noise = sg * (rng.choice([-1.0, 1.0], shape) if c.get('rademacher') else NOISE * rng.uniform(-1, 1, shape))
        t = (0.7 + 0.1 * k) * convolve_same(Rd, kk) + plane(shape, 5.0 + k, 2.0 * (c['bg'] > 0), -1.0 * (c['bg'] > 0)) + noise
        if c['clip']:
            t[oy, ox] += (1.0e4 if c.get('rademacher') else OUTLIER) * sg[oy, ox]
        if c.get('nan_T'):
            t[H // 2, W // 3] = np.nan
        T[k] = t
        if var is not None:
            var[k] = sg ** 2
            var[k, 3, 4] = 0.0
            var[k, H - 5, 5] = np.inf
        if mask is not None:
            mask[k, H // 3:H // 3 + 3, W // 2:W // 2 + 4] = 1
    if c.get('nan_R'):
        R = R.copy()
        R[H // 4, (2 * W) // 3] = np.nan
    if c.get('fail'):                    # region 0 keeps fewer than 2 P pixels
        mask[:, 0:20, 0:14] = 1
    sigma = np.full(K, SIGMA, np.float32) if c.get('sigma') else None
    return dict(R=R, T=T, var=var, mask=mask, sigma=sigma,
                settings=dict(r=r, bg_degree=c['bg'], regions=c['regions'], clip_iters=c['clip'],
                              n_sigma=c.get('n_sigma', 4.0)))


@functools.lru_cache(maxsize=None)
def wanted(name):
    """The restatement of every frame of a case, margins asserted."""
    c = case(name)
    return [subtract(c['T'][k], c['R'], var=None if c['var'] is None else c['var'][k],
                     mask=None if c['mask'] is None else c['mask'][k],
                     sigma=None if c['sigma'] is None else c['sigma'][k], check_margin=True, **c['settings'])
            for k in range(len(c['T']))]


# ---- the physics scene ----------------------------------------------------------------------------------------------------
PHYS = dict(shape=(56, 64), sigma=1.0, delta=400.0, aperture=6.0, r=2, n_frames=3, hit=50.0,
            stars=[(12.3, 10.8, 9000.0), (30.6, 14.2, 20000.0), (50.1, 9.7, 6000.0), (20.4, 30.3, 15000.0),
                   (44.7, 28.9, 30000.0), (9.8, 45.2, 12000.0), (32.5, 44.6, 8000.0), (54.2, 46.1, 25000.0)],
            variable=3, width=1.4, hit_at=(20, 56))


def _gaussian(shape, x0, y0, flux, s):
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return flux / (2.0 * np.pi * s * s) * np.exp(-0.5 * ((x - x0) ** 2 + (y - y0) ** 2) / (s * s))


@functools.lru_cache(maxsize=None)
def physics_scene():
    """A deep reference (noise sigma / 10) and frames of the same scene with star ``variable`` brighter by delta,
    blurred by the known kernel (here of sum 1), scaled by 0.7, on a tilted plane, with Gaussian noise of known sigma and
    one pixel hit of 50 sigma."""
    p = PHYS
    shape, s = p['shape'], p['sigma']
    rng = np.random.default_rng(2024)
    scene = sum(_gaussian(shape, x, y, f, p['width']) for x, y, f in p['stars'])
    R = (scene + 0.1 * s * rng.standard_normal(shape)).astype(np.float32)
    K = true_kernel() / 0.8
    x, y, _ = p['stars'][p['variable']]
    T = np.empty((p['n_frames'],) + shape, np.float32)
    for k in range(p['n_frames']):
        t = 0.7 * convolve_same(scene + _gaussian(shape, x, y, p['delta'], p['width']), K) + plane(shape, 20.0, 3.0, -2.0)
        t += s * rng.standard_normal(shape)
        t[p['hit_at']] += p['hit'] * s
        T[k] = t
    return dict(R=R, T=T, xy=np.array([(a, b) for a, b, _ in p['stars']]), K=K)


def aperture_sum_subsampled(img, x0, y0, radius, n=9):
    """The circular-aperture sum by n x n subsampling of every pixel: what the CPU check of the physics scene uses in
    place of the device's exact overlaps (its error, below 1e-3 of the sum, is far inside the 5 sigma of the check)."""
    H, W = img.shape
    off = (np.arange(n) + 0.5) / n - 0.5
    yy, xx = np.mgrid[0:H, 0:W]
    frac = np.zeros((H, W))
    for dy in off:
        for dx in off:
            frac += ((xx + dx - x0) ** 2 + (yy + dy - y0) ** 2 <= radius ** 2)
    frac /= n * n
    sel = frac > 0
    return float((img[sel] * frac[sel]).sum())
