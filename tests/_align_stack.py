"""NumPy restatement of the SPEC of DESIGN.md §5 "Align and stack" (lc_align_stack, include/lcmi.h): the cubic B-spline
prefilter and resample that scipy.ndimage.shift and scipy.ndimage.rotate run (order 3, mode='constant'), and the
sigma-clipped weighted stack.  ``dtype`` selects the precision of everything but the coordinates and the in-range test,
which are double as in the SPEC; float32 is the device's arithmetic operation by operation, float64 is what is pinned
against scipy.  Sums whose order matters (the recursions of the prefilter, the 16 taps, the sums over the epochs) are
sequential loops here, vectorised only across independent lines / pixels."""
import numpy as np

POLE = np.sqrt(3.0) - 2.0
HORIZON = 32            # terms of the causal initial sum: |POLE|^32 = 5e-19
SIZES = (8, 17, 32, 33, 64, 128)
# (s_y, s_x, angle in degrees): scipy's shift=(s_y, s_x) = (-dy, -dx), then rotate(angle)
GEOMETRIES = ((0.3, -0.7, 0.0), (-1.25, 2.5, 0.37), (0.0, 0.0, 180.2), (0.49, 0.51, -179.6), (3.7, -2.2, 12.0))
INTEGER_SHIFT = (2.0, -3.0, 0.0)
STACK_CASES = ((1, 16), (2, 16), (3, 16), (64, 32), (65, 33), (1000, 16))      # (E, n), C = 3

# Worst |float32 restatement - scipy float64| over the blobs of ``make_blobs(5, n, seed=n)`` x GEOMETRIES, in units of
# the peak of scipy's image; measured by tests/test_align_stack_cpu.py (which fails if a figure here is exceeded) and
# recorded in DESIGN.md.  The device is held to four times these.
F32_ALIGN_ERROR = {8: 3.2e-7, 17: 2.0e-7, 32: 2.8e-7, 33: 2.9e-7, 64: 3.5e-7, 128: 3.6e-7}
# Worst |float32 restatement - float64 restatement| of the stack over the pixels away from a rejection boundary, in
# units of the largest |stack| of the float64 restatement, per STACK_CASES entry (inputs: make_stack_case(3, E, n,
# stack_seed((E, n)))); measured and recorded the same way.
F32_STACK_ERROR = {(1, 16): 2.1e-8, (2, 16): 8.6e-8, (3, 16): 1.1e-7, (64, 32): 5.0e-7, (65, 33): 5.8e-7,
                   (1000, 16): 1.5e-6}
# The same figure at an n_sigma other than 3 (the rejection set differs, so it is measured per (case, n_sigma), not taken
# from F32_STACK_ERROR); (3, 16) at n_sigma 1 is left out: 2.6 % of its pixels sit on a rejection boundary, above NEAR_CAP.
N_SIGMA_CASES = (((64, 32), 1.0), ((64, 32), 1.5), ((64, 32), 2.0), ((64, 32), 5.0), ((65, 33), 1.0), ((65, 33), 1.5),
                 ((65, 33), 2.0), ((65, 33), 5.0), ((3, 16), 1.5), ((3, 16), 2.0))
F32_STACK_ERROR_N_SIGMA = {((64, 32), 1.0): 5.0e-7, ((64, 32), 1.5): 5.0e-7, ((64, 32), 2.0): 5.7e-7, ((64, 32), 5.0): 5.0e-7,
                           ((65, 33), 1.0): 4.7e-7, ((65, 33), 1.5): 4.7e-7, ((65, 33), 2.0): 5.9e-7, ((65, 33), 5.0): 5.7e-7,
                           ((3, 16), 1.5): 1.3e-7, ((3, 16), 2.0): 1.1e-7}
NEAR_CAP = 0.005        # largest share of pixels that may sit on a rejection boundary and be left out of a comparison


def stack_seed(case):
    return 1000 + STACK_CASES.index(tuple(case))


_n_sigma_wanted, _at_3_wanted = {}, {}


def n_sigma_wanted(case, n_sigma):
    """(values, noisemap, the float64 restatement at n_sigma, the float32 one, the float64 one at n_sigma = 3) of one
    N_SIGMA_CASES entry, computed once and shared by the CPU and the device tests."""
    key = (tuple(case), float(n_sigma))
    if key not in _n_sigma_wanted:
        E, n = case
        values, noise = make_stack_case(3, E, n, stack_seed(case))
        if tuple(case) not in _at_3_wanted:
            _at_3_wanted[tuple(case)] = stack_cubes(values, noise, dtype=np.float64)
        _n_sigma_wanted[key] = (values, noise, stack_cubes(values, noise, n_sigma=n_sigma, dtype=np.float64),
                                stack_cubes(values, noise, n_sigma=n_sigma, dtype=np.float32),
                                _at_3_wanted[tuple(case)])
    return _n_sigma_wanted[key]


def stack_cubes(values, noisemap, **kw):
    """``stack`` of every cube of values (C, E, n, n): a dict of arrays with a leading C axis."""
    parts = [stack(v, noisemap, **kw) for v in values]
    return {k: np.stack([p[k] for p in parts]) for k in parts[0]}


# ---- align -----------------------------------------------------------------------------------------------------------
def _prefilter_first_axis(c, dtype):
    """c (n, lines), in place: the coefficients of every line along axis 0."""
    n = c.shape[0]
    z, g = dtype(POLE), dtype(6.0)
    den, last = dtype(1.0 - POLE ** (2 * n - 2)), dtype(POLE / (POLE * POLE - 1.0))
    zk, s = dtype(1.0), np.zeros(c.shape[1], dtype)
    for k in range(min(2 * n - 2, HORIZON)):
        s = s + zk * (g * c[k if k < n else 2 * n - 2 - k])
        zk = dtype(zk * z)
    prev = s / den
    before = prev
    c[0] = prev
    for i in range(1, n):
        before = prev
        prev = g * c[i] + z * prev
        c[i] = prev
    nxt = last * (prev + z * before)
    c[n - 1] = nxt
    for i in range(n - 2, -1, -1):
        nxt = z * (nxt - c[i])
        c[i] = nxt
    return c


def prefilter(img, dtype=np.float64):
    """spline_filter(img, 3, mode='mirror') of a square image: lines along axis 0, then along axis 1."""
    c = np.array(img, dtype=dtype)
    with np.errstate(invalid='ignore'):
        c = _prefilter_first_axis(c, dtype)
        c = np.ascontiguousarray(_prefilter_first_axis(np.ascontiguousarray(c.T), dtype).T)
    return c


def _weights(t, dtype):
    one, two, three, four, six = (dtype(v) for v in (1, 2, 3, 4, 6))
    u = one - t
    w1 = (t * t * (t - two) * three + four) / six
    w2 = (u * u * (u - two) * three + four) / six
    w0 = u * u * u / six
    return [w0, w1, w2, one - w0 - w1 - w2]


def _mirror(i, n):
    i = np.abs(i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def resample(coef, cy, cx, dtype=np.float64):
    """The spline with coefficients ``coef`` at the double coordinates (cy, cx); 0 outside [0, n - 1]."""
    n = coef.shape[0]
    inside = (cy >= 0.0) & (cy <= n - 1) & (cx >= 0.0) & (cx <= n - 1)
    cy, cx = np.where(inside, cy, 0.0), np.where(inside, cx, 0.0)
    fy, fx = np.floor(cy), np.floor(cx)
    wy, wx = _weights((cy - fy).astype(dtype), dtype), _weights((cx - fx).astype(dtype), dtype)
    y0, x0 = fy.astype(np.int64) - 1, fx.astype(np.int64) - 1
    v = np.zeros(cy.shape, dtype)
    with np.errstate(invalid='ignore'):
        for a in range(4):
            yi = _mirror(y0 + a, n)
            for b in range(4):
                t = coef[yi, _mirror(x0 + b, n)]
                t = t * wy[a]
                t = t * wx[b]
                v = v + t
    return np.where(inside, v, dtype(0.0))


def coordinates(n, s_y, s_x, angle):
    """((cy, cx) of the shift step, (cy, cx) of the rotation step): scipy's own double expressions."""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    shift = (y + (-float(s_y)), x + (-float(s_x)))
    rad = np.deg2rad(float(angle))
    c, s = np.cos(rad), np.sin(rad)
    ctr = (n - 1) / 2.0
    oy, ox = ctr - (c * ctr + s * ctr), ctr - (-s * ctr + c * ctr)
    rot = ((oy + y * c) + x * s, (ox + y * (-s)) + x * c)
    return shift, rot


def coordinate_margin(n, s_y, s_x, angle):
    """Smallest distance of a resampling coordinate from the edges 0 and n - 1 of the in-range test, over the steps whose
    coordinates are rounded: an integer shift gives index + integer and a zero angle gives the identity matrix with a zero
    offset, both exact in double, so those steps decide the same everywhere and are left out."""
    shift, rot = coordinates(n, s_y, s_x, angle)
    worst = np.inf
    if float(s_y) != np.floor(s_y):
        worst = min(worst, np.abs(shift[0]).min(), np.abs(shift[0] - (n - 1)).min())
    if float(s_x) != np.floor(s_x):
        worst = min(worst, np.abs(shift[1]).min(), np.abs(shift[1] - (n - 1)).min())
    if float(angle) != 0.0:
        for c in rot:
            worst = min(worst, np.abs(c).min(), np.abs(c - (n - 1)).min())
    return worst


def align(img, s_y, s_x, angle, dtype=np.float64):
    """rotate(shift(img, (s_y, s_x)), angle, reshape=False) with scipy's defaults."""
    n = img.shape[0]
    shift, rot = coordinates(n, s_y, s_x, angle)
    moved = resample(prefilter(img, dtype), shift[0], shift[1], dtype)
    return resample(prefilter(moved, dtype), rot[0], rot[1], dtype)


def scipy_align(img, s_y, s_x, angle):
    from scipy.ndimage import rotate, shift
    return rotate(shift(np.asarray(img, np.float64), (s_y, s_x)), angle, reshape=False)


def make_blobs(E, n, seed):
    """(E, n, n) float32: Gaussian blobs on a pedestal (so that the zeros outside the moved frame show) plus noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n]
    out = np.empty((E, n, n))
    for e in range(E):
        img = 20.0 + rng.normal(0.0, 1.0, (n, n))
        for _ in range(3):
            cy, cx = rng.uniform(1.0, n - 2.0, 2)
            sig = rng.uniform(0.8, 1.0 + n / 16.0)
            img += rng.uniform(50.0, 500.0) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * sig * sig))
        out[e] = img
    return out.astype(np.float32)


def geometry_arrays(E, geometries=GEOMETRIES):
    g = np.array([geometries[e % len(geometries)] for e in range(E)], dtype=np.float64)
    return np.ascontiguousarray(g[:, :2]), np.ascontiguousarray(g[:, 2])


# ---- stack -----------------------------------------------------------------------------------------------------------
def median(values):
    """Exact per-pixel order statistic over the finite samples along axis 0, in the dtype of ``values``."""
    v = np.asarray(values)
    half = v.dtype.type(0.5)
    srt = np.sort(np.where(np.isfinite(v), v, np.nan), axis=0)        # NaN sorts last
    m = np.isfinite(v).sum(axis=0)
    lo = np.take_along_axis(srt, np.maximum((m - 1) // 2, 0)[None], axis=0)[0]
    hi = np.take_along_axis(srt, (m // 2)[None].clip(0, v.shape[0] - 1), axis=0)[0]
    with np.errstate(invalid='ignore'):
        med = np.where(m % 2 == 1, lo, half * (lo + hi))
    return np.where(m > 0, med, v.dtype.type(np.nan))


def stack(values, noisemap, n_sigma=3.0, clip=True, dtype=np.float64, near_tol=1e-5):
    """values (E, ...) and noisemap (E, ...) -> dict(median, dev, stack, n_rejected, near): the SPEC's stack in ``dtype``;
    near = a finite epoch of the pixel lies within near_tol * n_sigma * dev of the rejection threshold."""
    v, s = np.asarray(values, dtype=dtype), np.asarray(noisemap, dtype=dtype)
    fin = np.isfinite(v)
    m = fin.sum(axis=0).astype(dtype)
    med = median(v)
    E = v.shape[0]
    with np.errstate(invalid='ignore', divide='ignore'):
        tot = np.zeros(v.shape[1:], dtype)
        for e in range(E):
            tot = tot + np.where(fin[e], v[e], dtype(0))
        mean = tot / m
        q = np.zeros(v.shape[1:], dtype)
        for e in range(E):
            d = v[e] - mean
            q = q + np.where(fin[e], d * d, dtype(0))
        dev = np.sqrt(q / m)
        thr = dtype(n_sigma) * dev
        every = ~np.isfinite(dev) if clip else np.ones(dev.shape, bool)
        dist = np.abs(v - med)
        keep = fin & (every[None] | (dist <= thr))
        sw, swv = np.zeros(v.shape[1:], dtype), np.zeros(v.shape[1:], dtype)
        for e in range(E):
            w = dtype(1) / s[e]
            sw = sw + np.where(keep[e], w, dtype(0))
            swv = swv + np.where(keep[e], w * v[e], dtype(0))
        out = swv / sw
        # (dev = 0: every finite sample equals the median, 0 <= 0 in any precision: not a rounding boundary)
        near = (fin & (np.abs(dist - thr) <= dtype(near_tol) * thr)).any(axis=0) & ~every & (thr > 0)
    return dict(median=med, dev=dev, stack=out, n_rejected=(fin & ~keep).sum(axis=0).astype(np.int32), near=near)


def make_stack_case(C, E, n, seed):
    """(values (C, E, n, n), noisemap (E, n, n)) float32: Gaussian noise of the noise map's width around a smooth image,
    2 % of the samples moved out by 20 sigma, 1 % NaN."""
    rng = np.random.default_rng(seed)
    noise = rng.uniform(0.5, 2.0, (E, n, n))
    y, x = np.mgrid[0:n, 0:n]
    base = 10.0 + 5.0 * np.sin(0.3 * x) * np.cos(0.2 * y)
    v = base[None, None] + noise[None] * rng.standard_normal((C, E, n, n))
    out = rng.random(v.shape) < 0.02
    v = np.where(out, v + 20.0 * noise[None] * rng.choice([-1.0, 1.0], v.shape), v)
    v[rng.random(v.shape) < 0.01] = np.nan
    return v.astype(np.float32), noise.astype(np.float32)
