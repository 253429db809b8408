"""A float64 NumPy restatement of the SPEC of DESIGN.md section 5 "Aperture sums", written from the SPEC and not from the
kernel: the whole fraction grid from the closed form (no shortcut for the pixels inside the circle or outside it within
its bounding box), the four
outputs with the good-pixel rule, the bound of the GPU tests, and the same integrals in 50-digit arithmetic."""
import numpy as np

EPS = 2.0 ** -53


def _F(t, r):
    s = np.sqrt((r - t) * (r + t))
    return 0.5 * (t * s + r * r * np.arctan2(t, s))


def _Q(x, y, r):
    """Signed area of the circle of radius r about the origin inside [0, x] x [0, y]; x and y broadcast."""
    ax, ay = np.minimum(np.abs(x), r), np.minimum(np.abs(y), r)
    ax, ay = np.broadcast_arrays(ax, ay)
    xk = np.sqrt((r - ay) * (r + ay))
    q = np.where(ax * ax + ay * ay <= r * r, ax * ay, xk * ay + _F(ax, r) - _F(xk, r))
    return np.sign(x) * np.sign(y) * q


def fractions(h, w, xc, yc, r):
    """(h, w) float64: the area of every pixel's square inside the circle, clamped to [0, 1].  A pixel whose square does not
    reach into the circle's bounding square weighs exactly 0 (the four terms of the closed form cancel there only to
    rounding), so that a circle outside the image gives exact zeros, as the SPEC has it."""
    j, i = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    x0, x1, y0, y1 = (j - 0.5) - xc, (j + 0.5) - xc, (i - 0.5) - yc, (i + 0.5) - yc
    f = np.clip(_Q(x1, y1, r) - _Q(x0, y1, r) - _Q(x1, y0, r) + _Q(x0, y0, r), 0.0, 1.0)
    reach = np.zeros((h, w), bool)
    reach[box(h, w, xc, yc, r)] = True
    return np.where(reach, f, 0.0)


def pixel_fraction(i, j, xc, yc, r):
    """The fraction of one pixel (i, j), which may lie anywhere."""
    x0, x1, y0, y1 = (j - 0.5) - xc, (j + 0.5) - xc, (i - 0.5) - yc, (i + 0.5) - yc
    f = lambda x, y: float(_Q(np.float64(x), np.float64(y), r))
    return min(max(f(x1, y1) - f(x0, y1) - f(x1, y0) + f(x0, y0), 0.0), 1.0)


def aperture_sums(data, xc, yc, r, error=None, mask=None):
    """(sum, sum_err, area, bad_area) of one aperture on one 2-D float32 image, accumulated in float64.  sum_err is None
    without an error map."""
    d = np.asarray(data)
    assert d.dtype == np.float32 and d.ndim == 2
    f = fractions(d.shape[0], d.shape[1], xc, yc, r)
    unmasked = np.ones(d.shape, bool) if mask is None else np.asarray(mask) == 0
    finite = np.isfinite(d)
    e2 = None
    if error is not None:
        e = np.asarray(error)
        assert e.dtype == np.float32 and e.shape == d.shape
        finite &= np.isfinite(e)
        e2 = e.astype(np.float64) ** 2
    good, bad = unmasked & finite, unmasked & ~finite
    total = float(np.sum(f[good] * d[good].astype(np.float64)))
    err = None if e2 is None else float(np.sqrt(np.sum(f[good] * e2[good])))
    return total, err, float(np.sum(f[good])), float(np.sum(f[bad]))


def box(h, w, xc, yc, r):
    """The circle's bounding box clipped to the image, as (row slice, column slice); empty slices outside."""
    j0, j1 = max(0, int(np.floor(xc - r + 0.5))), min(w - 1, int(np.ceil(xc + r - 0.5)))
    i0, i1 = max(0, int(np.floor(yc - r + 0.5))), min(h - 1, int(np.ceil(yc + r - 0.5)))
    return slice(i0, max(i1 + 1, i0)), slice(j0, max(j1 + 1, j0))


def bound(values, xc, yc, r):
    """16 x 2^-53 max(1, pi r^2) sum |values| over the clipped bounding box (finite values only): what the device's sum of
    frac * values may differ by from the restatement's.  2 of the 16 is the measured error of the closed form against
    50-digit arithmetic, 4 the margin for the device's atan2 and sqrt; float64 summation of at most 2^9 terms per lane
    fits well inside."""
    v = np.asarray(values, np.float64)
    sl = box(v.shape[0], v.shape[1], xc, yc, r)
    part = np.abs(v[sl])
    return 16 * EPS * max(1.0, np.pi * r * r) * float(np.sum(part[np.isfinite(part)]))


def mp_pixel_fraction(i, j, xc, yc, r, dps=50):
    """The same integrals in ``dps``-digit arithmetic (mpmath) on the same float64 inputs, the asin form."""
    import mpmath as mp
    with mp.workdps(dps):
        R, X, Y = mp.mpf(float(r)), mp.mpf(float(xc)), mp.mpf(float(yc))

        def F(t):
            return (t * mp.sqrt(R * R - t * t) + R * R * mp.asin(t / R)) / 2

        def Q(x, y):
            ax, ay = min(abs(x), R), min(abs(y), R)
            if ax * ax + ay * ay <= R * R:
                q = ax * ay
            else:
                xk = mp.sqrt(R * R - ay * ay)
                q = xk * ay + F(ax) - F(xk)
            return mp.sign(x) * mp.sign(y) * q

        half = mp.mpf(1) / 2
        x0, x1, y0, y1 = j - half - X, j + half - X, i - half - Y, i + half - Y
        return float(Q(x1, y1) - Q(x0, y1) - Q(x1, y0) + Q(x0, y0))


def tangent_cases(n_general=100, n_tangent=100, seed=20):
    """(i, j, xc, yc, r, tangent) of single pixels on the rim: ``n_general`` anywhere on it (tangent None), ``n_tangent``
    with a pixel edge within 1e-12 .. 1e-5 px of the circle's extreme in x or in y (tangent 'x' or 'y'), on either side of
    it (the sliver pixel and its neighbour inside, alternately).  r is log-uniform in [0.2, 64]."""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n_general):
        r = float(np.exp(rng.uniform(np.log(0.2), np.log(64.0))))
        xc, yc, th = rng.uniform(60, 70), rng.uniform(60, 70), rng.uniform(0, 2 * np.pi)
        cases.append((int(np.rint(yc + r * np.sin(th))), int(np.rint(xc + r * np.cos(th))), xc, yc, r, None))
    for c in range(n_tangent):
        r = float(np.exp(rng.uniform(np.log(0.2), np.log(64.0))))
        delta = float(10.0 ** rng.uniform(-12, -5)) * (1 if c % 4 < 2 else -1)     # > 0: the extreme is inside the edge
        edge = int(rng.integers(100, 140)) + 0.5
        along, across = edge - delta - r, rng.uniform(60, 70)                        # extreme = along + r = edge - delta
        inner, outer = int(edge - 0.5), int(edge + 0.5)
        k = outer if c % 2 else inner
        if c % 8 < 4:
            cases.append((int(np.rint(across)), k, along, across, r, 'x'))
        else:
            cases.append((k, int(np.rint(across)), across, along, r, 'y'))
    return cases
