"""Checker for lc_background_frames: a NumPy restatement of the sky-background SPEC of DESIGN.md §5 ("Sky background"),
SExtractor's mesh background as ``sep.Background`` runs it for the reference's ``subtract_background``
(lightcurver/processes/background_estimation.py:25).

Not part of the product path.  ``background(frame, ...)`` follows the SPEC step by step in its precision: float32 where the
SPEC says float32, float64 sums.  ``exact=True`` runs every float32 step in float64 instead, for the float32-against-
float64 figures that set the bounds of the device tests.  Each call reports which paths its meshes took (``paths``), so
that a test can assert that its input reaches the path it is there for.  ``scene`` makes the seeded test frames."""
import functools

import numpy as np

NSIGMA, AMIN, MAX_LEVELS = 5.0, 4.0, 4096
STEP = np.sqrt(2.0 / np.pi) * NSIGMA / AMIN
LC_ERR_NONFINITE = -4


def grid(h, w, bw, bh):
    """(ny, nx) of step 1."""
    return (h - 1) // bh + 1, (w - 1) // bw + 1


# ---- steps 3 and 4: one mesh ---------------------------------------------------------------------------------------

def _moments(v):
    v = v.astype(np.float64)
    mean = v.sum() / v.size
    var = (v * v).sum() / v.size - mean * mean
    return mean, (np.sqrt(var) if var > 0.0 else 0.0)


def backstat(v, count, f=np.float32):
    """Step 3 over the good pixels v (float32, raster order) of a mesh of ``count`` pixels.  None for a bad mesh,
    otherwise dict(mean, sigma, npix, nlevels, qscale, qzero) with qscale, qzero in the precision f."""
    if 2 * v.size < count:
        return None
    mean, sigma = _moments(v)
    lcut, hcut = f(mean - 2.0 * sigma), f(mean + 2.0 * sigma)
    vf = v.astype(f)
    sel = v[(vf >= lcut) & (vf <= hcut)]
    if sel.size == 0:          # this project's rule: nothing inside the cuts is a bad mesh
        return None
    mean, sigma = _moments(sel)
    flev = STEP * sel.size + 1.0
    nlevels = int(flev) if flev < MAX_LEVELS else MAX_LEVELS
    qscale = f(2.0 * NSIGMA * sigma / nlevels) if sigma > 0.0 else f(1.0)
    qzero = f(mean - NSIGMA * sigma)
    return dict(mean=mean, sigma=sigma, npix=sel.size, nlevels=nlevels, qscale=qscale, qzero=qzero,
                capped=flev >= MAX_LEVELS)


def backhisto(v, st, f=np.float32):
    """Step 4: the histogram of all good pixels v, int64[nlevels]."""
    cste = f(0.499999) - st['qzero'] / st['qscale']
    b = v.astype(f) / st['qscale'] + cste
    assert b.dtype == f
    ok = (b > f(-1.0)) & (b < f(st['nlevels']))          # (int) truncates: bin 0 takes -1 < b < 1
    return np.bincount(np.trunc(b[ok]).astype(np.int64), minlength=st['nlevels'])


# ---- step 5: the mode ----------------------------------------------------------------------------------------------

def walk_serial(histo, lcut, hcut):
    """The two-ended walk over bins lcut .. hcut as SExtractor writes it: (ilo, ihi, lowsum, highsum), ilo the next bin
    of the low end and ihi the next bin of the high end when all bins are taken."""
    lowsum = highsum = 0
    ilo, ihi = lcut, hcut
    for _ in range(lcut, hcut + 1):
        if lowsum < highsum:
            lowsum += int(histo[ilo])
            ilo += 1
        else:
            highsum += int(histo[ihi])
            ihi -= 1
    return ilo, ihi, lowsum, highsum


def walk_merge(cum, lcut, hcut):
    """The same end state from cum = the inclusive prefix sums of the whole histogram.  The walk merges P[i] = sum of
    the first i bins from the low end with Q[j] = sum of the first j bins from the high end, ties to Q; after T = hcut -
    lcut + 1 steps it has taken a low-end bins, a found by bisection along the T-th diagonal of the merge."""
    def c(i):
        return 0 if i < 0 else int(cum[min(i, len(cum) - 1)])
    T = max(hcut - lcut + 1, 0)
    if T == 0:
        return lcut, hcut, 0, 0
    lo, hi, c0, c1 = 0, T, c(lcut - 1), c(hcut)
    while lo < hi:
        mid = (lo + hi) >> 1
        if c(lcut + mid - 1) - c0 < c1 - c(hcut - (T - 1 - mid)):
            lo = mid + 1
        else:
            hi = mid
    a = lo
    ilo, ihi = lcut + a, hcut - (T - a)
    return ilo, ihi, c(ilo - 1) - c0, c1 - c(ihi)


def backguess(histo, st, walk='merge'):
    """Step 5: (back, rms, path) as float64, path one of 'mode', 'median', 'mean', 'single'."""
    nl = st['nlevels']
    histo = np.asarray(histo, np.int64)
    cum = np.cumsum(histo)
    idx = np.arange(nl, dtype=np.int64)
    m1, m2 = np.cumsum(histo * idx), np.cumsum(histo * idx * idx)       # exact: integers below 2^53

    def rng(c, a, b):
        return int(c[b]) - (int(c[a - 1]) if a > 0 else 0) if b >= a else 0

    def h(i):
        return int(histo[i]) if 0 <= i < nl else 0
    lcut, hcut = 0, nl - 1
    sig, sig1, mea, med = 10.0 * (nl - 1), 1.0, 0.0, 0.0          # mea, med: set by the first round
    n, ran = 100, False
    while n > 0 and sig >= 0.1 and abs(sig / sig1 - 1.0) > 1e-4:
        n -= 1
        ran = True
        sig1 = sig
        if walk == 'merge':
            ilo, ihi, lowsum, highsum = walk_merge(cum, lcut, hcut)
        else:
            ilo, ihi, lowsum, highsum = walk_serial(histo, lcut, hcut) if hcut >= lcut else (lcut, hcut, 0, 0)
        peak = max(h(ilo), h(ihi))
        med = (ihi + 0.5 + ((float(highsum) - float(lowsum)) / (2.0 * peak) if peak > 0 else 0.0)) if ihi >= 0 else 0.0
        total = rng(cum, lcut, hcut)
        if total:
            mea = float(rng(m1, lcut, hcut)) / float(total)
            sig = float(rng(m2, lcut, hcut)) / float(total) - mea * mea
        else:
            mea = sig = 0.0
        sig = float(np.sqrt(sig)) if sig > 0.0 else 0.0
        t = med - 3.0 * sig
        lcut = int(t + 0.5) if t > 0.0 else 0
        t = med + 3.0 * sig
        hcut = int(t + 0.5 if t > 0.0 else t - 0.5) if t < nl - 1 else nl - 1
    if not ran:          # one level (one pixel inside the cuts): no round has run, the moments of step 3 are the result
        return st['mean'], st['sigma'], 'single'
    qz, qs = float(st['qzero']), float(st['qscale'])
    if sig > 0.0:
        if abs((mea - med) / sig) < 0.3:
            back, path = qz + (2.5 * med - 1.5 * mea) * qs, 'mode'
        else:
            back, path = qz + med * qs, 'median'
    else:
        back, path = qz + mea * qs, 'mean'
    return back, sig * qs, path


# ---- steps 6 - 8: the grid of meshes -------------------------------------------------------------------------------

def fill_bad(back, rms):
    """Step 6: NaN marks a bad mesh.  Float32 sums in raster order over the good meshes at the smallest squared
    distance.  Returns (back, rms, meshes filled)."""
    ny, nx = back.shape
    ob, orr = back.copy(), rms.copy()
    good = [(y, x) for y in range(ny) for x in range(nx) if back[y, x] == back[y, x]]
    filled = 0
    for py in range(ny):
        for px in range(nx):
            if back[py, px] == back[py, px]:
                continue
            best, vb, vr, cnt = None, np.float32(0), np.float32(0), 0
            for (y, x) in good:
                d2 = (x - px) ** 2 + (y - py) ** 2
                if best is None or d2 < best:
                    best, vb, vr, cnt = d2, back[y, x], rms[y, x], 1
                elif d2 == best:
                    vb, vr, cnt = vb + back[y, x], vr + rms[y, x], cnt + 1
            ob[py, px], orr[py, px] = vb / back.dtype.type(cnt), vr / back.dtype.type(cnt)
            filled += 1
    return ob, orr, filled


def median_filter(v, fw, fh):
    """Step 7: the fw x fh median; at the grid edge the window shrinks on both sides (SExtractor's filterback), so a
    corner keeps its value and an edge mesh takes the median along the edge."""
    ny, nx = v.shape
    out = np.empty_like(v)
    for py in range(ny):
        ay = min(fh // 2, py, ny - 1 - py)
        for px in range(nx):
            ax = min(fw // 2, px, nx - 1 - px)
            win = np.sort(v[py - ay:py + ay + 1, px - ax:px + ax + 1].ravel())
            out[py, px] = win[win.size // 2]
    return out


def sorted_median(s):
    """Median of a sorted vector in its own precision: the mean of the two middle values for an even count."""
    n = s.size
    return s[n // 2] if n & 1 else (s[n // 2 - 1] + s[n // 2]) / s.dtype.type(2)


def global_values(back, rms):
    """Step 8."""
    gb = sorted_median(np.sort(back.ravel()))
    s = np.sort(rms.ravel())
    gr = sorted_median(s)
    if gr <= 0 and (s > 0).any():
        gr = sorted_median(s[s > 0])
    return gb, gr


# ---- step 9: the spline ----------------------------------------------------------------------------------------------

def spline_z(y):
    """z = y'' / 6 of the natural cubic spline through the nodes y[k] (unit spacing) along axis 0, in float64: the
    Thomas sweep of z[k-1] + 4 z[k] + z[k+1] = y[k-1] - 2 y[k] + y[k+1] with z = 0 at both ends and the pivots c[k] = 1 /
    (4 - c[k-1])."""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    z = np.zeros_like(y)
    if n < 3:
        return z
    c = np.zeros(n)
    d = np.zeros_like(y)
    for k in range(1, n - 1):
        c[k] = 1.0 / (4.0 - c[k - 1])
        d[k] = (((y[k - 1] - 2.0 * y[k]) + y[k + 1]) - d[k - 1]) * c[k]
    for k in range(n - 2, 0, -1):
        z[k] = d[k] - c[k] * z[k + 1]
    return z


def _pieces(npix, b, n, f):
    """Node coordinate of the pixels 0 .. npix - 1 for meshes of b pixels: the piece k (of n >= 2 nodes) and offset B."""
    t = (np.arange(npix).astype(f) + f(0.5)) / f(b) - f(0.5)
    k = np.clip(np.floor(t).astype(np.int64), 0, n - 2)
    return k, t - k.astype(f)


def _cubic(y0, y1, z0, z1, B):
    A = B.dtype.type(1) - B
    return A * y0 + B * y1 + (A * A * A - A) * z0 + (B * B * B - B) * z1


def spline_map(mesh, h, w, bw, bh, f=np.float32):
    """Step 9: the map (h, w) in the precision f through the mesh values (ny, nx); the two solves in float64."""
    mesh = np.asarray(mesh).astype(f)
    ny, nx = mesh.shape
    if ny > 1:
        zy = spline_z(mesh).astype(f)
        k, B = _pieces(h, bh, ny, f)
        node = _cubic(mesh[k], mesh[k + 1], zy[k], zy[k + 1], B[:, None])
    else:
        node = np.repeat(mesh, h, axis=0)
    if nx == 1:
        return np.repeat(node, w, axis=1)
    zx = spline_z(node.T).T.astype(f)
    k, B = _pieces(w, bw, nx, f)
    out = _cubic(node[:, k], node[:, k + 1], zx[:, k], zx[:, k + 1], B[None, :])
    assert out.dtype == f
    return out


# ---- the whole of it -------------------------------------------------------------------------------------------------

def background(frame, mask=None, bw=64, bh=64, fw=3, fh=3, exact=False, maps=True, walk='merge'):
    """One frame (h, w) float32 through steps 1 - 10.  Returns dict(mesh_back, mesh_rms (ny, nx), globalback, globalrms,
    status, back, sub (h, w; with maps), raw_back, raw_rms (before steps 6 - 7, NaN = bad), paths)."""
    f = np.float64 if exact else np.float32
    D = np.asarray(frame, np.float32)
    h, w = D.shape
    ny, nx = grid(h, w, bw, bh)
    good = np.isfinite(D)
    if mask is not None:
        good &= ~np.asarray(mask).astype(bool)
    raw_b, raw_r = np.full((ny, nx), np.nan, f), np.full((ny, nx), np.nan, f)
    paths = dict(mode=0, median=0, mean=0, single=0, capped=0, bad=0, filled=0, partial_x=w % bw != 0, partial_y=h % bh != 0,
                 single_x=nx == 1, single_y=ny == 1)
    for my in range(ny):
        for mx in range(nx):
            sl = (slice(my * bh, min((my + 1) * bh, h)), slice(mx * bw, min((mx + 1) * bw, w)))
            pix = D[sl]
            v = pix[good[sl]]
            st = backstat(v, pix.size, f)
            if st is None:
                paths['bad'] += 1
                continue
            b, r, path = backguess(backhisto(v, st, f), st, walk)
            raw_b[my, mx], raw_r[my, mx] = f(b), f(r)
            paths[path] += 1
            paths['capped'] += bool(st['capped'])
    out = dict(raw_back=raw_b, raw_rms=raw_r, paths=paths)
    if paths['bad'] == nx * ny:
        nan = np.full((ny, nx), np.nan, f)
        out.update(mesh_back=nan, mesh_rms=nan.copy(), globalback=f(np.nan), globalrms=f(np.nan), status=LC_ERR_NONFINITE)
    else:
        b, r, paths['filled'] = fill_bad(raw_b, raw_r)
        b, r = median_filter(b, fw, fh), median_filter(r, fw, fh)
        gb, gr = global_values(b, r)
        out.update(mesh_back=b, mesh_rms=r, globalback=gb, globalrms=gr, status=0)
    if maps:
        out['back'] = spline_map(out['mesh_back'], h, w, bw, bh, f)
        out['sub'] = D.astype(f) - out['back']
    return out


def scene(h, w, nstars, seed, peak_lo=200.0, peak_hi=5000.0):
    """A sky plane 50 + 0.1 x + 0.05 y, N(0, 3) noise and nstars Gaussian stars (sigma 2 px, peaks log-uniform in
    200 .. 5000), float32."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 50.0 + 0.1 * x + 0.05 * y + rng.normal(0.0, 3.0, (h, w))
    for _ in range(nstars):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        peak = np.exp(rng.uniform(np.log(peak_lo), np.log(peak_hi)))
        img += peak * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * 2.0 ** 2))
    return img.astype(np.float32)


def reference_test_frame():
    """The frame of the reference's own test of subtract_background: normal(100, 5) on 100 x 100 pixels."""
    return np.random.default_rng(1).normal(100.0, 5.0, (100, 100)).astype(np.float32)


def one_pixel_corner_frame():
    """(frame, box, sky, sigma): normal(100, 5) on 101 x 101 pixels in boxes of 10, so that the corner mesh is one pixel."""
    return np.random.default_rng(2).normal(100.0, 5.0, (101, 101)).astype(np.float32), 10, 100.0, 5.0


def precision_scenes():
    """(frame, box) of the scenes the precision figures are taken over: the frames of the parity tests."""
    s = scene(130, 195, 40, 3)
    return [(reference_test_frame(), 10), (s, 65), (s, 13), (s, 8), (scene(130, 195, 40, 4), 13), (scene(130, 195, 40, 5), 13),
            (scene(67, 45, 6, 6), 8), (scene(67, 45, 6, 7), 8), (scene(16, 64, 2, 8), 16), (scene(12, 12, 0, 9), 12)]


@functools.lru_cache(maxsize=None)
def precision_figures():
    """The restatement in the SPEC's precision against all-float64 over precision_scenes(): the largest difference of a
    mesh back and of a mesh rms in units of the frame's globalrms, and of a map pixel in units of the frame's largest
    |mesh value| (the map of the float64 mesh values, evaluated in float32 and in float64)."""
    fig = dict(mesh_back=0.0, mesh_rms=0.0, map=0.0)
    for frame, box in precision_scenes():
        a = background(frame, bw=box, bh=box, maps=False)
        e = background(frame, bw=box, bh=box, maps=False, exact=True)
        fig['mesh_back'] = max(fig['mesh_back'], float(np.abs(a['mesh_back'] - e['mesh_back']).max() / e['globalrms']))
        fig['mesh_rms'] = max(fig['mesh_rms'], float(np.abs(a['mesh_rms'] - e['mesh_rms']).max() / e['globalrms']))
        h, w = frame.shape
        mesh = a['mesh_back']
        m32, m64 = spline_map(mesh, h, w, box, box, np.float32), spline_map(mesh, h, w, box, box, np.float64)
        fig['map'] = max(fig['map'], float(np.abs(m32 - m64).max() / np.abs(mesh).max()))
    return fig


# (h, w, bw, bh, nstars, seed, K, (ny, nx)): meshes whose sides differ, on scene(h, w, nstars, seed + k).  A kernel that
# swapped the two sides, or used one of them for both, gives another grid (tests/test_background_cpu.py asserts that the
# three wrong grids differ from the right one, and that the swapped restatement is far outside the device bounds).
UNEQUAL_CASES = (
    (67, 45, 8, 5, 6, 6, 2, (14, 6)),
    (130, 195, 13, 65, 40, 3, 1, (2, 15)),
    (130, 195, 65, 13, 40, 3, 1, (10, 3)),
    (48, 80, 16, 80, 4, 2, 1, (1, 5)),              # a single mesh row
    (48, 80, 48, 10, 4, 2, 1, (5, 2)),
)
_unequal_wanted = {}


def unequal_wanted(case):
    """(frames (K, h, w), [the restatement of each frame, without maps]) of one UNEQUAL_CASES entry, computed once and
    shared by the CPU and the device tests."""
    if case not in _unequal_wanted:
        h, w, bw, bh, nstars, seed, K, _ = case
        frames = np.stack([scene(h, w, nstars, seed + k) for k in range(K)])
        _unequal_wanted[case] = frames, [background(f, bw=bw, bh=bh, maps=False) for f in frames]
    return _unequal_wanted[case]


def unequal_mask(h, w):
    """The mask of the masked case: a block that covers whole meshes of 13 x 65 and 65 x 13 pixels, and scattered pixels."""
    m = np.random.default_rng(h + w).random((h, w)) < 0.02
    m[:65, :39] = True
    return m
