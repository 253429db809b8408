"""Checker for lc_ccdmask_stamps: a NumPy restatement of the bad row / column SPEC of DESIGN.md §5 ("Bad rows and
columns"): ccdproc's ``ccdmask(byblocks=False, findbadcolumns=True)`` followed by the reference's reduction to whole
rows and columns (lightcurver/processes/cutout_making.py:67-80).

Not part of the product path.  ``ccdmask(..., dtype=np.float32)`` follows the SPEC's float32 operation order, so the
device kernel must reproduce its masks exactly; ``dtype=np.float64`` is the same algorithm in double precision, for the
float32-against-float64 check.  Vectorised over a (K, n, n) stack, in chunks of stamps (the 49-value windows of a large
batch do not fit in memory at once)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

CHUNK = 256


def med7x7(X):
    """Step 2: the full 7 x 7 median (rank 24 of 49) with scipy's 'reflect' boundary (d c b a | a b c d | d c b a,
    which NumPy's pad calls 'symmetric')."""
    P = np.pad(X, [(0, 0)] * (X.ndim - 2) + [(3, 3), (3, 3)], mode='symmetric')
    w = sliding_window_view(P, (7, 7), axis=(-2, -1))
    w = w.reshape(w.shape[:-2] + (49,))
    return np.partition(w, 24, axis=-1)[..., 24]


def percentile(x, p):
    """Step 3: NumPy's linear percentile along the last axis, every operation in the dtype of x."""
    dt = x.dtype.type
    m = x.shape[-1]
    q = dt(p) / dt(100)
    v = dt(m - 1) * q
    lo = int(np.floor(v))
    hi = min(lo + 1, m - 1)
    t = dt(v - dt(lo))
    s = np.partition(x, (lo, hi), axis=-1)
    a, b = s[..., lo], s[..., hi]
    d = b - a
    if t >= dt(0.5):
        return b - d * (dt(1) - t)
    return a + d * t


def fill_short_gaps(M, ngood=5):
    """Step 5 (findbadcolumns), in place and in ccdproc's order, along axis -2 of a (..., n, n) bool array: for line =
    0 .. n - ngood - 2, where M[line] is set, for i = 2 .. ngood + 1: M[line + i] set -> M[line : line + i] set."""
    n = M.shape[-2]
    for line in range(0, n - ngood - 1):
        for i in range(2, ngood + 2):
            sel = M[..., line, :] & M[..., line + i, :]
            M[..., line:line + i, :] |= sel[..., None, :]
    return M


def reduce_lines(M):
    """Step 6: columns flagged at both ends, rows flagged at both ends, and the mask that holds them whole."""
    bad_cols = M[..., 0, :] & M[..., -1, :]
    bad_rows = M[..., :, 0] & M[..., :, -1]
    return bad_cols, bad_rows, bad_cols[..., None, :] | bad_rows[..., :, None]


def _chunk(D, lsigma, hsigma, ngood, findbadcolumns):
    dt = D.dtype.type
    K, n = D.shape[0], D.shape[-1]
    with np.errstate(invalid='ignore', over='ignore'):
        M = ~np.isfinite(D)
        R = D - med7x7(D)
        Rf = R.reshape(K, -1)
        sigma = (percentile(Rf, 69.1) - percentile(Rf, 30.9)) / dt(2)
        sigma[M.reshape(K, -1).any(axis=1)] = np.nan       # step 1: every comparison below is then false
        s = sigma[:, None, None]
        thr = (R < -(dt(lsigma) * s)) | (R > dt(hsigma) * s)
    M4 = M | thr
    M5 = fill_short_gaps(M4.copy(), ngood) if findbadcolumns else M4
    bad_cols, bad_rows, rowcol = reduce_lines(M5)
    return dict(R=R, sigma=sigma, mask4=M4, mask=M5, bad_cols=bad_cols, bad_rows=bad_rows, rowcol=rowcol)


def ccdmask(data, lsigma=9.0, hsigma=9.0, ngood=5, findbadcolumns=True, dtype=np.float32):
    """data (K, n, n) or (n, n).  Returns dict(R, sigma (K,), mask4 = the mask after step 4, mask = the ccdmask result,
    bad_cols, bad_rows (K, n), rowcol (K, n, n))."""
    D = np.asarray(data)
    single = D.ndim == 2
    D = np.array(D.reshape((-1,) + D.shape[-2:]), dtype=np.float32).astype(dtype)
    parts = [_chunk(D[k:k + CHUNK], lsigma, hsigma, ngood, findbadcolumns) for k in range(0, len(D), CHUNK)]
    out = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    if single:
        out = {key: (v if key == 'sigma' else v[0]) for key, v in out.items()}
    return out


def star_stamps(n, F=8, S=8, seed=None):
    """The F * S star stamps and noise maps of make_psf_dataset(F, S, n, seed=n), as (K, n, n) stacks."""
    from lightcurver_amd.synthetic import make_psf_dataset
    ds = make_psf_dataset(F=F, S=S, n=n, seed=n if seed is None else seed)
    return ds['data'].reshape(-1, n, n).copy(), ds['noisemap'].reshape(-1, n, n).copy()


def inject_lines(data, noisemap, rng, depth=30.0, modulation=0.3):
    """One bad column per stamp at depth x the stamp's median noise, modulated by +- modulation along the line; on odd
    stamps also a negative row of the same depth.  Returns (perturbed copy, column index per stamp, row index per
    stamp or -1)."""
    d = np.array(data, dtype=np.float32)
    K, n = d.shape[0], d.shape[-1]
    cols = rng.integers(0, n, size=K)
    rows = np.where(np.arange(K) % 2 == 1, rng.integers(0, n, size=K), -1)
    for k in range(K):
        amp = depth * float(np.nanmedian(noisemap[k]))
        d[k, :, cols[k]] += (amp * (1.0 + modulation * rng.uniform(-1.0, 1.0, size=n))).astype(np.float32)
        if rows[k] >= 0:
            d[k, rows[k], :] -= (amp * (1.0 + modulation * rng.uniform(-1.0, 1.0, size=n))).astype(np.float32)
    return d, cols, rows


def lines_found(res, cols, rows):
    """Per stamp: the injected column (and row, where there is one) is among bad_cols (bad_rows)."""
    k = np.arange(len(cols))
    return res['bad_cols'][k, cols] & np.where(rows >= 0, res['bad_rows'][k, np.maximum(rows, 0)], True)


def device_batch(n, K, seed):
    """The inputs of the device comparison: K star stamps with injected lines, a partial-cutout NaN border on every
    fifth stamp, stamp 1 constant and stamp 2 quantised (one level and a few outliers: sigma = 0) when K >= 3."""
    S = 8
    d, nm = star_stamps(n, F=(K + S - 1) // S, S=S, seed=seed)
    d, nm = d[:K], nm[:K]
    rng = np.random.default_rng(seed + 1)
    d, cols, rows = inject_lines(d, nm, rng)
    c = (cols[0] + n // 2) % n                               # stamp 0: two hot pixels three lines apart, a gap to fill
    d[0, [1, 4], c] += np.float32(30.0 * np.median(nm[0]))
    w = max(1, n // 5)
    for k in range(4, K, 5):
        sl = [(slice(None), slice(0, w)), (slice(0, w), slice(None)), (slice(None), slice(n - w, n)),
              (slice(n - w, n), slice(None))][k // 5 % 4]
        d[k][sl] = np.nan
    if K >= 3:
        d[1] = np.float32(0.25)
        d[2] = quantised_stamp(n)
    return d


def quantised_stamp(n):
    """A stamp of one level with a few pixels one step up or down, apart from each other: every 7 x 7 median is the
    level, R is 0 there and +-1 at those pixels, and both percentiles are 0, so sigma = 0."""
    q = np.full((n, n), 3.0, np.float32)
    q[1, 2] = 4.0
    q[n - 2, n - 3] = 2.0
    q[n // 2, 1] = 4.0
    q[n // 2 + 3, 1] = 4.0          # three lines below the other one in the same column: step 5 fills the gap
    return q


# ---- settings other than the defaults --------------------------------------------------------------------------------
SETTINGS_SIZES = ((16, 16), (33, 12))          # (n, K) of device_batch(n, K, seed=n)


def settings_cases(n):
    """The settings of the device comparison at stamp size n, each a dict of what differs from lsigma = hsigma = 9,
    ngood = 5.  Every one changes the restatement's ``mask`` on device_batch(n, K, seed=n) (asserted by
    tests/test_ccdmask_cpu.py).  The asymmetric pair catches a swap of the two thresholds; ngood = n - 2 is the last
    value at which the fill loop runs, and there it reads the last row; from n - 1 on no line can start a fill."""
    return ([dict(lsigma=3), dict(hsigma=3), dict(lsigma=3, hsigma=20), dict(lsigma=0)]
            + [dict(ngood=g) for g in (0, 1, 2, n - 3, n - 2, n - 1, n, n + 5)] + [dict(lsigma=2, hsigma=2, ngood=n - 2)])


_settings_wanted = {}


def settings_wanted(n, K):
    """(data, the restatement at the defaults, [(settings, the restatement with them)]) of one SETTINGS_SIZES entry,
    computed once and shared by the CPU and the device tests."""
    if (n, K) not in _settings_wanted:
        d = device_batch(n, K, seed=n)
        _settings_wanted[n, K] = d, ccdmask(d), [(kw, ccdmask(d, **kw)) for kw in settings_cases(n)]
    return _settings_wanted[n, K]
