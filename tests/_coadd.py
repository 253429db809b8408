"""NumPy restatement of the SPEC of DESIGN.md §5 "Co-addition of frames" (lc_frames_coadd, include/lcmi.h): the resampling
of a frame onto a grid of reference pixels through an affine map (order 1, or Keys' cubic convolution), and the combine.
``dtype`` selects the precision of everything but the coordinates, the floor and the all-taps-inside test, which are
double as in the SPEC; float32 is the device's arithmetic operation by operation, float64 is what is pinned against
scipy and what the device is compared with.  Sums whose order matters (the taps, the sums over the frames) are
sequential loops, vectorised only across pixels.  The cases the CPU and the device tests share are made here, once."""
import numpy as np

from tests import _align_stack as AS

COMBINES = ('mean', 'median', 'sigma_clip')
FRAME_SHAPE = (40, 48)                                   # (h, w): not square
K_SET = 8                                                # frames of the set
NAN_FRAME, NAN_PIXEL = 1, (20, 25)                       # one NaN pixel (y, x) in one frame of the set
GRIDS = (((40, 48), (0, 0)), ((50, 37), (-6, -4)))       # ((H, W), (x0, y0)): the frame's own, and one with uncovered pixels
# (shift x, shift y, rotation in degrees about the frame's centre, scale)
GEOMETRIES = ((0.0, 0.0, 0.0, 1.0), (3.0, -2.0, 0.0, 1.0), (0.3, -0.7, 0.0, 1.0), (-1.25, 2.5, 0.37, 1.0),
              (0.8, -0.4, 12.0, 1.015), (0.2, 0.1, 180.2, 1.0))
COUNTS = (1, 2, 5, 67)
N_SIGMA = 1.5            # of the parity cases: one sample can lie m / sqrt(m - 1) deviations from the median, 2.5 at m = 5
# the last frame count whose samples the combine keeps in LDS and the first beyond it; at 5 sigma a quarter of the pixels
# reject something and 0.4 % sit on a rejection boundary (at 3 sigma 1.2 % would, above NEAR_CAP)
LARGE_COUNTS, LARGE_N_SIGMA = (640, 641), 5.0
# Worst |float32 restatement - float64 restatement| of a warped sample in units of 2^-24 |s| sum_taps |v|, over
# GEOMETRIES x GRIDS x both orders on the frames of make_frames(); measured by tests/test_coadd_cpu.py (which fails if the
# figure here is exceeded) and recorded in DESIGN.md.  The device is held to C_BOUND = the next power of two >= 4 r.
F32_WARP_RATIO = 1.07          # measured: 1.064 at order 1, 0.481 at order 3
C_BOUND = 8.0
EPS = 2.0 ** -24


def next_power_of_two(x):
    return 2.0 ** np.ceil(np.log2(x))


def affine_of(geometry, shape=FRAME_SHAPE):
    """The (2, 3) map from reference pixels to frame pixels: scale and rotation about the frame's centre, then the shift."""
    sx, sy, angle, scale = geometry
    h, w = shape
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    rad = np.deg2rad(angle)
    a, b = scale * np.cos(rad), scale * np.sin(rad)
    return np.array([[a, -b, cx - (a * cx - b * cy) + sx], [b, a, cy - (b * cx + a * cy) + sy]])


def make_frames(K=K_SET, shape=FRAME_SHAPE, seed=5):
    """(K, h, w) float32: Gaussian blobs on a pedestal plus noise, one NaN pixel in frame NAN_FRAME."""
    rng = np.random.default_rng(seed)
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((K, h, w))
    for k in range(K):
        img = 20.0 + rng.normal(0.0, 1.0, (h, w))
        for _ in range(4):
            cy, cx = rng.uniform(2.0, h - 3.0), rng.uniform(2.0, w - 3.0)
            sig = rng.uniform(0.9, 3.0)
            img += rng.uniform(50.0, 500.0) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * sig * sig))
        out[k] = img
    out[NAN_FRAME][NAN_PIXEL] = np.nan
    return out.astype(np.float32)


# ---- resample ---------------------------------------------------------------------------------------------------------
def cubic_weights(t, dtype):
    """Keys' cubic convolution with a = -1/2, Horner as the SPEC writes it: the weights of the taps f - 1 .. f + 2."""
    one, two, three, four, five = (dtype(v) for v in (1, 2, 3, 4, 5))
    return [((two - t) * t - one) * t / two, ((three * t - five) * t * t + two) / two,
            ((four - three * t) * t + one) * t / two, (t - one) * t * t / two]


def warp(img, affine, grid_shape, origin=(0, 0), order=3, flux_scale=1.0, dtype=np.float64):
    """dict(sample (H, W) in ``dtype``, NaN where a tap lies outside; inside (H, W) bool: every tap in the frame; tapabs
    (H, W) float64: the sum of |v| over the taps, 0 outside; s: the factor applied, in ``dtype``)."""
    img = np.asarray(img)
    h, w = img.shape
    H, W = grid_shape
    A = np.asarray(affine, np.float64)[:2]
    y, x = np.mgrid[0:H, 0:W]
    x, y = (x + int(origin[0])).astype(np.float64), (y + int(origin[1])).astype(np.float64)
    xs, ys = (A[0, 0] * x + A[0, 1] * y) + A[0, 2], (A[1, 0] * x + A[1, 1] * y) + A[1, 2]
    fx, fy = np.floor(xs), np.floor(ys)
    before, after = (1, 2) if order == 3 else (0, 1)
    inside = (fx >= before) & (fx <= w - 1 - after) & (fy >= before) & (fy <= h - 1 - after)
    tx, ty = (xs - fx).astype(dtype), (ys - fy).astype(dtype)
    if order == 3:
        wx, wy = cubic_weights(tx, dtype), cubic_weights(ty, dtype)
    elif order == 1:
        wx, wy = [dtype(1) - tx, tx], [dtype(1) - ty, ty]
    else:
        raise ValueError(order)
    ix = np.where(inside, fx, before).astype(np.int64) - before
    iy = np.where(inside, fy, before).astype(np.int64) - before
    v = np.zeros((H, W), dtype)
    tapabs = np.zeros((H, W))
    src = img.astype(dtype)
    with np.errstate(invalid='ignore'):
        for a in range(len(wy)):
            for b in range(len(wx)):
                t = src[iy + a, ix + b]
                tapabs = tapabs + np.abs(t.astype(np.float64))
                t = t * wy[a]
                t = t * wx[b]
                v = v + t
        det = abs(A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0])
        s = dtype(float(flux_scale) * det)
        v = v * s
    return dict(sample=np.where(inside, v, dtype(np.nan)), inside=inside, tapabs=np.where(inside, tapabs, 0.0), s=s)


def scipy_warp_order1(img, affine, grid_shape, origin=(0, 0)):
    """scipy.ndimage.affine_transform(order=1, mode='constant', cval=nan) on the same grid, times |det|."""
    from scipy.ndimage import affine_transform
    A = np.asarray(affine, np.float64)[:2]
    x0, y0 = origin
    # scipy: input coordinate (row, column) = matrix @ output (row, column) + offset
    matrix = np.array([[A[1, 1], A[1, 0]], [A[0, 1], A[0, 0]]])
    offset = np.array([A[1, 0] * x0 + A[1, 1] * y0 + A[1, 2], A[0, 0] * x0 + A[0, 1] * y0 + A[0, 2]])
    out = affine_transform(np.asarray(img, np.float64), matrix, offset=offset, output_shape=tuple(grid_shape), order=1,
                           mode='constant', cval=np.nan)
    return out * abs(A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0])


# ---- combine ----------------------------------------------------------------------------------------------------------
def combine(samples, weights, mode='sigma_clip', n_sigma=3.0, dtype=np.float64):
    """samples (n, ...) and weights (n,) -> dict(image, weight, count, n_rejected, margin): the SPEC's combine in
    ``dtype`` over the finite samples in the order given; margin: the smallest | |v - med| - n_sigma dev | among the
    finite samples of a pixel (inf where nothing is decided: another mode, no sample, a deviation that is 0 or not finite)."""
    v = np.asarray(samples, dtype=dtype)
    wk = np.asarray(weights, dtype=dtype).reshape(-1)
    n = v.shape[0]
    fin = np.isfinite(v)
    m = fin.sum(axis=0)
    margin = np.full(v.shape[1:], np.inf)
    with np.errstate(invalid='ignore', divide='ignore'):
        med = AS.median(v) if mode != 'mean' else np.zeros(v.shape[1:], dtype)
        keep = fin
        if mode == 'sigma_clip':
            mf = m.astype(dtype)
            tot = np.zeros(v.shape[1:], dtype)
            for k in range(n):
                tot = tot + np.where(fin[k], v[k], dtype(0))
            mean = tot / mf
            q = np.zeros(v.shape[1:], dtype)
            for k in range(n):
                d = v[k] - mean
                q = q + np.where(fin[k], d * d, dtype(0))
            dev = np.sqrt(q / mf)
            thr = dtype(n_sigma) * dev
            every = ~np.isfinite(dev)
            dist = np.abs(v - med)
            keep = fin & (every[None] | (dist <= thr))
            # (dev = 0: every finite sample equals the median, and 0 <= thr in any precision: not a rounding boundary)
            gap = np.where(fin & ~every[None] & (thr > 0)[None], np.abs(dist - thr), np.inf).astype(np.float64)
            margin = gap.min(axis=0)
        sw, swv = np.zeros(v.shape[1:], dtype), np.zeros(v.shape[1:], dtype)
        for k in range(n):
            sw = sw + np.where(keep[k], wk[k], dtype(0))
            swv = swv + np.where(keep[k], wk[k] * v[k], dtype(0))
        image = med if mode == 'median' else swv / sw
        image = np.where(m > 0, image, dtype(np.nan))
    return dict(image=image, weight=sw, count=keep.sum(axis=0).astype(np.int32),
                n_rejected=(fin & ~keep).sum(axis=0).astype(np.int32), margin=margin)


def coadd(frames, frame_index, affines, grid_shape, origin=(0, 0), flux_scale=None, weights=None, order=3,
          mode='sigma_clip', n_sigma=3.0, dtype=np.float64):
    """The whole SPEC: ``combine`` of the ``warp`` of every listed frame, plus samples (n, H, W), tapabs (n, H, W) and
    s (n,): what the bounds of the device tests are made of."""
    n = len(frame_index)
    g = np.ones(n) if flux_scale is None else np.asarray(flux_scale, np.float32).astype(np.float64)
    wk = np.ones(n, np.float32) if weights is None else np.asarray(weights, np.float32)
    parts = [warp(frames[frame_index[k]], affines[k], grid_shape, origin, order, g[k], dtype) for k in range(n)]
    samples = np.stack([p['sample'] for p in parts])
    out = combine(samples, wk, mode, n_sigma, dtype)
    out.update(samples=samples, tapabs=np.stack([p['tapabs'] for p in parts]), s=np.array([float(p['s']) for p in parts]))
    return out


def sample_bound(tapabs, s, c=None):
    """B = c 2^-24 |s| sum_taps |v| of every sample: (n, H, W)."""
    c = C_BOUND if c is None else c
    return c * EPS * np.abs(np.asarray(s, np.float64)).reshape((-1,) + (1,) * (tapabs.ndim - 1)) * tapabs


def pixel_bound(ref):
    """The bound on a combined pixel of ``coadd(..., dtype=float64)``: max_k B_k + (m + 2) 2^-24 max_k |v_k| over the
    finite samples (mean and median are 1-Lipschitz in the samples; the second term is the float32 sums of the combine)."""
    fin = np.isfinite(ref['samples'])
    B = np.where(fin, sample_bound(ref['tapabs'], ref['s']), 0.0).max(axis=0)
    vmax = np.where(fin, np.abs(ref['samples']), 0.0).max(axis=0)
    return B + (fin.sum(axis=0) + 2) * EPS * vmax


# ---- the cases shared by tests/test_coadd_cpu.py and tests/test_coadd_gpu.py ---------------------------------------------
_frames = {}


def frames():
    if 'f' not in _frames:
        _frames['f'] = make_frames()
    return _frames['f']


def case_inputs(n):
    """(frame_index (n,), affines (n, 2, 3), flux_scale (n,) float32, weights (n,) float32) of the parity case with n
    frames: slot k takes GEOMETRIES[(k + n) % 6]; from n = 5 on, slot 1 lies wholly outside either grid, slot 2 has the
    weight 0 and slot 3 lists the frame of slot 0 again."""
    rng = np.random.default_rng(100 + n)
    index = (np.arange(n) * 3 + 1) % K_SET                     # frame NAN_FRAME is slot 0
    affines = np.stack([affine_of(GEOMETRIES[(k + n) % len(GEOMETRIES)]) for k in range(n)])
    g = rng.uniform(0.8, 1.2, n).astype(np.float32)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32)
    if n >= 5:
        affines[1] = affine_of((500.0, -300.0, 2.0, 1.0))
        w[2] = 0.0
        index[3] = index[0]
    return index.astype(np.int32), affines, g, w


_wanted = {}


def wanted(n, grid, order, mode):
    """The float64 restatement of one parity case, computed once."""
    key = (n, grid, order, mode)
    if key not in _wanted:
        index, affines, g, w = case_inputs(n)
        shape, origin = GRIDS[grid]
        _wanted[key] = coadd(frames(), index, affines, shape, origin, g, w, order, mode, N_SIGMA, np.float64)
    return _wanted[key]


def guarded(ref):
    """The pixels of a sigma_clip case whose decision margin is below twice the tolerance: left out of the comparison
    of values and counts, and at most NEAR_CAP of all."""
    return ref['margin'] < 2.0 * pixel_bound(ref)


NEAR_CAP = 0.01
