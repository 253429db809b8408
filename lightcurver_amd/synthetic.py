"""Seeded synthetic stamp stacks for benchmarks, smoke runs and parity tests.

There is no network and no survey data on the build or GPU boxes, so every workload of
BASELINE.json (C1..C5) is generated on the fly from ``numpy.random.default_rng(seed)`` following
SURVEY.md section 8(d): elliptical Moffat PSFs (beta = 3, FWHM 3-5 data px) with a 2 % smooth
perturbation, star fluxes log-uniform in [1e3, 1e5] e-, noise sigma^2 = rms^2 + |data| with
rms = 5 e- (the noise model of the reference's cutout_making.py:43-51), 1 % masked pixels, values
rescaled to O(1).  This is data generation (NumPy/SciPy on the host), not part of the hot path.
"""
import math

import numpy as np
from scipy.ndimage import gaussian_filter, map_coordinates
from scipy.signal import fftconvolve

GAUSS_FWHM = 2.0
SIGMA_G = GAUSS_FWHM / (2.0 * math.sqrt(2.0 * math.log(2.0)))

CONFIGS = {
    'C1': dict(kind='psf', F=10, S=4, n=32, ss=2, seed=101),
    'C2': dict(kind='psf', F=100, S=8, n=32, ss=2, seed=102),
    'C3': dict(kind='psf', F=500, S=8, n=64, ss=2, seed=103),
    'C4': dict(kind='roi', E=200, M=2, n=64, ss=2, seed=104),
    'C5': dict(kind='roi', E=1000, M=4, n=128, ss=2, seed=105),
}


def _gauss2d(N, X, Y):
    v = np.arange(N, dtype=np.float64)
    gx = np.exp(-0.5 * ((v - X) / SIGMA_G) ** 2)
    gy = np.exp(-0.5 * ((v - Y) / SIGMA_G) ** 2)
    return np.outer(gy, gx) / (2.0 * math.pi * SIGMA_G ** 2)


def _moffat(N, ss, fwhm_x, fwhm_y, phi, beta):
    c = (N - 1) // 2
    idx = np.arange(N, dtype=np.float64) - c
    x, y = idx[None, :], idx[:, None]
    k = 2.0 * math.sqrt(2.0 ** (1.0 / beta) - 1.0)
    ax, ay = ss * fwhm_x / k, ss * fwhm_y / k
    xr = x * math.cos(phi) + y * math.sin(phi)
    yr = -x * math.sin(phi) + y * math.cos(phi)
    m = (1.0 + (xr / ax) ** 2 + (yr / ay) ** 2) ** (-beta)
    return m / m.sum()


def _blocksum(img, ss):
    n = img.shape[-1] // ss
    return img.reshape(img.shape[:-2] + (n, ss, n, ss)).sum(axis=(-1, -3))


def make_narrow_psf(rng, N, ss, perturb=0.02):
    """One 'true' narrow PSF (unit sum) and the parameters it was drawn from."""
    fwhm_full = rng.uniform(3.0, 5.0)
    q = rng.uniform(0.9, 1.0)
    phi = rng.uniform(0.0, math.pi)
    fwhm = math.sqrt(max(fwhm_full ** 2 - (GAUSS_FWHM / ss) ** 2, 1.0))
    mof = _moffat(N, ss, fwhm, fwhm * q, phi, 3.0)
    pert = gaussian_filter(rng.standard_normal((N, N)), 2.0)
    pert *= perturb * mof.max() / np.abs(pert).max()
    # keep the perturbation where the PSF has signal so the truth stays positive and compact
    pert *= mof / mof.max() * 4.0
    s = mof + pert
    return s / s.sum(), dict(fwhm_x=fwhm, fwhm_y=fwhm * q, phi=phi, beta=3.0, fwhm_full=fwhm_full)


def make_psf_dataset(F, S, n, ss=2, seed=0, rms=5.0, masked_fraction=0.01, dtype=np.float32):
    """F frames of S star stamps (n x n): returns dict with data, noisemap, masks (F,S,n,n),
    fwhm_guess (F,), and the truth (narrow PSFs, fluxes, offsets)."""
    rng = np.random.default_rng(seed)
    N = ss * n
    c0 = (N - 1) / 2.0
    data = np.zeros((F, S, n, n))
    noise = np.zeros((F, S, n, n))
    narrow = np.zeros((F, N, N))
    flux = np.exp(rng.uniform(math.log(1e3), math.log(1e5), size=(F, S)))
    x0 = rng.uniform(-0.5, 0.5, size=(F, S))
    y0 = rng.uniform(-0.5, 0.5, size=(F, S))
    fwhm_guess = np.zeros(F)
    for f in range(F):
        narrow[f], par = make_narrow_psf(rng, N, ss)
        fwhm_guess[f] = par['fwhm_full'] * rng.uniform(0.9, 1.1)
        for s in range(S):
            g = _gauss2d(N, c0 + ss * x0[f, s], c0 + ss * y0[f, s])
            clean = flux[f, s] * _blocksum(fftconvolve(g, narrow[f], mode='same'), ss)
            sig = np.sqrt(rms ** 2 + np.abs(clean))
            data[f, s] = clean + sig * rng.standard_normal((n, n))
            noise[f, s] = np.sqrt(rms ** 2 + np.abs(data[f, s]))
    masks = rng.uniform(size=(F, S, n, n)) >= masked_fraction
    scale = np.percentile(data, 99.9)
    return dict(data=(data / scale).astype(dtype), noisemap=(noise / scale).astype(dtype), masks=masks,
                fwhm_guess=fwhm_guess, scale=scale, ss=ss,
                truth=dict(narrow_psf=narrow, flux=flux / scale, x0=x0, y0=y0))


def make_roi_dataset(E, M, n, ss=2, seed=0, rms=5.0, with_background=True, shift_sigma=0.3,
                     alpha_sigma=0.0, dtype=np.float32, alpha=None, dx=None, dy=None):
    """E epochs of an n x n ROI with M point sources, a smooth background and one narrow PSF per
    epoch.  Returns data, noisemap (E,n,n), psf (E,N,N), truth parameters (STARRED kwargs layout:
    a epoch-major, c_x, c_y, dx, dy, alpha, h flat, mean).

    alpha, dx, dy: optional explicit rotation per epoch in degrees (a pier flip, an alt-az field) and shift
    per epoch in data pixels (length E each).  They replace the drawn values and consume no random draws:
    every other value is what the same seed gives without them (the draws still happen and are discarded)."""
    rng = np.random.default_rng(seed)
    N = ss * n
    c0 = (N - 1) / 2.0
    c_x = rng.uniform(-n / 4.0, n / 4.0, size=M)
    c_y = rng.uniform(-n / 4.0, n / 4.0, size=M)
    base = np.exp(rng.uniform(math.log(2e3), math.log(5e4), size=M))
    phase = rng.uniform(0, 2 * math.pi, size=M)
    e = np.arange(E)
    a = base[None, :] * (1.0 + 0.1 * np.sin(2 * math.pi * e[:, None] / max(E, 1) + phase[None, :]))
    dx_drawn = rng.normal(0.0, shift_sigma, size=E)
    dy_drawn = rng.normal(0.0, shift_sigma, size=E)
    dx_drawn[0] = dy_drawn[0] = 0.0
    alpha_drawn = rng.normal(0.0, alpha_sigma, size=E) if alpha_sigma > 0 else np.zeros(E)
    alpha_drawn[0] = 0.0

    def _given(v, drawn, name):
        if v is None:
            return drawn
        v = np.array(v, dtype=np.float64).reshape(-1)
        if v.shape != (E,):
            raise ValueError(f'{name} must hold one value per epoch ({E}), got {v.shape}')
        return v
    dx, dy, alpha = _given(dx, dx_drawn, 'dx'), _given(dy, dy_drawn, 'dy'), _given(alpha, alpha_drawn, 'alpha')
    h = np.zeros((N, N))
    if with_background:
        u = np.arange(N, dtype=np.float64)
        for _ in range(3):
            bx, by = rng.uniform(0.3 * N, 0.7 * N, size=2)
            bs = rng.uniform(0.08 * N, 0.2 * N)
            amp = rng.uniform(5.0, 20.0)
            h += amp * np.exp(-0.5 * (((u[None, :] - bx) / bs) ** 2 + ((u[:, None] - by) / bs) ** 2))
    psf = np.zeros((E, N, N))
    data = np.zeros((E, n, n))
    noise = np.zeros((E, n, n))
    idx = np.arange(N, dtype=np.float64)
    for k in range(E):
        psf[k], _ = make_narrow_psf(rng, N, ss)
        ca, sa = math.cos(math.radians(alpha[k])), math.sin(math.radians(alpha[k]))
        scene = np.zeros((N, N))
        for i in range(M):
            X = c0 + ss * (ca * c_x[i] - sa * c_y[i] + dx[k])
            Y = c0 + ss * (sa * c_x[i] + ca * c_y[i] + dy[k])
            scene += a[k, i] * _gauss2d(N, X, Y)
        px = (idx - c0)[None, :] - ss * dx[k]
        py = (idx - c0)[:, None] - ss * dy[k]
        Xs = c0 + ca * px + sa * py
        Ys = c0 - sa * px + ca * py
        scene += map_coordinates(h, [Ys, Xs], order=1, mode='nearest')
        clean = _blocksum(fftconvolve(scene, psf[k], mode='same'), ss)
        sig = np.sqrt(rms ** 2 + np.abs(clean))
        data[k] = clean + sig * rng.standard_normal((n, n))
        noise[k] = np.sqrt(rms ** 2 + np.abs(data[k]))
    scale = np.max(data)
    truth = dict(a=(a / scale).reshape(E * M), c_x=c_x, c_y=c_y, dx=dx, dy=dy, alpha=alpha,
                 h=(h / scale).reshape(N * N), mean=np.zeros(E))
    return dict(data=(data / scale).astype(dtype), noisemap=(noise / scale).astype(dtype),
                psf=psf.astype(dtype), ss=ss, scale=scale, truth=truth)


def _narrow_psf_of_seeing(rng, N, ss, fwhm_full, perturb=0.02):
    """``make_narrow_psf`` with the full-resolution FWHM given instead of drawn (data pixels): (psf, parameters)."""
    q = rng.uniform(0.9, 1.0)
    phi = rng.uniform(0.0, math.pi)
    fwhm = math.sqrt(max(fwhm_full ** 2 - (GAUSS_FWHM / ss) ** 2, 1.0))
    mof = _moffat(N, ss, fwhm, fwhm * q, phi, 3.0)
    pert = gaussian_filter(rng.standard_normal((N, N)), 2.0)
    pert *= perturb * mof.max() / np.abs(pert).max()
    pert *= mof / mof.max() * 4.0
    s = mof + pert
    return s / s.sum(), dict(fwhm_x=fwhm, fwhm_y=fwhm * q, phi=phi, beta=3.0, fwhm_full=fwhm_full)


def similarity_matrix(rotation_deg, shift_xy, frame_shape, scale=1.0):
    """The 3 x 3 matrix (reference pixels -> frame pixels, (x, y), as ``plate_solving.register_frames`` returns them) of a
    rotation by ``rotation_deg`` about the frame's centre ((w-1)/2, (h-1)/2) followed by ``shift_xy``."""
    h, w = frame_shape
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    th = math.radians(rotation_deg)
    lin = scale * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    m = np.eye(3)
    m[:2, :2] = lin
    m[:2, 2] = c - lin @ c + np.asarray(shift_xy, np.float64)
    return m


def make_frames(frame_shape, stars_xy, star_fluxes, roi_sources_xy, roi_fluxes, rotations_deg, shifts_xy, seeing_pixels,
                transparency, sky_levels, exptimes, ss=2, psf_size=16, rms_electrons=10.0, blank_frames=(), seed=0,
                good_frames=None, footprint_margin=None, min_good_stars=6, min_peak_to_noise=50.0, dtype=np.float32):
    """K whole frames of one field, in electrons per second and NOT sky-subtracted, with the truth that made them: the
    scene of the tests of ``pipeline.light_curves_from_frames``.

    frame_shape (h, w).  stars_xy (S, 2), roi_sources_xy (M, 2): (x, y) in pixels of the reference frame, which is the
    frame whose rotation and shift are zero.  star_fluxes (S,), roi_fluxes (K, M): electrons per second at transparency 1.
    Per frame: rotations_deg and shifts_xy (K, 2) (``similarity_matrix``: reference pixels -> the frame's), seeing_pixels
    (FWHM of the full PSF), transparency (multiplies every source), sky_levels (electrons per second, constant over the
    frame) and exptimes (seconds).  ``blank_frames``: frames that hold sky and noise only.

    Every source is rendered with its frame's PSF, built as the stamp generators of this file build theirs: a narrow PSF
    on an (ss psf_size)^2 grid, convolved with the Gaussian of FWHM 2 high-resolution pixels placed at the source's
    position, binned by ss.  A source therefore has no light beyond psf_size / 2 pixels.  The noise is Gaussian with the
    variance that the noise map of ``FrameSet.cut_stamps`` assumes: per pixel, in electrons, ``rms_electrons``^2 + the
    sources' electrons; ``rms_electrons / exptime`` is the background rms of the frame in its own units.

    Returns dict: frames (K, h, w), exptimes (K,), truth = dict(transforms (K, 3, 3), stars_xy (K, S, 2) and roi_xy
    (K, M, 2): the positions in every frame, star_fluxes (K, S) and roi_fluxes (K, M): electrons per second in the frame
    (transparency included), narrow_psf (K, ss psf_size, ss psf_size), transparency, seeing_pixels, background_rms (K,),
    stars_in_frames (K, S) where ``footprint_margin`` is given).

    Asserted here, on the host in float64, so that tests can rely on it: with ``footprint_margin`` and ``good_frames``
    given, every good frame holds at least ``min_good_stars`` stars inside its footprint shrunk by the margin
    (``utilities.footprint.points_in_footprints``), and no star lies within 1 pixel of a shrunk footprint's boundary in
    any frame with sources (the stars-in-frames table then cannot hinge on registration noise); every star that is in a
    frame's table peaks above ``min_peak_to_noise`` times the noise of a sky pixel of that frame."""
    from .utilities.footprint import frame_footprints, points_in_footprints
    rng = np.random.default_rng(seed)
    h, w = (int(v) for v in frame_shape)
    stars_xy = np.asarray(stars_xy, np.float64).reshape(-1, 2)
    roi_sources_xy = np.asarray(roi_sources_xy, np.float64).reshape(-1, 2)
    S, M = len(stars_xy), len(roi_sources_xy)
    K = len(rotations_deg)
    star_fluxes = np.asarray(star_fluxes, np.float64).reshape(S)
    roi_fluxes = np.asarray(roi_fluxes, np.float64).reshape(K, M)
    per_frame = [np.asarray(v, np.float64).reshape(-1) for v in (seeing_pixels, transparency, sky_levels, exptimes)]
    shifts_xy = np.asarray(shifts_xy, np.float64).reshape(-1, 2)
    if any(len(v) != K for v in per_frame) or len(shifts_xy) != K:
        raise ValueError(f'one rotation, shift, seeing, transparency, sky level and exposure time per frame ({K})')
    seeing, transparency, sky, t = per_frame
    blank = set(int(k) for k in blank_frames)
    N = ss * int(psf_size)
    pad = 2                                                   # the Gaussian's own reach beyond the narrow PSF's support
    pn = int(psf_size) + 2 * pad
    P = ss * pn
    transforms = np.stack([similarity_matrix(rotations_deg[k], shifts_xy[k], (h, w)) for k in range(K)])
    sources_ref = np.concatenate([stars_xy, roi_sources_xy])
    positions = np.stack([sources_ref @ transforms[k][:2, :2].T + transforms[k][:2, 2] for k in range(K)])   # (K, S + M, 2)
    fluxes = np.concatenate([np.broadcast_to(star_fluxes, (K, S)), roi_fluxes], axis=1) * transparency[:, None]
    narrow = np.zeros((K, N, N))
    frames = np.zeros((K, h, w))
    peaks = np.zeros((K, S + M))
    for k in range(K):
        narrow[k], _ = _narrow_psf_of_seeing(rng, N, ss, float(seeing[k]))
        clean = np.zeros((h, w))
        if k not in blank:
            for i, (x, y) in enumerate(positions[k]):
                x0, y0 = int(round(x)) - pn // 2, int(round(y)) - pn // 2        # the patch covers [x0, x0 + pn)
                if x0 >= w or y0 >= h or x0 + pn <= 0 or y0 + pn <= 0:
                    continue
                # high-resolution index of data coordinate u: ss (u - x0) + (ss - 1) / 2
                g = _gauss2d(P, ss * (x - x0) + (ss - 1) / 2.0, ss * (y - y0) + (ss - 1) / 2.0)
                stamp = fluxes[k, i] * _blocksum(fftconvolve(g, narrow[k], mode='same'), ss)
                peaks[k, i] = stamp.max()
                xs, xe, ys, ye = max(x0, 0), min(x0 + pn, w), max(y0, 0), min(y0 + pn, h)
                clean[ys:ye, xs:xe] += stamp[ys - y0:ye - y0, xs - x0:xe - x0]
        sigma = np.sqrt(rms_electrons ** 2 + np.abs(clean) * t[k]) / t[k]
        frames[k] = sky[k] + clean + sigma * rng.standard_normal((h, w))
    truth = dict(transforms=transforms, stars_xy=positions[:, :S], roi_xy=positions[:, S:], star_fluxes=fluxes[:, :S],
                 roi_fluxes=fluxes[:, S:], narrow_psf=narrow, transparency=transparency, seeing_pixels=seeing,
                 background_rms=rms_electrons / t)
    if footprint_margin is not None:
        footprints = frame_footprints(list(transforms), (h, w))
        table = points_in_footprints(stars_xy, footprints, footprint_margin)
        truth['stars_in_frames'] = table
        with_sources = [k for k in range(K) if k not in blank]
        for sign in (-1.0, 1.0):
            moved = points_in_footprints(stars_xy, footprints, max(footprint_margin + sign, 0.0))
            assert np.array_equal(moved[with_sources], table[with_sources]), \
                'a star within 1 pixel of the boundary of a shrunk footprint'
        for k in (good_frames if good_frames is not None else ()):
            assert table[k].sum() >= min_good_stars, f'frame {k}: {table[k].sum()} stars inside its shrunk footprint'
        for k in with_sources:
            ratio = peaks[k, :S][table[k]] * t[k] / rms_electrons
            assert np.all(ratio > min_peak_to_noise), f'frame {k}: a star peaks at {ratio.min():.1f} x the sky noise'
    return dict(frames=frames.astype(dtype), exptimes=t, truth=truth)


def make_config(name, **overrides):
    cfg = dict(CONFIGS[name])
    cfg.update(overrides)
    kind = cfg.pop('kind')
    if kind == 'psf':
        return make_psf_dataset(**cfg)
    return make_roi_dataset(**cfg)
