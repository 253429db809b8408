"""Difference imaging: a reference image, typically the deep co-add, PSF-matched to each frame and subtracted
(``lc_diffim_frames``, ``lc_frames_subtract_reference``; DESIGN.md §5 "Difference imaging").  The reference has no such
step, as it has no co-add.  Per frame and per region of the image a convolution kernel of free pixel values and a
polynomial background are fitted by least squares; what is left after the subtraction is what varied.  The light curves
this gives use no PSF model, no starlet background and no optimiser: a cross-check of the forward model's."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import f32, ptr

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)

DOWNLOAD_ALL = tuple(name for name, _ in _lib.DIFFIM_OUT_FIELDS if name != 'split_ms')
DOWNLOAD_DEFAULT = ('diff', 'kernel', 'bg', 'scale', 'n_used', 'chi2', 'status')
_NP = {C.c_float: np.float32, C.c_double: np.float64, C.c_int32: np.int32}


def _n_background(bg_degree):
    return {0: 1, 1: 3, 2: 6}[bg_degree]


def _settings(shape, r, bg_degree, regions, clip_iters, n_sigma, download, what):
    """The checks that need no library, then (DiffimCfg, gy, gx).  Raises ValueError."""
    h, w = shape
    r, bg_degree, clip_iters = int(r), int(bg_degree), int(clip_iters)
    try:
        gy, gx = (int(v) for v in regions)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: regions must be (gy, gx), not {regions!r}') from None
    if not 1 <= r <= 7:
        raise ValueError(f'{what}: r must lie in 1 .. 7, not {r}')
    if bg_degree not in (0, 1, 2):
        raise ValueError(f'{what}: bg_degree must be 0, 1 or 2, not {bg_degree}')
    if gy < 1 or gx < 1 or gy * gx > 64:
        raise ValueError(f'{what}: regions of at least 1 x 1 and at most 64 in all, not {gy} x {gx}')
    if clip_iters < 0:
        raise ValueError(f'{what}: clip_iters must be >= 0, not {clip_iters}')
    if not (np.isfinite(n_sigma) and n_sigma > 0):
        raise ValueError(f'{what}: n_sigma must be positive and finite, not {n_sigma}')
    if h < 2 * r + 1 or w < 2 * r + 1 or h * w >= 2 ** 31 or gy > h or gx > w:
        raise ValueError(f'{what}: images of {h} x {w} pixels with r = {r} and {gy} x {gx} regions')
    unknown = set(download) - set(DOWNLOAD_ALL)
    if unknown:
        raise ValueError(f'{what}: download takes {DOWNLOAD_ALL}, not {sorted(unknown)}')
    if not len(tuple(download)):
        raise ValueError(f'{what}: nothing to download')
    return _lib.DiffimCfg(r, bg_degree, gy, gx, clip_iters, float(n_sigma)), gy, gx


def _outputs(K, shape, cfg, download):
    """(dict of arrays, DiffimOut) for K frames."""
    h, w = shape
    G, nk = cfg.gy * cfg.gx, (2 * cfg.r + 1) ** 2
    P = nk + _n_background(cfg.bg_degree)
    shapes = dict(diff=(K, h, w), kernel=(K, G, 2 * cfg.r + 1, 2 * cfg.r + 1), bg=(K, G, 6), scale=(K, G), n_used=(K, G),
                  chi2=(K, G), status=(K, G), gram=(K, G, P, P), rhs=(K, G, P), split_ms=(3,))
    arrays, struct = {}, _lib.DiffimOut()
    for name, t in _lib.DIFFIM_OUT_FIELDS:
        if name in download or name == 'split_ms':
            arrays[name] = np.zeros(shapes[name], _NP[t])
            setattr(struct, name, arrays[name].ctypes.data_as(C.POINTER(t)))
    return arrays, struct


def _per_slot(values, n, what):
    if values is None:
        return None
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(values, np.float32).reshape(-1), (n,)), dtype=np.float32)
    if not (np.isfinite(s) & (s > 0)).all():
        raise ValueError(f'{what}: sigma must be finite and > 0')
    return s


def _mask(mask, shape, what):
    if mask is None:
        return None
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if m.shape != shape:
        raise ValueError(f'{what}: the mask must have the shape {shape}, got {m.shape}')
    return m


def match_and_subtract(images, reference, variance=None, mask=None, sigma=None, r=3, bg_degree=1, regions=(1, 1),
                       clip_iters=2, n_sigma=4.0, download=DOWNLOAD_DEFAULT, ctx=None):
    """``reference`` (h, w) matched to each of ``images`` ((h, w) or (K, h, w), already on the reference's grid) and
    subtracted, in one device call (``lc_diffim_frames``).  variance: per pixel, of the shape of ``images``: the fit is
    weighted by 1 / variance, and a pixel whose variance is not finite or not > 0 stays out of it.  mask: nonzero keeps a
    pixel out of the fit; its difference is still computed.  sigma: per frame, for the clipping and chi2 where no
    variance is given; with neither, the residual rms of the previous round clips.  r: half width of the kernel, 1 .. 7;
    bg_degree 0, 1 or 2; regions (gy, gx): the kernel and the background are fitted per region; clip_iters further
    rounds leave out the pixels with |D| > n_sigma sigma.  download: which of diff, kernel, bg, scale, n_used, chi2,
    status, gram, rhs come back.  Returns a dict of them (K first, then the gy gx regions, row-major; for a 2-D ``images``
    without the K axis) plus kernel_ms and split_ms (Gram sums, host solves, subtraction)."""
    what = 'match_and_subtract'
    d = f32(images)
    single = d.ndim == 2
    if single:
        d = d[None]
    if d.ndim != 3 or 0 in d.shape:
        raise ValueError(f'{what}: expected (h, w) or (K, h, w) images, got {np.shape(images)}')
    K, h, w = d.shape
    ref = f32(reference)
    if ref.shape != (h, w):
        raise ValueError(f'{what}: the reference must have the shape {(h, w)}, got {ref.shape}')
    cfg, gy, gx = _settings((h, w), r, bg_degree, regions, clip_iters, n_sigma, download, what)
    var = None
    if variance is not None:
        var = f32(variance)[None] if single and np.ndim(variance) == 2 else f32(variance)
        if var.shape != d.shape:
            raise ValueError(f'{what}: the variance must have the shape of the images')
    m = _mask(np.asarray(mask)[None] if single and np.ndim(mask) == 2 else mask, (K, h, w), what)
    s = _per_slot(sigma, K, what)
    arrays, struct = _outputs(K, (h, w), cfg, download)
    ctx = ctx or _lib.default_context()
    ms = C.c_float()
    ctx.check(_lib.lib().lc_diffim_frames(ctx.h, K, h, w, ptr(d), ptr(ref), ptr(var),
                                          None if m is None else m.ctypes.data_as(_u8p), ptr(s), C.byref(cfg),
                                          C.byref(struct), C.byref(ms)), 'lc_diffim_frames')
    out = {name: (a[0] if single and name != 'split_ms' else a) for name, a in arrays.items()}
    out['kernel_ms'] = ms.value
    return out


def difference_frames(fs, results, reference_image, frames=None, sigma=None, mask=None, **kw):
    """``FrameSet.subtract_reference`` of the frames that ``register_frames`` solved, with the conventions of
    ``coadd_frames``: ``results`` is its list, one entry per frame of ``fs``; ``frames`` (default: all) the frames to
    take, of which those that failed are skipped.  reference_image: typically ``coadd_frames(...)['image']``, on the grid
    that ``origin`` names (default: the reference frame's).  sigma: None, one value, or one per frame of the SET, indexed
    like ``results`` (as ``coadd_frames`` takes ``flux_scale``).  mask: None, one (H, W) mask for every frame, or
    (K, H, W) with one per frame of the set.  So the caller need not know which registrations failed.  Everything else
    goes to ``FrameSet.subtract_reference``.  Returns its dict plus ``frames``: the frames that went in, in the order of
    the outputs."""
    K = len(results)
    take = np.arange(K) if frames is None else np.asarray(frames, np.int64).reshape(-1)
    used = np.array([k for k in take if results[k]['success']], dtype=np.int64)
    if not len(used):
        raise ValueError('difference_frames: no registered frame to subtract from')
    if sigma is not None:
        try:
            sigma = np.broadcast_to(np.asarray(sigma, np.float32).reshape(-1), (K,))[used]
        except ValueError:
            raise ValueError(f'difference_frames: sigma must be one value or one per frame of the set ({K})') from None
    if mask is not None:
        mask = np.asarray(mask)
        if mask.ndim == 2:
            mask = np.broadcast_to(mask, (len(used),) + mask.shape)
        elif mask.ndim == 3 and len(mask) == K:
            mask = mask[used]
        else:
            raise ValueError(f'difference_frames: the mask must be (H, W) or ({K}, H, W), got {mask.shape}')
    out = fs.subtract_reference(used, [results[k]['transform'] for k in used], reference_image, sigma=sigma, mask=mask, **kw)
    out['frames'] = used
    return out


def difference_light_curves(diff, scale, positions_xy, r, sigma=None, regions=(1, 1), ctx=None):
    """Exact circular-aperture sums of ``D / scale`` per frame: the flux of each position against the reference image, in
    the reference's units (``photutils.aperture_photometry``).  diff: (K, h, w); scale: (K,) or (K, G) as the
    subtraction gives it, with ``regions`` (gy, gx) where G > 1: a position takes the scale of the region it lies in;
    positions_xy: (S, 2); r: the radius.  sigma: per frame, the pixel noise of the frame: adds ``flux_err`` =
    sigma sqrt(pi r^2) / scale.  Returns dict(flux (K, S), NaN where the aperture touches a NaN or leaves the image, and
    flux_err (K, S) or None)."""
    from ..photutils import CircularAperture, aperture_photometry
    d = f32(diff)
    if d.ndim == 2:
        d = d[None]
    K, h, w = d.shape
    xy = np.asarray(positions_xy, np.float64).reshape(-1, 2)
    gy, gx = (int(v) for v in regions)
    sc = np.asarray(scale, np.float64).reshape(K, -1)
    if sc.shape[1] != gy * gx:
        raise ValueError(f'difference_light_curves: {sc.shape[1]} scales per frame for {gy} x {gx} regions')
    # the region of a position: rows [i h // gy, (i + 1) h // gy), columns likewise
    row = np.clip(np.rint(xy[:, 1]).astype(np.int64), 0, h - 1)
    col = np.clip(np.rint(xy[:, 0]).astype(np.int64), 0, w - 1)
    gi = np.searchsorted(np.arange(1, gy + 1) * h // gy, row, side='right')
    gj = np.searchsorted(np.arange(1, gx + 1) * w // gx, col, side='right')
    per_pos = sc[:, gi * gx + gj]                                   # (K, S)
    flux = np.empty((K, len(xy)))
    aperture = CircularAperture(xy, r)
    for k in range(K):
        flux[k] = aperture_photometry(d[k], aperture, ctx=ctx)['aperture_sum'] / per_pos[k]
    err = None
    if sigma is not None:
        s = np.broadcast_to(np.asarray(sigma, np.float64).reshape(-1), (K,))
        err = s[:, None] * np.sqrt(np.pi * float(r) ** 2) / np.abs(per_pos)
    return dict(flux=flux, flux_err=err)
