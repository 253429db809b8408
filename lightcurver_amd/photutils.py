"""``aperture_photometry`` with ``CircularAperture`` in photutils' call shape, on the device (``lc_aperture_sums``,
include/lcmi.h).

The reference takes the starting fluxes of the ROI's point sources from ``aperture_photometry(np.nanmedian(data, 0),
CircularAperture(positions, r))`` (lightcurver/processes/roi_modelling.py:198-204): exact circle / pixel overlaps.  Here
the SPEC of DESIGN.md §5 ("Aperture sums") runs as one HIP kernel, one wave per aperture, in float64:
``aperture_sums_batch`` sums any number of apertures on a (K, h, w) stack in one call, ``aperture_photometry`` is one 2-D
image with photutils' columns.  Only ``method='exact'`` on circles is built (what the reference uses); anything else
raises ``NotImplementedError``.  photutils' treatment of edges and bad pixels is restated from recollection and, like
the sums themselves, not pinned against photutils (it is absent here): the sum is NaN where an unmasked pixel with a
non-finite value has overlap, and NaN for an aperture that does not reach the image.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import f32, ptr

_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)


def _f64ptr(a):
    return None if a is None else a.ctypes.data_as(_lib.dp)


class CircularAperture:
    """photutils.aperture.CircularAperture: ``positions`` is one (x, y) or a list of them, ``r`` the radius in pixels."""

    def __init__(self, positions, r):
        pos = np.asarray(positions, dtype=np.float64)
        if pos.shape == (2,):
            self.isscalar = True
        elif pos.ndim == 2 and pos.shape[1] == 2:
            self.isscalar = False
        else:
            raise ValueError(f'positions must be one (x, y) or an (N, 2) list of them, got {pos.shape}')
        if not np.isfinite(pos).all():
            raise ValueError('positions must be finite')
        if np.ndim(r) != 0 or not np.isfinite(r) or not r > 0:
            raise ValueError(f"'r' must be a positive scalar, got {r!r}")
        self.positions = pos
        self.r = float(r)

    def __len__(self):
        if self.isscalar:
            raise TypeError('a scalar CircularAperture has no len()')
        return len(self.positions)

    @property
    def area(self):
        return np.pi * self.r ** 2


def _aperture_list(K, image_index, positions_xy, r):
    """(image (P,) int32, xy (P, 2) float64, r (P,) float64) of a batch, shapes checked."""
    xy = np.ascontiguousarray(np.asarray(positions_xy, np.float64).reshape(-1, 2))
    P = len(xy)
    try:
        image = np.ascontiguousarray(np.broadcast_to(np.asarray(image_index, np.int32).reshape(-1), (P,)), dtype=np.int32)
        rr = np.ascontiguousarray(np.broadcast_to(np.asarray(r, np.float64).reshape(-1), (P,)), dtype=np.float64)
    except ValueError:
        raise ValueError(f'{P} positions against {np.size(image_index)} image indices and {np.size(r)} radii') from None
    if ((image < 0) | (image >= K)).any():
        raise ValueError(f'an image index outside 0 .. {K - 1}')
    return image, xy, rr


def aperture_sums_batch(images, image_index, positions_xy, r, error=None, mask=None, ctx=None):
    """P exact circular-aperture sums on a (K, h, w) float32 stack in one device call.  image_index: (P,) or one image for
    all; positions_xy: (P, 2) pixel positions (x, y), 0-based with the pixel centres at integers; r: (P,) or one radius
    for all.  error: (K, h, w) per-pixel errors; mask: (K, h, w), nonzero excludes the pixel.  Returns dict(sum, sum_err
    (None without ``error``), area, bad_area float64 (P,) as include/lcmi.h defines them, kernel_ms).  No aperture gives
    empty arrays without a call."""
    d = f32(images)
    if d.ndim != 3 or 0 in d.shape:
        raise ValueError(f'expected a (K, h, w) stack of images, got {d.shape}')
    K, h, w = d.shape
    e = m = None
    if error is not None:
        e = f32(error)
        if e.shape != d.shape:
            raise ValueError(f'the error map must have the shape of the images {d.shape}, got {e.shape}')
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != d.shape:
            raise ValueError(f'the mask must have the shape of the images {d.shape}, got {m.shape}')
    image, xy, rr = _aperture_list(K, image_index, positions_xy, r)
    P = len(xy)
    out = dict(sum=np.zeros(P), sum_err=None if e is None else np.zeros(P), area=np.zeros(P), bad_area=np.zeros(P),
               kernel_ms=0.0)
    if not P:
        return out
    ms = C.c_float()
    ctx = ctx or _lib.default_context()
    ctx.check(_lib.lib().lc_aperture_sums(
        ctx.h, K, h, w, ptr(d), ptr(e), None if m is None else m.ctypes.data_as(_u8p), P, image.ctypes.data_as(_i32p),
        _f64ptr(xy), _f64ptr(rr), _f64ptr(out['sum']), _f64ptr(out['sum_err']), _f64ptr(out['area']),
        _f64ptr(out['bad_area']), C.byref(ms)), 'lc_aperture_sums')
    out['kernel_ms'] = ms.value
    return out


def _reaches(xy, r, h, w):
    """True where the circle has area in common with the image [-0.5, w - 0.5] x [-0.5, h - 0.5]."""
    dx = np.maximum(np.maximum(-0.5 - xy[:, 0], xy[:, 0] - (w - 0.5)), 0.0)
    dy = np.maximum(np.maximum(-0.5 - xy[:, 1], xy[:, 1] - (h - 0.5)), 0.0)
    return dx * dx + dy * dy < r * r


def aperture_photometry(data, apertures, error=None, mask=None, method='exact', ctx=None):
    """photutils.aperture.aperture_photometry for a ``CircularAperture`` on a 2-D image.  Returns a dict of arrays, one
    row per position: ``id`` (from 1), ``xcenter``, ``ycenter``, ``aperture_sum`` and, with ``error``,
    ``aperture_sum_err``.  Masked pixels do not count; the sum (and its error) is NaN where an unmasked pixel with a
    non-finite value or error has overlap, and for an aperture that does not reach the image."""
    if method != 'exact':
        raise NotImplementedError(f"aperture_photometry: method={method!r} is not built, only 'exact' (the reference passes none)")
    if not isinstance(apertures, CircularAperture):
        raise NotImplementedError('aperture_photometry: only CircularAperture is built')
    d = f32(data)
    if d.ndim != 2 or 0 in d.shape:
        raise ValueError(f'data must be a 2-D image, got {d.shape}')
    for name, a in (('error', error), ('mask', mask)):
        if a is not None and np.shape(a) != d.shape:
            raise ValueError(f'{name} must have the shape of data {d.shape}, got {np.shape(a)}')
    xy = apertures.positions.reshape(-1, 2)
    r = aperture_sums_batch(d[None], 0, xy, apertures.r, None if error is None else f32(error)[None],
                            None if mask is None else np.asarray(mask)[None], ctx=ctx)
    undefined = (r['bad_area'] > 0) | ~_reaches(xy, apertures.r, *d.shape)
    out = dict(id=np.arange(1, len(xy) + 1), xcenter=xy[:, 0].copy(), ycenter=xy[:, 1].copy(),
               aperture_sum=np.where(undefined, np.nan, r['sum']))
    if error is not None:
        out['aperture_sum_err'] = np.where(undefined, np.nan, r['sum_err'])
    return out
