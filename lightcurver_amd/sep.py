"""``Background`` and ``extract`` with sep's signatures, on the device (``lc_background_frames``, ``lc_extract_frames``,
include/lcmi.h).

The reference estimates the sky of every frame it imports with ``sep.Background(image, bw=box, bh=box, fw=3, fh=3)``,
subtracts it (``image - bkg``) and keeps ``bkg.globalrms`` for the noise maps of the stamps
(lightcurver/processes/background_estimation.py:25, frame_importation.py:81-91).  Here the SPEC of DESIGN.md §5 ("Sky
background") runs as HIP kernels over whole frames: a 2-D input is one frame, a (K, h, w) stack is one batched call
whose ``globalback`` and ``globalrms`` are arrays of K.  Only ``fw = fh`` of 1 or 3 with ``fthresh = 0`` is built (the
reference uses 3); anything else raises ``NotImplementedError``.

``extract`` is the SPEC "Source extraction of frames" of the same section: detection, 8-connected labelling and
measurement of whole frames, that is ``sep.extract`` WITHOUT de-blending and WITHOUT cleaning.  ``extract_deblended``
is ``sep.extract`` with both and with sep's own defaults (``lc_extract_frames_deblended``, the SPEC "De-blending and
cleaning of frame objects"); it is not pinned against sep itself, which is absent here.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import f32, ptr

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)


def supported(h, w, bw, bh, fw=3, fh=3):
    """True if the kernels take (h, w) frames with bw x bh meshes and an fw x fh filter (no device needed)."""
    return bool(_lib.lib().lc_background_supported(int(h), int(w), int(bw), int(bh), int(fw), int(fh)))


def _refuse(shape, bw, bh, fw, fh, fthresh):
    if (int(fw), int(fh)) not in ((1, 1), (3, 3)):
        raise NotImplementedError(f'Background: an {fw} x {fh} filter is not built, only 1 x 1 and 3 x 3')
    if float(fthresh) != 0.0:
        raise NotImplementedError('Background: fthresh other than 0 is not built (the reference never sets it)')
    if int(bw) < 1 or int(bh) < 1:
        raise ValueError(f'Background: mesh size {bw} x {bh}')
    if not supported(shape[-2], shape[-1], bw, bh, fw, fh):
        raise NotImplementedError(f'Background: {shape[-2]} x {shape[-1]} pixels in {bw} x {bh} meshes is more than '
                                  '256 meshes along an axis or 2048 in all')


def mesh_shape(h, w, bw, bh):
    return (h - 1) // bh + 1, (w - 1) // bw + 1


def background_frames(stack, mask=None, bw=64, bh=64, fw=3, fh=3, fthresh=0.0, sub=True, back=False, ctx=None):
    """One device call over a (K, h, w) stack; mask (K, h, w), non-zero = ignore.  Returns dict(mesh_back, mesh_rms float32
    (K, ny, nx), globalback, globalrms float32 (K,), status int32 (K,): 0, or -4 for a frame without one good mesh (its
    values are NaN), sub and back float32 (K, h, w) where asked for (None otherwise), kernel_ms device time of the kernels)."""
    d = f32(stack)
    if d.ndim != 3:
        raise ValueError(f'expected a (K, h, w) stack of frames, got {d.shape}')
    _refuse(d.shape, bw, bh, fw, fh, fthresh)
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != d.shape:
            raise ValueError('mask must have the shape of the data')
    ctx = ctx or _lib.default_context()
    K, h, w = d.shape
    ny, nx = mesh_shape(h, w, int(bw), int(bh))
    out = dict(mesh_back=np.empty((K, ny, nx), np.float32), mesh_rms=np.empty((K, ny, nx), np.float32),
               globalback=np.empty(K, np.float32), globalrms=np.empty(K, np.float32), status=np.zeros(K, np.int32),
               sub=np.empty(d.shape, np.float32) if sub else None, back=np.empty(d.shape, np.float32) if back else None)
    ms = C.c_float()
    cfg = _lib.BackgroundCfg(int(bw), int(bh), int(fw), int(fh), float(fthresh))
    if K:
        ctx.check(_lib.lib().lc_background_frames(
            ctx.h, K, h, w, ptr(d), m.ctypes.data_as(_u8p) if m is not None else None, C.byref(cfg), ptr(out['sub']),
            ptr(out['back']), ptr(out['mesh_back']), ptr(out['mesh_rms']), ptr(out['globalback']), ptr(out['globalrms']),
            out['status'].ctypes.data_as(_i32p), C.byref(ms)), 'lc_background_frames')
    out['kernel_ms'] = ms.value
    return out


def background_map(mesh, h, w, bw, bh, ctx=None):
    """The spline map (K, h, w) through the mesh values (K, ny, nx) (``lc_background_map``)."""
    v = f32(mesh)
    if v.ndim != 3 or v.shape[1:] != mesh_shape(h, w, int(bw), int(bh)):
        raise ValueError(f'expected (K, ny, nx) mesh values for {h} x {w} pixels, got {v.shape}')
    ctx = ctx or _lib.default_context()
    out = np.empty((v.shape[0], h, w), np.float32)
    if v.shape[0]:
        ctx.check(_lib.lib().lc_background_map(ctx.h, v.shape[0], int(h), int(w), int(bw), int(bh), ptr(v), ptr(out), None),
                  'lc_background_map')
    return out


class Background:
    """sep.Background: ``globalback``, ``globalrms``, ``back()``, ``rms()``, ``subfrom(data)`` and ``image - bkg``.  For a
    (K, h, w) stack the two global values are arrays of K and the maps are stacks.  ``maskthresh``: a pixel is ignored where
    mask > maskthresh, as in sep."""

    def __init__(self, data, mask=None, maskthresh=0.0, bw=64, bh=64, fw=3, fh=3, fthresh=0.0, ctx=None):
        d = np.asarray(data)
        if d.ndim not in (2, 3):
            raise ValueError(f'Background takes one (h, w) frame or a (K, h, w) stack, got {d.shape}')
        stack = d.reshape((-1,) + d.shape[-2:])
        m = None if mask is None else (np.asarray(mask) > maskthresh).reshape(stack.shape)
        r = background_frames(stack, m, bw, bh, fw, fh, fthresh, sub=False, back=False, ctx=ctx)
        self._set(r, d.shape, bw, bh, ctx)

    @classmethod
    def _from_result(cls, r, shape, bw, bh, ctx=None, frame=None):
        """The object for the whole result r of background_frames, or for its frame ``frame`` alone."""
        self = cls.__new__(cls)
        if frame is not None:
            r = {k: (v[frame:frame + 1] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
        self._set(r, shape, bw, bh, ctx)
        return self

    def _set(self, r, shape, bw, bh, ctx):
        self._shape, self._bw, self._bh, self._ctx = tuple(shape), int(bw), int(bh), ctx
        self._single = len(shape) == 2
        self.mesh_back, self.mesh_rms, self.status = r['mesh_back'], r['mesh_rms'], r['status']
        self.globalback = float(r['globalback'][0]) if self._single else r['globalback']
        self.globalrms = float(r['globalrms'][0]) if self._single else r['globalrms']
        self._maps = {'back': r.get('back')}

    def _map(self, which, mesh, dtype):
        if self._maps.get(which) is None:
            self._maps[which] = background_map(mesh, self._shape[-2], self._shape[-1], self._bw, self._bh, self._ctx)
        return self._maps[which].reshape(self._shape).astype(dtype, copy=False)

    def back(self, dtype=np.float32):
        """The background map of the shape of the data."""
        return self._map('back', self.mesh_back, dtype)

    def rms(self, dtype=np.float32):
        """The map of the background rms: the same spline through the mesh rms."""
        return self._map('rms', self.mesh_rms, dtype)

    def subfrom(self, data):
        """Subtracts the background map from ``data`` in place."""
        data -= self.back(data.dtype)

    def __array__(self, dtype=None, copy=None):
        return self.back() if dtype is None else self.back(dtype)

    __array_ufunc__ = None      # ``ndarray - bkg`` comes to __rsub__ instead of going through __array__

    def __rsub__(self, other):
        """``image - bkg``, subtracted on the host from ``back()`` (a second device call, lc_background_map, the first
        time): for a float32 image the same bits as the ``sub`` of lc_background_frames.  One call for both is
        ``processes.background_estimation.subtract_background``, which takes the fused ``sub``."""
        return np.asarray(other) - self.back()


# ---- source extraction ---------------------------------------------------------------------------------------------

DEFAULT_FILTER_KERNEL = np.array([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]])       # sep's default
OBJECT_FIELDS = ('x', 'y', 'a', 'b', 'theta', 'flux', 'npix', 'peak', 'cpeak', 'xmin', 'xmax', 'ymin', 'ymax', 'xpeak',
                 'ypeak', 'flag')
OBJECT_DTYPE = np.dtype([(n, _lib.EXTRACT_OBJECT_DTYPE[n]) for n in OBJECT_FIELDS])
FLAG_LARGE, FLAG_RANGE, FLAG_EDGE = 1, 2, 4
FLAG_NODEBLEND = 8          # a parent whose box is over 64 pixels, or whose tree exceeds 32 leaves or 64 nodes: kept whole
DEBLEND_DEFAULTS = dict(deblend_nthresh=32, deblend_cont=0.005, clean=True, clean_param=1.0)       # sep's
_DEFAULT = object()


def extract_supported(h, w):
    """True if the kernels take (h, w) frames (no device needed): h, w >= 1 and h w < 2^31."""
    return bool(_lib.lib().lc_extract_supported(int(h), int(w)))


def _filter_flag(filter_kernel):
    if filter_kernel is None:
        return 0
    if filter_kernel is _DEFAULT:
        return 1
    k = np.asarray(filter_kernel, dtype=np.float64)
    if k.shape == (3, 3) and np.array_equal(k, DEFAULT_FILTER_KERNEL):
        return 1
    raise NotImplementedError("extract: only sep's default 3 x 3 filter_kernel and None are built")


def extract_cfg(thresh, minarea, filter_kernel=_DEFAULT):
    if not np.isfinite(thresh) or not thresh > 0:
        raise ValueError(f'extract: thresh = {thresh} must be finite and > 0')
    if int(minarea) < 1:
        raise ValueError(f'extract: minarea = {minarea}')
    return _lib.ExtractCfg(float(thresh), int(minarea), _filter_flag(filter_kernel))


def deblend_cfg(deblend):
    """``lc_deblend_cfg`` of ``deblend``: None or False -> None (no de-blending, no cleaning), True -> sep's defaults, a
    dict -> those defaults with its entries (deblend_nthresh, deblend_cont, clean, clean_param)."""
    if deblend is None or deblend is False:
        return None
    s = dict(DEBLEND_DEFAULTS)
    if deblend is not True:
        unknown = set(deblend) - set(s)
        if unknown:
            raise TypeError(f'deblend: unknown settings {sorted(unknown)}')
        s.update(deblend)
    if float(s['clean_param']) != 1.0:
        raise NotImplementedError('extract: only clean_param = 1.0 is built')
    if int(s['deblend_nthresh']) not in (4, 8, 16, 32):
        raise NotImplementedError('extract: deblend_nthresh must be 4, 8, 16 or 32')
    if not np.isfinite(s['deblend_cont']) or s['deblend_cont'] < 0:
        raise ValueError(f"extract: deblend_cont = {s['deblend_cont']} must be finite and >= 0")
    return _lib.DeblendCfg(int(s['deblend_nthresh']), float(s['deblend_cont']), int(bool(s['clean'])),
                           float(s['clean_param']))


def extract_frames(stack, var, thresh, minarea=5, filter_kernel=_DEFAULT, max_objects=8192, segmentation_map=False,
                   mask=False, objects=True, ctx=None, deblend=None):
    """One device call over a (K, h, w) stack.  ``deblend``: None for ``lc_extract_frames``; True (sep's defaults) or a
    dict of deblend_nthresh, deblend_cont, clean, clean_param for ``lc_extract_frames_deblended``.  ``var``: a (K, h, w) stack of variances, or one variance per frame
    (a scalar or K of them).  Returns dict(objects: list of K record arrays of lc_extract_object (all its fields; None
    without ``objects``), nobj, status int32 (K,): 0, 1 = more objects than ``max_objects`` (the call is repeated once
    with the largest nobj, so 1 is not seen from here), 2 = the labelling's guard, segmap int32 (K, h, w) and mask uint8
    where asked for, kernel_ms)."""
    d = f32(stack)
    if d.ndim != 3:
        raise ValueError(f'expected a (K, h, w) stack of frames, got {d.shape}')
    K, h, w = d.shape
    cfg = extract_cfg(thresh, minarea, filter_kernel)
    dcfg = deblend_cfg(deblend)
    if h < 1 or w < 1:
        raise ValueError(f'extract: frames of {h} x {w} pixels')
    if not extract_supported(h, w):
        raise NotImplementedError(f'extract: {h} x {w} pixels is 2^31 or more')
    if int(max_objects) < 1:
        raise ValueError(f'extract: max_objects = {max_objects}')
    v = f32(var)
    if v.ndim == 3:
        if v.shape != d.shape:
            raise ValueError('var must have the shape of the data, or be one value per frame')
        vplane, vscalar = v, None
    else:
        vplane, vscalar = None, np.ascontiguousarray(np.broadcast_to(v.reshape(-1), (K,)), dtype=np.float32)
    ctx = ctx or _lib.default_context()
    out = dict(nobj=np.zeros(K, np.int32), status=np.zeros(K, np.int32), objects=None,
               segmap=np.zeros(d.shape, np.int32) if segmentation_map else None,
               mask=np.zeros(d.shape, np.uint8) if mask else None, kernel_ms=0.0)
    if not K:
        out['objects'] = [] if objects else None
        return out
    cap = int(max_objects)
    for attempt in range(2):
        table = np.zeros((K, cap), _lib.EXTRACT_OBJECT_DTYPE) if objects else None
        ms = C.c_float()
        outputs = (cap, table.ctypes.data_as(C.c_void_p) if objects else None, out['nobj'].ctypes.data_as(_i32p),
                   out['segmap'].ctypes.data_as(_i32p) if segmentation_map else None,
                   out['mask'].ctypes.data_as(_u8p) if mask else None, out['status'].ctypes.data_as(_i32p), C.byref(ms))
        if dcfg is None:
            ctx.check(_lib.lib().lc_extract_frames(ctx.h, K, h, w, ptr(d), ptr(vplane), ptr(vscalar), C.byref(cfg),
                                                   *outputs), 'lc_extract_frames')
        else:
            ctx.check(_lib.lib().lc_extract_frames_deblended(ctx.h, K, h, w, ptr(d), ptr(vplane), ptr(vscalar),
                                                             C.byref(cfg), C.byref(dcfg), *outputs),
                      'lc_extract_frames_deblended')
        out['kernel_ms'] += ms.value
        if not objects or not (out['status'] == 1).any():
            break
        cap = int(out['nobj'].max())          # the true counts: the second call holds them all
    if objects:
        out['objects'] = [table[k, :min(int(out['nobj'][k]), cap)].copy() for k in range(K)]
    return out


def extract(data, thresh, err=None, var=None, mask=None, minarea=5, filter_kernel=_DEFAULT, deblend_cont=1.0, clean=False,
            segmentation_map=False, max_objects=65536, ctx=None):
    """``sep.extract`` of one frame, without de-blending and without cleaning: note that sep's own defaults are
    ``deblend_cont=0.005`` and ``clean=True``, which are not built, so those two arguments default to what is
    (``deblend_cont=1.0``, ``clean=False``) and anything else raises ``NotImplementedError``, as does a ``filter_kernel``
    other than ``None`` or sep's default 3 x 3 one.  ``thresh`` is in units of the pixel's noise: ``err`` (an rms) or
    ``var`` (a variance), a scalar or an array; without either the variance is 1.  ``mask``: non-zero pixels are invalid.
    Returns a structured array with sep's field names for what is measured (x, y, a, b, theta, flux, npix, peak, cpeak,
    xmin, xmax, ymin, ymax, xpeak, ypeak, flag), and with ``segmentation_map=True`` also the int32 map.  A blended pair
    comes out as one elongated object."""
    if float(deblend_cont) != 1.0:
        raise NotImplementedError('extract: de-blending is not built; pass deblend_cont=1.0 (sep\'s default is 0.005)')
    if clean:
        raise NotImplementedError('extract: cleaning is not built; pass clean=False (sep\'s default is True)')
    return _extract_one(data, thresh, err, var, mask, minarea, filter_kernel, None, segmentation_map, max_objects, ctx)


def extract_deblended(data, thresh, err=None, var=None, mask=None, minarea=5, filter_kernel=_DEFAULT, deblend_nthresh=32,
                      deblend_cont=0.005, clean=True, clean_param=1.0, segmentation_map=False, max_objects=65536, ctx=None):
    """``sep.extract`` of one frame with sep's own defaults: de-blending (``deblend_nthresh`` 4, 8, 16 or 32,
    ``deblend_cont``; >= 1 switches it off) and cleaning (``clean``; only ``clean_param=1.0`` is built).  The other
    arguments and the structured array it returns are those of ``extract``.  A parent whose box is over 64 pixels on a
    side, or whose tree has more than 32 leaves or 64 nodes, stays whole and carries ``FLAG_NODEBLEND``."""
    deblend = dict(deblend_nthresh=deblend_nthresh, deblend_cont=deblend_cont, clean=clean, clean_param=clean_param)
    deblend_cfg(deblend)
    return _extract_one(data, thresh, err, var, mask, minarea, filter_kernel, deblend, segmentation_map, max_objects, ctx)


def _extract_one(data, thresh, err, var, mask, minarea, filter_kernel, deblend, segmentation_map, max_objects, ctx):
    _filter_flag(filter_kernel)
    d = f32(data)
    if d.ndim != 2:
        raise ValueError(f'extract takes one 2-D frame, got {d.shape}')
    if err is not None and var is not None:
        raise ValueError('extract: err and var are exclusive')
    if err is not None:
        e = np.asarray(err, dtype=np.float32)
        v = e * e                             # in float32, as the SPEC says of a caller with err
    elif var is not None:
        v = np.asarray(var, dtype=np.float32)
    else:
        v = np.float32(1.0)
    v = np.asarray(v, np.float32)
    if v.ndim not in (0, 2) or (v.ndim == 2 and v.shape != d.shape):
        raise ValueError('extract: err / var must be a scalar or have the shape of the data')
    if mask is not None:
        m = np.asarray(mask) != 0
        if m.shape != d.shape:
            raise ValueError('mask must have the shape of the data')
        v = np.where(m, np.float32(np.nan), np.broadcast_to(v, d.shape)).astype(np.float32)
    r = extract_frames(d[None], v[None] if v.ndim == 2 else v, thresh, minarea, filter_kernel, max_objects,
                       segmentation_map=segmentation_map, ctx=ctx, deblend=deblend)
    if int(r['status'][0]) == 2:
        raise _lib.LcError('extract: the iteration guard of the labelling was reached')
    objects = objects_view(r['objects'][0])
    return (objects, r['segmap'][0]) if segmentation_map else objects


def objects_view(table):
    """The record array of lc_extract_object as a structured array with sep's field names, in their order."""
    out = np.zeros(len(table), OBJECT_DTYPE)
    for n in OBJECT_FIELDS:
        out[n] = table[n]
    return out
