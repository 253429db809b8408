"""``Background`` with sep's signature, on the device (``lc_background_frames``, include/lcmi.h).

The reference estimates the sky of every frame it imports with ``sep.Background(image, bw=box, bh=box, fw=3, fh=3)``,
subtracts it (``image - bkg``) and keeps ``bkg.globalrms`` for the noise maps of the stamps
(lightcurver/processes/background_estimation.py:25, frame_importation.py:81-91).  Here the SPEC of DESIGN.md §5 ("Sky
background") runs as HIP kernels over whole frames: a 2-D input is one frame, a (K, h, w) stack is one batched call
whose ``globalback`` and ``globalrms`` are arrays of K.  Only ``fw = fh`` of 1 or 3 with ``fthresh = 0`` is built (the
reference uses 3); anything else raises ``NotImplementedError``.  There is no CPU fallback."""
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
