"""``detect_cosmics`` with astroscrappy's signature, on the device (``lc_detect_cosmics``, include/lcmi.h).

The reference masks the cosmics of every stamp it cuts with ``astroscrappy.detect_cosmics`` (one call per stamp,
lightcurver/processes/cutout_making.py:85).  Here the L.A.Cosmic SPEC of DESIGN.md §5 ("Cosmic-ray detection") runs as
one HIP kernel over a whole stack of stamps: a 2-D input is one stamp, a (K, n, n) stack is one batched call.  Only
``cleantype='meanmask'`` and ``fsmode='median'`` are built; ``inbkg``, the other clean types and ``fsmode='convolve'``
raise ``NotImplementedError`` (the reference uses none of them).  An image that is not a square stamp of 8 .. 128 pixels,
a whole frame for one, runs the same SPEC with the frame as the stamp (``lc_detect_cosmics_frames``, DESIGN.md §5
"Cosmic rays of whole frames"; separable medians only).  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import f32, ptr

_u8p = C.POINTER(C.c_uint8)


def supported(n):
    """True if the kernel takes n x n stamps (8 .. 128)."""
    return bool(_lib.lib().lc_cosmics_supported(int(n)))


def _cfg(sigclip, sigfrac, objlim, gain, readnoise, satlevel, niter, sepmed):
    return _lib.CosmicsCfg(float(sigclip), float(sigfrac), float(objlim), float(gain), float(readnoise),
                           float(satlevel), int(niter), int(bool(sepmed)), 0, 0)


def _refuse(inbkg, cleantype, fsmode):
    if inbkg is not None:
        raise NotImplementedError('detect_cosmics: inbkg is not built (the reference never passes a background)')
    if cleantype != 'meanmask':
        raise NotImplementedError(f"detect_cosmics: cleantype={cleantype!r} is not built, only 'meanmask'")
    if fsmode != 'median':
        raise NotImplementedError(f"detect_cosmics: fsmode={fsmode!r} is not built, only 'median'")


def lacosmic(stack, inmask=None, invar=None, sigclip=4.5, sigfrac=0.3, objlim=5.0, gain=1.0, readnoise=6.5,
             satlevel=65536.0, niter=4, sepmed=True, ctx=None):
    """One device call over a (K, n, n) stack.  Returns dict(crmask bool, clean float32 (both (K, n, n)), iters int32
    (K,) iterations done per stamp, kernel_ms device time of the kernel)."""
    ctx = ctx or _lib.default_context()
    lib = _lib.lib()
    d = f32(stack)
    if d.ndim != 3 or d.shape[1] != d.shape[2]:
        raise ValueError(f'expected a (K, n, n) stack of square stamps, got {d.shape}')
    K, n = d.shape[0], d.shape[1]
    if not lib.lc_cosmics_supported(n):
        raise _lib.LcError(f'lc_detect_cosmics takes stamps of 8 .. 128 pixels, not {n}')
    iv = f32(invar) if invar is not None else None
    m = np.ascontiguousarray(np.asarray(inmask).astype(np.uint8)) if inmask is not None else None
    if iv is not None and iv.shape != d.shape or m is not None and m.shape != d.shape:
        raise ValueError('invar / inmask must have the shape of the data')
    cr = np.empty(d.shape, np.uint8)
    clean = np.empty(d.shape, np.float32)
    iters = np.empty(K, np.int32)
    ms = C.c_float()
    cfg = _cfg(sigclip, sigfrac, objlim, gain, readnoise, satlevel, niter, sepmed)
    if K:
        ctx.check(lib.lc_detect_cosmics(ctx.h, K, n, ptr(d), ptr(iv), m.ctypes.data_as(_u8p) if m is not None else None,
                                        C.byref(cfg), cr.ctypes.data_as(_u8p), ptr(clean),
                                        iters.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms)), 'lc_detect_cosmics')
    return dict(crmask=cr.astype(bool), clean=clean, iters=iters, kernel_ms=ms.value)


def lacosmic_frames(stack, inmask=None, invar=None, sigclip=4.5, sigfrac=0.3, objlim=5.0, gain=1.0, readnoise=6.5,
                    satlevel=65536.0, niter=4, sepmed=True, scratch_frames=0, ctx=None):
    """One device call over a (K, h, w) stack of frames of any shape from 8 x 8 (``lc_detect_cosmics_frames``; DESIGN.md
    §5 "Cosmic rays of whole frames"): the SPEC with the frame as the stamp.  Only the separable medians are built:
    ``sepmed=False`` raises ``NotImplementedError``.  ``scratch_frames``: frames per chunk (0: from a budget); the result
    does not depend on it.  Returns dict(crmask bool, clean float32 (both (K, h, w)), iters int32 (K,), n_flagged int32
    (K,) pixels of crmask per frame, kernel_ms device time of all launches)."""
    if not sepmed:
        raise NotImplementedError('lacosmic_frames: only the separable medians (sepmed=True) are built for frames')
    ctx = ctx or _lib.default_context()
    lib = _lib.lib()
    d = f32(stack)
    if d.ndim != 3:
        raise ValueError(f'expected a (K, h, w) stack of frames, got {d.shape}')
    K, h, w = d.shape
    if not lib.lc_cosmics_frames_supported(h, w):
        raise _lib.LcError(f'lc_detect_cosmics_frames takes frames of h, w >= 8 with h w < 2^31, not {h} x {w}')
    iv = f32(invar) if invar is not None else None
    m = np.ascontiguousarray(np.asarray(inmask).astype(np.uint8)) if inmask is not None else None
    if iv is not None and iv.shape != d.shape or m is not None and m.shape != d.shape:
        raise ValueError('invar / inmask must have the shape of the data')
    cr = np.empty(d.shape, np.uint8)
    clean = np.empty(d.shape, np.float32)
    iters = np.empty(K, np.int32)
    flagged = np.empty(K, np.int32)
    ms = C.c_float()
    cfg = _cfg(sigclip, sigfrac, objlim, gain, readnoise, satlevel, niter, sepmed)
    i32p = C.POINTER(C.c_int32)
    if K:
        ctx.check(lib.lc_detect_cosmics_frames(
            ctx.h, K, h, w, ptr(d), ptr(iv), m.ctypes.data_as(_u8p) if m is not None else None, C.byref(cfg),
            int(scratch_frames), cr.ctypes.data_as(_u8p), ptr(clean), iters.ctypes.data_as(i32p),
            flagged.ctypes.data_as(i32p), C.byref(ms)), 'lc_detect_cosmics_frames')
    return dict(crmask=cr.astype(bool), clean=clean, iters=iters, n_flagged=flagged, kernel_ms=ms.value)


def detect_cosmics(indat, inmask=None, inbkg=None, invar=None, sigclip=4.5, sigfrac=0.3, objlim=5.0, gain=1.0,
                   readnoise=6.5, satlevel=65536.0, niter=4, sepmed=True, cleantype='meanmask', fsmode='median',
                   psfmodel='gauss', psffwhm=2.5, psfsize=7, psfk=None, psfbeta=4.765, verbose=False, ctx=None):
    """astroscrappy.detect_cosmics: returns (crmask bool, cleanarr float32) of the shape of ``indat``, one image or a
    stack of K handled in one device call.  Square stamps of 8 .. 128 pixels go to the stamp kernel (``lacosmic``), every
    other image of at least 8 x 8 pixels to the frame kernel (``lacosmic_frames``), which builds the separable medians
    only: ``sepmed=False`` raises ``NotImplementedError`` there.  The psf* arguments belong to fsmode='convolve' and are
    accepted for signature compatibility only."""
    _refuse(inbkg, cleantype, fsmode)
    d = np.asarray(indat)
    if d.ndim not in (2, 3):
        raise ValueError(f'detect_cosmics takes one (h, w) image or a (K, h, w) stack, got {d.shape}')
    shape = d.shape
    stack = d.reshape((-1,) + shape[-2:])
    stamp = shape[-2] == shape[-1] and supported(shape[-1])               # what detect_cosmics has always taken
    run = lacosmic if stamp or min(shape[-2:]) < 8 else lacosmic_frames
    r = run(stack, inmask=None if inmask is None else np.asarray(inmask).reshape(stack.shape),
            invar=None if invar is None else np.asarray(invar).reshape(stack.shape), sigclip=sigclip,
            sigfrac=sigfrac, objlim=objlim, gain=gain, readnoise=readnoise, satlevel=satlevel, niter=niter,
            sepmed=sepmed, ctx=ctx)
    return r['crmask'].reshape(shape), r['clean'].reshape(shape)
