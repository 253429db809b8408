"""``ccdmask`` with ccdproc's signature, on the device (``lc_ccdmask_stamps``, include/lcmi.h).

With ``mask_bad_rows_and_columns`` set (config.yaml:208) the reference runs ``ccdproc.ccdmask(ccd, findbadcolumns=True)``
on every stamp it cuts and keeps the lines that reach both ends of the stamp (lightcurver/processes/cutout_making.py:67-80).
Here the SPEC of DESIGN.md §5 ("Bad rows and columns") runs as one HIP kernel over a whole stack of stamps: a 2-D input
is one stamp, a (K, n, n) stack is one batched call.  Only ``byblocks=False`` with the 7 x 7 median window on square
stamps is built (what the reference uses); anything else raises ``NotImplementedError``.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import f32, ptr

_u8p = C.POINTER(C.c_uint8)


def supported(n):
    """True if the kernel takes n x n stamps (8 .. 128)."""
    return bool(_lib.lib().lc_ccdmask_supported(int(n)))


def _cfg(ncmed=7, nlmed=7, lsigma=9, hsigma=9, ngood=5, byblocks=False, findbadcolumns=True):
    return _lib.CcdmaskCfg(int(ncmed), int(nlmed), float(lsigma), float(hsigma), int(ngood), int(bool(byblocks)),
                           int(bool(findbadcolumns)))


def _refuse(shape, byblocks, ncmed, nlmed):
    if byblocks:
        raise NotImplementedError('ccdmask: byblocks=True is not built (the reference never sets it)')
    if (int(ncmed), int(nlmed)) != (7, 7):
        raise NotImplementedError(f'ccdmask: a {nlmed} x {ncmed} median window is not built, only 7 x 7')
    if shape[-1] != shape[-2]:
        raise NotImplementedError(f'ccdmask: rectangular stamps are not built, got {tuple(shape[-2:])}')


def ccdmask_stamps(stack, findbadcolumns=True, byblocks=False, ncmed=7, nlmed=7, lsigma=9, hsigma=9, ngood=5, ctx=None):
    """One device call over a (K, n, n) stack.  Returns dict(mask bool (K, n, n) the ccdmask result, bad_cols and
    bad_rows bool (K, n) the columns / rows flagged at both ends, rowcol bool (K, n, n) those lines whole, sigma float32
    (K,), kernel_ms device time of the kernel)."""
    d = f32(stack)
    if d.ndim != 3:
        raise ValueError(f'expected a (K, n, n) stack of square stamps, got {d.shape}')
    _refuse(d.shape, byblocks, ncmed, nlmed)
    ctx = ctx or _lib.default_context()
    lib = _lib.lib()
    K, n = d.shape[0], d.shape[1]
    if not lib.lc_ccdmask_supported(n):
        raise _lib.LcError(f'lc_ccdmask_stamps takes stamps of 8 .. 128 pixels, not {n}')
    mask, rowcol = np.zeros(d.shape, np.uint8), np.zeros(d.shape, np.uint8)
    cols, rows = np.zeros((K, n), np.uint8), np.zeros((K, n), np.uint8)
    sigma = np.zeros(K, np.float32)
    ms = C.c_float()
    cfg = _cfg(ncmed, nlmed, lsigma, hsigma, ngood, byblocks, findbadcolumns)
    if K:
        ctx.check(lib.lc_ccdmask_stamps(ctx.h, K, n, ptr(d), C.byref(cfg), mask.ctypes.data_as(_u8p),
                                        rowcol.ctypes.data_as(_u8p), cols.ctypes.data_as(_u8p),
                                        rows.ctypes.data_as(_u8p), ptr(sigma), C.byref(ms)), 'lc_ccdmask_stamps')
    return dict(mask=mask.astype(bool), rowcol=rowcol.astype(bool), bad_cols=cols.astype(bool),
                bad_rows=rows.astype(bool), sigma=sigma, kernel_ms=ms.value)


def ccdmask(ratio, findbadcolumns=False, byblocks=False, ncmed=7, nlmed=7, ncsig=15, nlsig=15, lsigma=9, hsigma=9,
            ngood=5, ctx=None):
    """ccdproc.ccdmask: returns the bool mask (True = bad) of the shape of ``ratio``, either one (n, n) stamp or a
    (K, n, n) stack handled in one device call.  ncsig / nlsig belong to byblocks=True and are accepted for signature
    compatibility only."""
    d = np.asarray(ratio)
    if d.ndim not in (2, 3):
        raise ValueError(f'ccdmask takes one (n, n) stamp or a (K, n, n) stack, got {d.shape}')
    _refuse(d.shape, byblocks, ncmed, nlmed)
    shape = d.shape
    r = ccdmask_stamps(d.reshape((-1,) + shape[-2:]), findbadcolumns=findbadcolumns, byblocks=byblocks, ncmed=ncmed,
                       nlmed=nlmed, lsigma=lsigma, hsigma=hsigma, ngood=ngood, ctx=ctx)
    return r['mask'].reshape(shape)
