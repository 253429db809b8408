"""The reference's ``mask_cutout`` (lightcurver/processes/cutout_making.py:54-91) over every stamp at once.  Cutting the
stamps (FITS, WCS, ``Cutout2D``) stays with the caller; the reference then runs, once per stamp, ``ccdmask(cutout,
findbadcolumns=True)`` reduced to the rows and columns flagged at both ends (:67-80, when ``mask_bad_rows_and_columns``
is set) and ``detect_cosmics(cutout, invar=noisemap**2, **cosmics_masking_params)`` (:85, from :194 and :247).  Here
all stamps of one size go through one device call: ``mask_cutout_batch`` (both halves, ``lc_mask_cutouts``) or
``mask_cosmics_batch`` (the cosmics alone, ``lightcurver_amd.astroscrappy``, ``lc_detect_cosmics``).  The result is the
``cosmicsmask`` of regions.h5 that ``lc_prepare_stamps(bad=...)``, ``prepare_psf_stamps`` and ``prepare_star_epochs``
consume."""
import ctypes as C

import numpy as np

from . import per_shape
from .. import _lib
from ..astroscrappy import _cfg as _cosmics_cfg, _refuse as _refuse_cosmics, detect_cosmics
from ..ccdproc import _cfg as _ccdmask_cfg


def mask_cosmics_batch(cutouts, noisemaps, cosmics_masking_params=None, do_mask_bad_columns=False, ctx=None):
    """cutouts, noisemaps: a (K, n, n) stack each, or equal-length lists of square stamps (sizes may differ, e.g. the
    ROI and the stars of a frame: one call per size).  cosmics_masking_params: astroscrappy arguments as in the
    reference's config (``cosmics_masking_params``).  Returns the masks, True = cosmic, as a (K, n, n) array for a
    stack input and as a list otherwise."""
    if do_mask_bad_columns:
        raise NotImplementedError("mask_cosmics_batch: the bad row / column mask (ccdproc's ccdmask, "
                                  "cutout_making.py:67-80) is not built; only the cosmics are masked here")
    params = dict(cosmics_masking_params or {})
    if isinstance(cutouts, np.ndarray) and cutouts.ndim == 3:
        nm = np.asarray(noisemaps, dtype=np.float32)
        return detect_cosmics(np.asarray(cutouts, dtype=np.float32), invar=nm ** 2, ctx=ctx, **params)[0]
    return per_shape(lambda d, nm: detect_cosmics(d, invar=nm ** 2, ctx=ctx, **params)[0], cutouts, noisemaps)


def _mask_cutouts(d, nm, do_bad_columns, do_cosmics, params, ctx):
    """One lc_mask_cutouts call over a (K, n, n) stack."""
    d, nm = _lib.f32(d), _lib.f32(nm)
    if d.ndim != 3 or d.shape[1] != d.shape[2]:
        raise ValueError(f'expected a (K, n, n) stack of square stamps, got {d.shape}')
    if nm.shape != d.shape:
        raise ValueError('the noise maps must have the shape of the cutouts')
    mask = np.zeros(d.shape, np.uint8)
    if not (do_bad_columns or do_cosmics) or not len(d):
        return mask.astype(bool)
    p = dict(sigclip=4.5, sigfrac=0.3, objlim=5.0, gain=1.0, readnoise=6.5, satlevel=65536.0, niter=4, sepmed=True)
    extra = {k: params.pop(k) for k in ('inbkg', 'cleantype', 'fsmode') if k in params}
    _refuse_cosmics(extra.get('inbkg'), extra.get('cleantype', 'meanmask'), extra.get('fsmode', 'median'))
    for k in ('psfmodel', 'psffwhm', 'psfsize', 'psfk', 'psfbeta', 'verbose'):   # of fsmode='convolve': no effect
        params.pop(k, None)
    unknown = set(params) - set(p)
    if unknown:
        raise TypeError(f'mask_cutout_batch: cosmics_masking_params not taken here: {sorted(unknown)}')
    p.update(params)
    ctx = ctx or _lib.default_context()
    lib = _lib.lib()
    K, n = d.shape[0], d.shape[1]
    if not (lib.lc_cosmics_supported(n) and lib.lc_ccdmask_supported(n)):
        raise _lib.LcError(f'lc_mask_cutouts takes stamps of 8 .. 128 pixels, not {n}')
    ccfg, bcfg = _cosmics_cfg(**p), _ccdmask_cfg()
    ctx.check(lib.lc_mask_cutouts(ctx.h, K, n, _lib.ptr(d), _lib.ptr(nm), int(bool(do_bad_columns)),
                                  int(bool(do_cosmics)), C.byref(ccfg), C.byref(bcfg),
                                  mask.ctypes.data_as(C.POINTER(C.c_uint8)), None), 'lc_mask_cutouts')
    return mask.astype(bool)


def mask_cutout_batch(cutouts, noisemaps, do_mask_bad_columns, do_mask_cosmics, cosmics_masking_params=None, ctx=None):
    """The reference's ``mask_cutout`` with its argument names, over every stamp at once.  cutouts, noisemaps: a
    (K, n, n) stack each, or equal-length lists of square stamps (sizes may differ: one device call per size).
    do_mask_bad_columns: the rows and columns that ccdmask(findbadcolumns=True) flags at both ends of the stamp;
    do_mask_cosmics: detect_cosmics(invar=noisemap**2, **cosmics_masking_params).  Returns the OR of the two, True =
    masked, as a (K, n, n) array for a stack input and as a list otherwise; all False without a device call when both
    switches are off."""
    params = dict(cosmics_masking_params or {})
    if isinstance(cutouts, np.ndarray) and cutouts.ndim == 3:
        return _mask_cutouts(cutouts, noisemaps, do_mask_bad_columns, do_mask_cosmics, params, ctx)
    return per_shape(lambda d, nm: _mask_cutouts(d, nm, do_mask_bad_columns, do_mask_cosmics, dict(params), ctx),
                     cutouts, noisemaps)
