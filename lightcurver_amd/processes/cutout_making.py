"""The cosmic half of the reference's ``mask_cutout`` (lightcurver/processes/cutout_making.py:54-91) over every stamp at
once.  Cutting the stamps (FITS, WCS, ``Cutout2D``) stays with the caller; the reference then calls
``detect_cosmics(cutout, invar=noisemap**2, **cosmics_masking_params)`` once per stamp (:85, from :194 and :247), here
all stamps of one size go through one device call (``lightcurver_amd.astroscrappy``, ``lc_detect_cosmics``).  The
result is the ``cosmicsmask`` of regions.h5 that ``lc_prepare_stamps(bad=...)``, ``prepare_psf_stamps`` and
``prepare_star_epochs`` consume."""
import numpy as np

from ..astroscrappy import detect_cosmics


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
    cutouts = [np.asarray(c, dtype=np.float32) for c in cutouts]
    noisemaps = [np.asarray(m, dtype=np.float32) for m in noisemaps]
    if len(cutouts) != len(noisemaps):
        raise ValueError('one noise map per cutout')
    out = [None] * len(cutouts)
    for shape in sorted({c.shape for c in cutouts}):
        idx = [i for i, c in enumerate(cutouts) if c.shape == shape]
        nm = np.stack([noisemaps[i] for i in idx])
        masks = detect_cosmics(np.stack([cutouts[i] for i in idx]), invar=nm ** 2, ctx=ctx, **params)[0]
        for i, m in zip(idx, masks):
            out[i] = m
    return out
