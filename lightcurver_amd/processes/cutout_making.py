"""The reference's stamp making (lightcurver/processes/cutout_making.py) over every stamp at once.

Cutting (``extract_stamp``, :23-51, called once per stamp at :188 and :238): ``cutout_origin`` is the host arithmetic of
``Cutout2D`` on pixel positions, ``extract_stamps_batch`` cuts every stamp of one size from frames on the device with its
noise map and its mask (``lightcurver_amd.frames.FrameSet``, ``lc_frames_cut_stamps``), and
``extract_all_stamps_of_frames`` does it for the ROI and the stars of every frame of a set, one device call per stamp
size, and returns the frame groups of regions.h5.  FITS, WCS, sky -> pixel and proper motions stay with the caller:
positions are pixel positions as ``skycoord_to_pixel`` gives them, 0-based with the pixel centres at integers.

Masking (``mask_cutout``, :54-91) of stamps the caller holds: the reference runs, once per stamp, ``ccdmask(cutout,
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


def _mask_settings(params):
    """The reference's ``cosmics_masking_params`` (a dict this function empties) as the two settings structures of
    ``lc_mask_cutouts`` and ``lc_frames_cut_stamps``: (lc_cosmics_cfg, lc_ccdmask_cfg)."""
    p = dict(sigclip=4.5, sigfrac=0.3, objlim=5.0, gain=1.0, readnoise=6.5, satlevel=65536.0, niter=4, sepmed=True)
    extra = {k: params.pop(k) for k in ('inbkg', 'cleantype', 'fsmode') if k in params}
    _refuse_cosmics(extra.get('inbkg'), extra.get('cleantype', 'meanmask'), extra.get('fsmode', 'median'))
    for k in ('psfmodel', 'psffwhm', 'psfsize', 'psfk', 'psfbeta', 'verbose'):   # of fsmode='convolve': no effect
        params.pop(k, None)
    unknown = set(params) - set(p)
    if unknown:
        raise TypeError(f'mask_cutout_batch: cosmics_masking_params not taken here: {sorted(unknown)}')
    p.update(params)
    return _cosmics_cfg(**p), _ccdmask_cfg()


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
    ccfg, bcfg = _mask_settings(params)
    ctx = ctx or _lib.default_context()
    lib = _lib.lib()
    K, n = d.shape[0], d.shape[1]
    if not (lib.lc_cosmics_supported(n) and lib.lc_ccdmask_supported(n)):
        raise _lib.LcError(f'lc_mask_cutouts takes stamps of 8 .. 128 pixels, not {n}')
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


def cutout_origin(position_xy, size, frame_shape):
    """Where ``Cutout2D(frame, position, size, mode='partial')`` puts a stamp of ``size`` x ``size`` pixels (DESIGN.md
    section 5 "Stamp cutting"), in float64: x0 = ceil(x - size / 2), likewise in y; the stamp covers [x0, x0 + size) x
    [y0, y0 + size).  position_xy: (2,) or (S, 2), (x, y) with the pixel centres at integers; frame_shape: (rows,
    columns).  Returns (origin, center_original) with the shape of ``position_xy``: origin (x0, y0) as int64, and the
    centre (x, y) of the part of the stamp that lies in the frame, which the reference stores as
    ``image_pixel_coordinates``.  ValueError for a position that is not finite and for a stamp without a pixel in the
    frame (astropy's NoOverlapError is one)."""
    pos = np.asarray(position_xy, np.float64)
    if pos.shape[-1:] != (2,) or pos.ndim not in (1, 2):
        raise ValueError(f'expected positions of shape (2,) or (S, 2), got {pos.shape}')
    n = int(size)
    if n < 1 or n != size:
        raise ValueError(f'the stamp size must be a whole number >= 1, not {size!r}')
    h, w = (int(v) for v in frame_shape)
    if not np.isfinite(pos).all():
        raise ValueError('cutout_origin: a position that is not finite')
    p = pos.reshape(-1, 2)
    start = np.ceil(p - n / 2.0)                       # (x0, y0), still float64: tested before the cast
    dims = np.array([w, h], np.float64)
    if ((start + n <= 0) | (start >= dims)).any():
        raise ValueError('cutout_origin: a stamp without one pixel in the frame (no overlap)')
    origin = start.astype(np.int64)
    lo = np.maximum(origin, 0)
    hi = np.minimum(origin + n, np.array([w, h], np.int64))
    centre = 0.5 * (lo + hi - 1).astype(np.float64)
    return origin.reshape(pos.shape), centre.reshape(pos.shape)


def extract_stamps_batch(frames, frame_index, positions_xy, exptimes, background_rms, cutout_size,
                         do_mask_bad_columns=False, do_mask_cosmics=False, cosmics_masking_params=None, ctx=None):
    """The reference's ``extract_stamp`` (and ``mask_cutout``) for every stamp of one size at once.  frames: a (K, h, w)
    stack of sky-subtracted frames in electrons per second, uploaded for this call, or a ``FrameSet`` that holds them
    already; frame_index (S,), positions_xy (S, 2) pixel positions; exptimes, background_rms: one per frame, or one for
    all (None with a ``FrameSet`` that has been imported: the recorded values).  Returns the dict of
    ``FrameSet.cut_stamps``."""
    kw = dict(exptimes=exptimes, background_rms=background_rms, do_mask_bad_columns=do_mask_bad_columns,
              do_mask_cosmics=do_mask_cosmics, cosmics_masking_params=cosmics_masking_params)
    if hasattr(frames, 'cut_stamps'):
        return frames.cut_stamps(frame_index, positions_xy, cutout_size, **kw)
    from ..frames import FrameSet
    with FrameSet(frames, ctx) as fs:
        return fs.cut_stamps(frame_index, positions_xy, cutout_size, **kw)


def extract_all_stamps_of_frames(frameset, roi_xy_per_frame, stars_xy_per_frame, names_per_frame, stamp_size_ROI,
                                 stamp_size_stars, do_mask_bad_columns=False, do_mask_cosmics=False,
                                 cosmics_masking_params=None, exptimes=None, background_rms=None, image_relpaths=None):
    """The stamps the reference's ``extract_all_stamps`` writes for every frame (cutout_making.py:186-266), from a
    ``FrameSet`` (or anything with its ``shape`` and ``cut_stamps``): one device call for the ROI stamps of all frames
    and one for all star stamps.  roi_xy_per_frame: (K, 2) pixel position of the ROI in every frame;
    stars_xy_per_frame: K arrays (S_k, 2); names_per_frame: K lists of S_k star names.  exptimes, background_rms: as in
    ``FrameSet.cut_stamps``.  Returns a nested mapping {image_relpath (default: the frame's index as a string): group},
    every group laid out as a frame group of regions.h5 (``io/regions.py``): ``frame_shape`` and ``data``, ``noisemap``,
    ``cosmicsmask``, ``image_pixel_coordinates`` keyed by star name and ``'ROI'``; ``read_psf_batch`` takes it as
    ``regions``.  There is no ``wcs`` entry: the WCS of a stamp is the caller's."""
    K, h, w = frameset.shape
    roi = np.asarray(roi_xy_per_frame, np.float64).reshape(-1, 2)
    if len(roi) != K or len(stars_xy_per_frame) != K or len(names_per_frame) != K:
        raise ValueError('one ROI position, one array of star positions and one list of names per frame')
    rels = [str(k) for k in range(K)] if image_relpaths is None else [str(r) for r in image_relpaths]
    if len(rels) != K or len(set(rels)) != K:
        raise ValueError('one distinct image_relpath per frame')
    stars = [np.asarray(p, np.float64).reshape(-1, 2) for p in stars_xy_per_frame]
    names = [[str(s) for s in ids] for ids in names_per_frame]
    if any(len(p) != len(ids) for p, ids in zip(stars, names)):
        raise ValueError('one name per star position')
    kw = dict(exptimes=exptimes, background_rms=background_rms, do_mask_bad_columns=do_mask_bad_columns,
              do_mask_cosmics=do_mask_cosmics, cosmics_masking_params=cosmics_masking_params)
    out = {rel: dict(frame_shape=np.array([h, w]), data={}, noisemap={}, cosmicsmask={}, image_pixel_coordinates={})
           for rel in rels}

    def store(cut, where):
        for s, (k, name) in enumerate(where):
            g = out[rels[k]]
            g['data'][name] = cut['data'][s]
            g['noisemap'][name] = cut['noisemap'][s]
            g['cosmicsmask'][name] = cut['mask'][s]
            g['image_pixel_coordinates'][name] = cut['center_original'][s]

    store(frameset.cut_stamps(np.arange(K), roi, stamp_size_ROI, **kw), [(k, 'ROI') for k in range(K)])
    where = [(k, name) for k in range(K) for name in names[k]]
    if where:
        index = np.array([k for k, _ in where])
        store(frameset.cut_stamps(index, np.concatenate(stars), stamp_size_stars, **kw), where)
    return out
