"""Calibrated cutouts of the region of interest: the numeric part of the reference's
lightcurver/processes/roi_file_preparation.py:138-201 on arrays.  The reference selects its frames with an SQL join
(:34-63), reads the stamps frame by frame from the regions file and cleans them with NumPy; here the selection is
restated on arrays and the whole stack goes through ONE ``prepare_stamps`` call (``lc_prepare_stamps``, csrc/prep.hip:
divide by the coefficient, NaN pairs to 0 / 1e7, noise x 1000 on flagged pixels, in the reference's order).  Writing the
result is ``io.regions.write_roi_file``."""
import numpy as np

from ..io.regions import rescale_image_coordinates
from ..starred.psf.psf import apply_distortion, distortion_coefficients
from .preprocessing import prepare_stamps

NAN_NOISE = 1e7        # roi_file_preparation.py:196
NOISE_BOOST = 1000.0   # roi_file_preparation.py:201


def _between(values, bounds, n, what):
    v = np.asarray(values, dtype=np.float64)
    if v.shape != (n,):
        raise ValueError(f'{what} must hold one value per frame ({n}), got {v.shape}')
    lo, hi = bounds
    with np.errstate(invalid='ignore'):
        return (v >= lo) & (v <= hi)      # SQL's BETWEEN: inclusive, false for a missing value


def select_frames(coefficient, coefficient_uncertainty=None, psf_chi2=None, psf_chi2_bounds=None, coefficient_bounds=None,
                  frame_columns=None, frame_constraints=None, mjd=None):
    """Indices of the frames ``get_frames_for_roi`` (roi_file_preparation.py:34-63) returns, in its order: a frame needs a
    (finite) normalisation coefficient, a PSF chi2 inside ``psf_chi2_bounds``, every column named in ``frame_constraints``
    ({name: (lo, hi)}, the arrays in ``frame_columns``) inside its interval, and ``coefficient_bounds`` ({'coefficient' |
    'coefficient_uncertainty': (lo, hi)}, or a bare (lo, hi) for the coefficient) likewise; then ordered by ``mjd``
    (stable) when it is given."""
    c = np.asarray(coefficient, dtype=np.float64)
    if c.ndim != 1:
        raise ValueError(f'coefficient must be (E,), got {c.shape}')
    E = c.size
    keep = np.isfinite(c)
    if psf_chi2_bounds is not None:
        if psf_chi2 is None:
            raise ValueError('psf_chi2_bounds given without psf_chi2')
        keep &= _between(psf_chi2, psf_chi2_bounds, E, 'psf_chi2')
    for name, bounds in (frame_constraints or {}).items():
        if frame_columns is None or name not in frame_columns:
            raise KeyError(f'frame_constraints names the column {name!r}, which frame_columns does not hold')
        keep &= _between(frame_columns[name], bounds, E, f'frame_columns[{name!r}]')
    if coefficient_bounds is not None:
        if not isinstance(coefficient_bounds, dict):
            coefficient_bounds = {'coefficient': coefficient_bounds}
        columns = {'coefficient': c, 'coefficient_uncertainty': coefficient_uncertainty}
        for name, bounds in coefficient_bounds.items():
            if columns.get(name) is None:
                raise KeyError(f"coefficient_bounds: unknown or missing column {name!r}; known: 'coefficient', "
                               f"'coefficient_uncertainty'")
            keep &= _between(columns[name], bounds, E, name)
    kept = np.flatnonzero(keep)
    if mjd is not None:
        t = np.asarray(mjd, dtype=np.float64)
        if t.shape != (E,):
            raise ValueError(f'mjd must hold one value per frame ({E}), got {t.shape}')
        kept = kept[np.argsort(t[kept], kind='stable')]
    return kept


def _distorted_psfs(narrow_psf, kwargs_distortion, positions, ctx):
    """The narrow PSF of every frame resampled at the ROI's position with that frame's distortion.  ``lc_apply_distortion``
    takes ONE PSF and ONE coefficient set for its K positions, and every frame has its own of both, so frames are grouped
    by (PSF, coefficients), the group's positions being the K of its call: one call per frame unless frames share a PSF model."""
    out = np.empty(narrow_psf.shape, np.float32)
    groups = {}
    for j in range(len(narrow_psf)):
        key = (narrow_psf[j].tobytes(), distortion_coefficients(kwargs_distortion[j]).tobytes())
        groups.setdefault(key, []).append(j)
    for members in groups.values():
        j0 = members[0]
        res = apply_distortion(narrow_psf=narrow_psf[j0], kwargs_distortion=kwargs_distortion[j0],
                               star_xy_coordinates=positions[members], ctx=ctx)
        out[members] = np.asarray(res).reshape(len(members), *narrow_psf.shape[1:])
    return out


def prepare_roi_cutouts(data, noisemap, cosmics_mask, narrow_psf, coefficient, coefficient_uncertainty, *, psf_chi2=None,
                        psf_chi2_bounds=None, coefficient_bounds=None, frame_columns=None, frame_constraints=None, mjd=None,
                        kwargs_distortion=None, roi_xy=None, frame_shape=None, ctx=None):
    """data, noisemap (E, n, n): the ROI stamps of all frames, in the units of the frames; cosmics_mask (E, n, n) bool,
    True = flagged; narrow_psf (E, P, P): every frame's PSF model; coefficient, coefficient_uncertainty (E,) of
    ``normalization_calculation.calculate_coefficients`` (NaN = no coefficient: the frame is dropped, as the reference's
    join drops it).  Selection and ordering: ``select_frames``.

    ``kwargs_distortion``: list of E dicts (``build_psf(field_distortion=True)``); the PSFs are then resampled at the ROI's
    position ``rescale_image_coordinates(roi_xy, frame_shape)`` (roi_xy (2,) or (E, 2) frame pixels (x, y), frame_shape (2,)
    or (E, 2) (rows, columns)), :169-180.

    Returns dict: data, noisemap (K, n, n) float32 divided by the coefficient and cleaned, mask (K, n, n) bool True = good,
    psf (K, P, P), relative_normalization_error (K,) = the kept frames' coefficient_uncertainty (:190, 225), kept (K,)
    indices into the input, in the output's order, and mjd (K,) when it was given.  There is no host fall-back for the
    stamps or the resampling."""
    data, noisemap = np.asarray(data), np.asarray(noisemap)
    bad = np.asarray(cosmics_mask).astype(bool)
    narrow_psf = np.asarray(narrow_psf)
    E = data.shape[0]
    if data.ndim != 3 or noisemap.shape != data.shape or bad.shape != data.shape:
        raise ValueError('data, noisemap and cosmics_mask must be (E, n, n) stacks of one shape')
    if narrow_psf.ndim != 3 or narrow_psf.shape[0] != E:
        raise ValueError(f'narrow_psf must be (E, P, P) with E = {E}, got {narrow_psf.shape}')
    coefficient = np.asarray(coefficient, dtype=np.float64)
    uncertainty = np.asarray(coefficient_uncertainty, dtype=np.float64)
    if coefficient.shape != (E,) or uncertainty.shape != (E,):
        raise ValueError(f'coefficient and coefficient_uncertainty must be ({E},)')
    kept = select_frames(coefficient, uncertainty, psf_chi2, psf_chi2_bounds, coefficient_bounds, frame_columns,
                         frame_constraints, mjd)
    if kept.size == 0:
        raise ValueError('no frame passes the selection')
    psf = narrow_psf[kept]
    if kwargs_distortion is not None:
        if len(kwargs_distortion) != E or roi_xy is None or frame_shape is None:
            raise ValueError('kwargs_distortion needs one dict per frame, roi_xy and frame_shape')
        xy = np.broadcast_to(np.asarray(roi_xy, dtype=np.float64), (E, 2))
        shapes = np.broadcast_to(np.asarray(frame_shape, dtype=np.float64), (E, 2))
        positions = np.stack([rescale_image_coordinates(xy[j], shapes[j]) for j in kept])
        psf = _distorted_psfs(np.ascontiguousarray(psf), [kwargs_distortion[j] for j in kept], positions, ctx)
    stamps = prepare_stamps(data[kept], noisemap[kept], coefficient=coefficient[kept], bad=bad[kept], nan_noise=NAN_NOISE,
                            noise_boost=NOISE_BOOST, boost_whole_stamp=False, ctx=ctx, want=('data', 'noisemap'))
    out = dict(data=stamps['data'], noisemap=stamps['noisemap'], mask=~bad[kept], psf=psf,
               relative_normalization_error=uncertainty[kept], kept=kept)
    if mjd is not None:
        out['mjd'] = np.asarray(mjd, dtype=np.float64)[kept]
    return out
