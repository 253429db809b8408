"""From raw frames to calibrated light curves in one call: the stages of the reference's pipeline
(pipeline_dependency_graph.yaml: importation, plate solving, footprints, star selection, stamp extraction, PSF modelling,
star photometry, normalisation, zero-points, ROI preparation, ROI modelling) joined on arrays.  Every stage is a public
function of this package called as a user would call it (DESIGN.md section 5 "From frames to light curves" lists the
conventions at each joint); the driver adds no numerics of its own, only the bookkeeping between the stages: which frame
survives and why, which star is in which frame, and the scatter of stamps into per-frame and per-star stacks.  There is no
database, no FITS and no plot; catalogue magnitudes are passed in."""
import time

import numpy as np

from . import _lib
from .utilities.chi2_selector import get_chi2_bounds
from .utilities.footprint import (bad_pointings, common_footprint, frame_angles, frame_footprints, frame_scales,
                                  points_in_footprints, total_bounds)

STRATEGIES = ('stars_per_frame', 'common_footprint_stars')
MAX_PSF_STARS = 16            # the most stars of a frame the PSF fit takes
MIN_FRAMES = 3


class _FrameSubset:
    """Some frames of a ``FrameSet``, numbered 0 .. len - 1, with the ``shape`` and ``cut_stamps`` that
    ``extract_all_stamps_of_frames`` asks of its frame set."""

    def __init__(self, frameset, frames):
        self.frameset, self.frames = frameset, np.asarray(frames, dtype=np.int64)
        self.shape = (len(self.frames),) + tuple(frameset.shape[1:])

    def cut_stamps(self, frame_index, positions_xy, size, **kw):
        return self.frameset.cut_stamps(self.frames[np.asarray(frame_index, dtype=np.int64)], positions_xy, size, **kw)


def _check_stamp_sizes(stamp_size_stars, stamp_size_ROI, ss, masks):
    """ValueError for a stamp size that no kernel or embedding takes; asks the library, launches nothing."""
    from .joint import joint_fit_size
    from .starred.procedures.psf_routines import _fit_size
    if ss not in (1, 2):
        raise ValueError(f'subsampling_factor must be 1 or 2, not {ss!r}')
    lib = _lib.lib()
    for name, n, checks in (('stamp_size_stars', stamp_size_stars, (_fit_size, joint_fit_size)),
                            ('stamp_size_ROI', stamp_size_ROI, (joint_fit_size,))):
        if n != int(n) or int(n) < 1:
            raise ValueError(f'{name} must be a whole number of pixels, not {n!r}')
        try:
            for check in checks:
                check(int(n), ss)
        except _lib.LcError as e:
            raise ValueError(f'{name} = {n}: {e}') from None
        if not lib.lc_cutout_supported(int(n), int(masks)):
            raise ValueError(f'{name} = {n}: stamps are cut with their masks at 8 .. 128 pixels')


def light_curves_from_frames(frames, exptimes, roi_xy, point_sources_xy, *, reference=0, mjd=None, catalog_mags=None,
                             star_catalogue=None, star_selection_strategy='stars_per_frame', footprint_margin=None,
                             roi_exclusion_radius=None, stars_to_use_psf=None, stars_to_use_norm=None,
                             stars_to_exclude_psf=None, stars_to_exclude_norm=None, stamp_size_stars=24, stamp_size_ROI=32,
                             mask_bad_rows_and_columns=True, clean_cosmics=True, cosmics_masking_params=None,
                             subsampling_factor=2, psf_n_iter_analytic=100, psf_n_iter_pixels=3000,
                             psf_fit_exclude_strategy=None, star_deconv_n_iter=2000,
                             star_photometry_uniform_background_per_epoch=False,
                             star_photometry_starlet_global_background=False, fluxes_fit_exclude_strategy=None,
                             constraints_on_frame_columns_for_roi=None, constraints_on_normalization_coeff=None,
                             fix_point_source_astrometry=False, starting_background=None, further_optimize_background=True,
                             roi_model_regularization=None, roi_deconv_translations_iters=300, roi_deconv_all_iters=2000,
                             max_scale_deviation=0.02, import_options=None, star_catalogue_from='reference',
                             coadd_order=3, coadd_combine=None, ctx=None):
    """frames: a (K, h, w) array in electrons per second, NOT sky-subtracted, or a ``FrameSet`` that has not been imported
    (it is imported here and stays open; an array is uploaded to a set of its own, closed on return).  exptimes: one per
    frame, or one for all.  roi_xy (2,) and point_sources_xy (M, 2): pixel positions (x, y) in frame ``reference``,
    0-based with the pixel centres at integers.  mjd (K,): orders the frames of the light curves.  Frames keep the
    caller's numbering in everything returned.  Keyword names and defaults are those of the reference's config.yaml
    wherever it has the key (INTEGRATION.md gives the table); the others:

    * ``star_catalogue``: a record array as ``processes.star_selection.reference_star_catalogue`` returns it (name, x, y,
      flux, distance_to_roi; reference pixels), for a caller who has a real catalogue; by default it is built from the
      reference frame's own sources, those within ``roi_exclusion_radius`` pixels of the ROI dropped (default: half the
      ROI stamp).  ``catalog_mags``: one calibrated magnitude per star of ``star_catalogue``, which it therefore needs.
    * ``star_catalogue_from``: where the catalogue comes from when ``star_catalogue`` is None.  'reference': the sources
      of the reference frame, as above.  'coadd': the sources of the co-add of the frames that pass stage 3
      (``processes.coaddition.coadd_frames`` on the reference frame's grid with ``relative_flux_scales`` and the weights
      1 / (scale rms)^2, interpolation ``coadd_order``; ``coadd_combine`` None means 'median' below 11 frames, where the
      deviation of so few samples says little, and 'sigma_clip' from 11 on), extracted with ``extract_stars`` at the variance
      1 / weight: deeper than one frame by about the root of their number, without cosmic rays, and not tied to what
      the reference frame happened to detect.  The co-add is returned as ``coadd`` and timed as ``seconds['coadd']``.
    * ``star_selection_strategy``: 'stars_per_frame' (every frame uses the stars inside its own footprint) or
      'common_footprint_stars' (only stars that are in every surviving frame).  ``footprint_margin``: pixels a star must
      keep from a frame's edge (``points_in_footprints``; the reference's 4 arcseconds; default: half the star stamp).
    * ``max_scale_deviation``: a frame whose registration has a scale further than this from 1 is dropped: the joint
      model has no scale.  ``import_options``: keyword arguments of ``FrameSet.import_frames``.

    Stages: 1 ``FrameSet.import_frames``, the sources table, seeing and ellipticity of every frame;
    2 ``register_frames`` against ``reference``; 3 elimination - 'registration', 'scale', 'bad_pointing'
    (``bad_pointings``), 'roi_not_in_footprint' (the ROI with a margin of half its stamp); 4 the star catalogue and the
    stars-in-frames table; 5 ``positions_in_frames`` and ``extract_all_stamps_of_frames`` on the surviving frames: one cut
    for the ROI stamps, one for all star stamps; 6 per frame ``select_stars(..., stars_to_use_psf, stars_to_exclude_psf,
    available=row)``, at most 16, and ``model_psfs_of_frames(mask_neighbours=True)`` with the frame's seeing: a frame
    without a result is eliminated as 'no_psf'; 7 per normalisation star (``stars_to_use_norm``, ``_exclude_norm``) the
    frames where it is in the table and whose PSF chi2 is inside ``get_chi2_bounds(psf_chi2, psf_fit_exclude_strategy)``,
    cleaned with ``prepare_star_epochs``, each epoch with its frame's ``narrow_psf``; 8 ``calibrated_light_curves`` with
    ``angles_to_north = frame_angles(results)`` and the point sources given per frame, in the pixels of that frame's ROI
    stamp (position in the frame minus the stamp's origin), of which it takes the first kept frame's.

    Returns the dict of ``calibrated_light_curves`` (its nested products, ``prepared['kept']`` among them, number the
    frames 0 .. n - 1 over ``frames_fitted``) with ``kept`` in the caller's numbering, plus: eliminated {frame: reason},
    frames_fitted (the frames that reached stage 8), registration (the list of ``register_frames``), footprints (K, 4, 2),
    common_footprint (of the frames that passed stage 3; (V, 2) or None), total_bounds, stars (the catalogue in use),
    stars_in_frames (K, S) bool, psf_stars {frame: names}, normalization_stars (names), star_frame_index (per
    normalisation star, frames in the caller's numbering), sources_tables, psf_results (K, None where there is none),
    psf_chi2 (K,), seeing_pixels (K,), ellipticity (K,), background_rms (K,), angles (K,) degrees, scales (K,), roi_origin
    (K, 2) int (x0, y0) of the ROI stamps (-1 where none was cut), point_sources_in_stamps (K, M, 2), seconds {stage: wall
    clock}; with the catalogue taken from the co-add also coadd: the dict of ``coadd_frames`` plus its ``sources_table``.

    ValueError, before anything runs on the device, for shapes that do not match, a frame set that was imported already,
    fewer than 3 frames, a ROI outside the reference frame, and a stamp size no kernel or embedding takes; and as soon as
    they are known, before any stamp is cut or fitted, for fewer than 3 surviving frames and for a selection that leaves
    no star.

    Memory: all frames live in one ``FrameSet``, K h w 4 bytes on the device, and during the import the raw planes, the
    sky-subtracted planes and four planes of scratch beside them (2 K h w 4 + 4 h w 4 bytes); the host holds the caller's
    array and a float32 copy.  A set that does not fit is the caller's to split; chunked import is not built."""
    from . import sep
    from .frames import FrameSet
    from .processes.calibration import calibrated_light_curves
    from .processes.coaddition import coadd_frames, relative_flux_scales
    from .processes.cutout_making import cutout_origin, extract_all_stamps_of_frames
    from .processes.frame_characterization import estimate_seeing
    from .processes.plate_solving import positions_in_frames, register_frames
    from .processes.psf_modelling import model_psfs_of_frames
    from .processes.star_extraction import extract_stars, sources_table_from_objects
    from .processes.star_photometry import prepare_star_epochs
    from .processes.star_selection import reference_star_catalogue, select_stars

    # ---- refusals that need no device ------------------------------------------------------------------------------
    own_set = not hasattr(frames, 'import_frames')
    shape = tuple(np.shape(frames)) if own_set else tuple(frames.shape)
    if len(shape) != 3 or 0 in shape:
        raise ValueError(f'expected (K, h, w) frames, got {shape}')
    K, h, w = shape
    if K < MIN_FRAMES:
        raise ValueError(f'{K} frames: a light curve needs at least {MIN_FRAMES} surviving frames')
    t = np.asarray(exptimes, np.float64).reshape(-1)
    if t.size not in (1, K):
        raise ValueError(f'exptimes must hold one value, or one per frame ({K}), got {t.size}')
    t = np.broadcast_to(t, (K,))
    if not (np.isfinite(t) & (t > 0)).all():
        raise ValueError('exposure times must be finite and > 0')
    if mjd is not None and np.shape(mjd) != (K,):
        raise ValueError(f'mjd must hold one value per frame ({K}), got {np.shape(mjd)}')
    if not isinstance(reference, (int, np.integer)) or not 0 <= reference < K:
        raise ValueError(f'reference must be a frame index in 0 .. {K - 1}, not {reference!r}')
    roi = np.asarray(roi_xy, np.float64)
    if roi.shape != (2,) or not np.isfinite(roi).all():
        raise ValueError(f'roi_xy must be one finite (x, y), got shape {roi.shape}')
    if not (0 <= roi[0] <= w - 1 and 0 <= roi[1] <= h - 1):
        raise ValueError(f'roi_xy = {tuple(roi)} is outside the reference frame ({h} x {w} pixels)')
    sources = np.asarray(point_sources_xy, np.float64)
    if sources.ndim != 2 or sources.shape[1] != 2 or not len(sources) or not np.isfinite(sources).all():
        raise ValueError(f'point_sources_xy must be (M, 2) finite positions with M >= 1, got shape {sources.shape}')
    M = len(sources)
    if star_selection_strategy not in STRATEGIES:
        raise ValueError(f'star_selection_strategy must be one of {STRATEGIES}, not {star_selection_strategy!r}')
    ss = subsampling_factor
    masks = bool(mask_bad_rows_and_columns or clean_cosmics)
    _check_stamp_sizes(stamp_size_stars, stamp_size_ROI, ss, masks)
    n_star, n_roi, ss = int(stamp_size_stars), int(stamp_size_ROI), int(ss)
    if star_catalogue is not None:
        names = getattr(np.asarray(star_catalogue).dtype, 'names', None) or ()
        if not {'name', 'x', 'y', 'distance_to_roi'} <= set(names):
            raise ValueError('star_catalogue must be a record array as reference_star_catalogue returns it')
        if catalog_mags is not None and np.shape(catalog_mags) != np.shape(star_catalogue):
            raise ValueError('catalog_mags must hold one magnitude per star of star_catalogue')
        if not len(star_catalogue):
            raise ValueError('star_catalogue holds no star')
    elif catalog_mags is not None:
        raise ValueError('catalog_mags needs star_catalogue: the magnitudes go with its stars, one each')
    if not own_set and frames.imported:
        raise ValueError('the frame set has been imported already: its planes no longer hold the frames')
    if star_catalogue_from not in ('reference', 'coadd'):
        raise ValueError(f"star_catalogue_from must be 'reference' or 'coadd', not {star_catalogue_from!r}")
    if coadd_order not in (1, 3):
        raise ValueError(f'coadd_order must be 1 or 3, not {coadd_order!r}')
    if coadd_combine not in (None,) + tuple(_lib.COADD_COMBINE):
        raise ValueError(f'coadd_combine must be None or one of {tuple(_lib.COADD_COMBINE)}, not {coadd_combine!r}')
    margin = n_star / 2.0 if footprint_margin is None else float(footprint_margin)
    exclusion = n_roi / 2.0 if roi_exclusion_radius is None else float(roi_exclusion_radius)

    seconds, eliminated = {}, {}
    clock = time.perf_counter()

    def lap(stage):
        nonlocal clock
        now = time.perf_counter()
        seconds[stage] = now - clock
        clock = now

    fs = FrameSet(frames, ctx) if own_set else frames
    try:
        # ---- 1 import ------------------------------------------------------------------------------------------------
        imported = fs.import_frames(np.asarray(t, np.float32), **dict(import_options or {}))
        tables = []
        for k in range(K):
            if int(imported['ex_status'][k]) == 2:
                raise _lib.LcError(f'frame {k}: the iteration guard of the labelling was reached')
            tables.append(sources_table_from_objects(sep.objects_view(imported['objects'][k])))
        seeing = np.array([float(estimate_seeing(tab)) for tab in tables])
        with np.errstate(all='ignore'):
            ellipticity = np.array([float(np.nanmedian(tab['ellipticity'])) if len(tab) else np.nan for tab in tables])
        background_rms = np.asarray(imported['globalrms'], np.float64)
        lap('import')

        # ---- 2 registration ------------------------------------------------------------------------------------------
        results = register_frames(tables, reference=int(reference), ctx=ctx)
        lap('registration')

        # ---- 3 elimination -------------------------------------------------------------------------------------------
        footprints = frame_footprints(results, (h, w))
        angles, scales = frame_angles(results), frame_scales(results)
        for k in range(K):
            if not results[k]['success']:
                eliminated[k] = 'registration'
            elif abs(scales[k] - 1.0) > max_scale_deviation:
                eliminated[k] = 'scale'
        remaining = np.where(np.isin(np.arange(K), list(eliminated))[:, None, None], np.nan, footprints)
        for k in np.flatnonzero(bad_pointings(remaining)):
            eliminated[int(k)] = 'bad_pointing'
        roi_inside = points_in_footprints(roi, footprints, n_roi / 2.0)[:, 0]
        for k in range(K):
            if k not in eliminated and not roi_inside[k]:
                eliminated[k] = 'roi_not_in_footprint'
        alive = np.array([k for k in range(K) if k not in eliminated], dtype=np.int64)
        if len(alive) < MIN_FRAMES:
            raise ValueError(f'{len(alive)} of {K} frames survive ({eliminated}): a light curve needs at least {MIN_FRAMES}')
        common = common_footprint(footprints[alive])

        # ---- 4 stars -------------------------------------------------------------------------------------------------
        coadd = None
        if star_catalogue is None and star_catalogue_from == 'coadd':
            began = time.perf_counter()
            coadd = coadd_frames(fs, results, alive, flux_scale=relative_flux_scales(tables, results, int(reference)),
                                 order=int(coadd_order),
                                 combine=coadd_combine or ('median' if len(alive) < 11 else 'sigma_clip'))
            with np.errstate(divide='ignore'):
                coadd['sources_table'] = extract_stars(coadd['image'], 1.0 / coadd['weight'], ctx=ctx)
            stars = reference_star_catalogue(coadd['sources_table'], roi, exclusion)
            mags = None
            seconds['coadd'] = time.perf_counter() - began
            clock += seconds['coadd']                                      # not part of the lap that follows
        elif star_catalogue is None:
            stars = reference_star_catalogue(tables[int(reference)], roi, exclusion)
            mags = None
        else:
            stars = np.asarray(star_catalogue)
            mags = None if catalog_mags is None else np.asarray(catalog_mags, np.float64)
        stars_xy = np.stack([stars['x'], stars['y']], axis=1).astype(np.float64).reshape(-1, 2)
        in_frames = points_in_footprints(stars_xy, footprints, margin) if len(stars) else np.zeros((K, 0), bool)
        if star_selection_strategy == 'common_footprint_stars':
            everywhere = in_frames[alive].all(axis=0)
            stars, stars_xy, in_frames = stars[everywhere], stars_xy[everywhere], in_frames[:, everywhere]
            mags = None if mags is None else mags[everywhere]
        norm_stars = select_stars(stars, stars_to_use_norm, stars_to_exclude_norm)
        norm_stars = norm_stars[in_frames[alive][:, norm_stars].any(axis=0)] if len(norm_stars) else norm_stars
        psf_stars = {int(k): select_stars(stars, stars_to_use_psf, stars_to_exclude_psf, available=in_frames[k])[:MAX_PSF_STARS]
                     for k in alive}
        if not len(stars) or not len(norm_stars) or not any(len(v) for v in psf_stars.values()):
            raise ValueError(f'the star selection leaves no star ({len(stars)} in the catalogue, {len(norm_stars)} for the '
                             f'normalisation, {sum(len(v) for v in psf_stars.values())} PSF stamps over all frames)')
        lap('footprints_and_stars')

        # ---- 5 stamps ------------------------------------------------------------------------------------------------
        roi_in_frames = positions_in_frames(results, roi[None])                       # per frame (1, 2)
        stars_in_each = positions_in_frames(results, stars_xy)                        # per frame (S, 2)
        sources_in_frames = positions_in_frames(results, sources)                     # per frame (M, 2)
        cut = [np.flatnonzero(in_frames[k] & (np.isin(np.arange(len(stars)), psf_stars[int(k)])
                                              | np.isin(np.arange(len(stars)), norm_stars))) for k in alive]
        regions = extract_all_stamps_of_frames(
            _FrameSubset(fs, alive), np.stack([roi_in_frames[k][0] for k in alive]),
            [stars_in_each[k][idx] for k, idx in zip(alive, cut)], [list(stars['name'][idx]) for idx in cut], n_roi, n_star,
            do_mask_bad_columns=bool(mask_bad_rows_and_columns), do_mask_cosmics=bool(clean_cosmics),
            cosmics_masking_params=cosmics_masking_params, image_relpaths=[str(int(k)) for k in alive])
        roi_origin = np.full((K, 2), -1, dtype=np.int64)
        in_stamps = np.full((K, M, 2), np.nan)
        for k in alive:
            roi_origin[k] = cutout_origin(roi_in_frames[k][0], n_roi, (h, w))[0]
            in_stamps[k] = sources_in_frames[k] - roi_origin[k]
        lap('stamps')

        # ---- 6 PSFs --------------------------------------------------------------------------------------------------
        def stamps_of(k, idx, key):
            group = regions[str(int(k))][key]
            return np.stack([group[name] for name in stars['name'][idx]]) if len(idx) else np.zeros((0, n_star, n_star), np.float32)

        psf_frames = [dict(id=int(k), datas=stamps_of(k, psf_stars[int(k)], 'data'),
                           noisemaps=stamps_of(k, psf_stars[int(k)], 'noisemap'),
                           cosmics_masks=stamps_of(k, psf_stars[int(k)], 'cosmicsmask').astype(bool),
                           seeing_pixels=seeing[k] if seeing[k] > 0 else 3.0) for k in alive]
        fitted = model_psfs_of_frames(psf_frames, ss, psf_n_iter_analytic, psf_n_iter_pixels, mask_neighbours=True,
                                      **({} if ctx is None else {'ctx': ctx}))
        psf_results = [None] * K
        psf_chi2 = np.full(K, np.nan)
        for k, (_, res) in zip(alive, fitted):
            if res is None:
                eliminated[int(k)] = 'no_psf'
            else:
                psf_results[k], psf_chi2[k] = res, res['chi2']
        final = np.array([k for k in alive if k not in eliminated], dtype=np.int64)
        if len(final) < MIN_FRAMES:
            raise ValueError(f'{len(final)} of {K} frames survive ({eliminated}): a light curve needs at least {MIN_FRAMES}')
        lap('psf')

        # ---- 7 star stacks -------------------------------------------------------------------------------------------
        lo, hi = get_chi2_bounds(psf_chi2[final], psf_fit_exclude_strategy)
        with np.errstate(invalid='ignore'):
            usable = (psf_chi2[final] >= lo) & (psf_chi2[final] <= hi)
        star_stacks, star_frame_index, used = [], [], []
        for g in norm_stars:
            rows = np.flatnonzero(in_frames[final, g] & usable)                        # numbered over ``final``
            if not len(rows):
                continue
            name = stars['name'][g]
            data, noisemap = prepare_star_epochs(
                np.stack([regions[str(int(final[j]))]['data'][name] for j in rows]),
                np.stack([regions[str(int(final[j]))]['noisemap'][name] for j in rows]),
                np.stack([regions[str(int(final[j]))]['cosmicsmask'][name] for j in rows]))
            star_stacks.append((data, noisemap, np.stack([psf_results[final[j]]['narrow_psf'] for j in rows])))
            star_frame_index.append(rows)
            used.append(int(g))
        if not star_stacks:
            raise ValueError('no normalisation star has a frame with a usable PSF')
        roi_stack = tuple(np.stack([regions[str(int(k))][key]['ROI'] for k in final])
                          for key in ('data', 'noisemap', 'cosmicsmask')) + \
            (np.stack([psf_results[k]['narrow_psf'] for k in final]),)
        lap('star_stacks')

        # ---- 8 the calibration chain ---------------------------------------------------------------------------------
        columns = dict(seeing_pixels=seeing[final], ellipticity=ellipticity[final], background_rms=background_rms[final],
                       psf_chi2=psf_chi2[final], angle=angles[final], scale=scales[final], exptime=np.asarray(t)[final])
        out = calibrated_light_curves(
            star_stacks, roi_stack, ss, in_stamps[final, :, 0], in_stamps[final, :, 1], star_frame_index=star_frame_index,
            n_frames=len(final), catalog_mags=None if mags is None else mags[used],
            mjd=None if mjd is None else np.asarray(mjd, np.float64)[final], star_n_iter=star_deconv_n_iter,
            uniform_background_per_epoch=star_photometry_uniform_background_per_epoch,
            starlet_global_background=star_photometry_starlet_global_background,
            fluxes_chi2_strategy=fluxes_fit_exclude_strategy, psf_chi2=psf_chi2[final],
            psf_chi2_strategy=psf_fit_exclude_strategy, coefficient_bounds=constraints_on_normalization_coeff,
            frame_columns=columns, frame_constraints=constraints_on_frame_columns_for_roi,
            angles_to_north=angles[final], ctx=ctx, fix_point_source_astrometry=fix_point_source_astrometry,
            starting_background=starting_background, further_optimize_background=further_optimize_background,
            regularization=roi_model_regularization, roi_deconv_translations_iters=roi_deconv_translations_iters,
            roi_deconv_all_iters=roi_deconv_all_iters)
        lap('calibrated_light_curves')
    finally:
        if own_set:
            fs.close()

    out = dict(out)
    out.update(kept=final[out['kept']], eliminated=eliminated, frames_fitted=final, registration=results,
               footprints=footprints, common_footprint=common, total_bounds=total_bounds(footprints), stars=stars,
               stars_in_frames=in_frames, psf_stars={k: list(stars['name'][v]) for k, v in psf_stars.items()},
               normalization_stars=list(stars['name'][used]), star_frame_index=[final[rows] for rows in star_frame_index],
               sources_tables=tables, psf_results=psf_results, psf_chi2=psf_chi2, seeing_pixels=seeing,
               ellipticity=ellipticity, background_rms=background_rms, angles=angles, scales=scales, roi_origin=roi_origin,
               point_sources_in_stamps=in_stamps, seconds=seconds)
    if coadd is not None:
        out['coadd'] = coadd
    return out
