"""From the stamps of the reference stars and of the region of interest to calibrated light curves, in one call: the
reference's pipeline steps ``star_photometry`` -> ``calculate_normalization_coefficient`` ->
``calculate_absolute_zeropoints`` -> ``prepare_calibrated_cutouts`` -> ``model_calibrated_cutouts``
(pipeline_dependency_graph.yaml) chained on arrays.  Every stage is a public function of this package called as a user
would call it; the chain adds no numerics of its own (only the scatter of the stars' epochs into (stars x frames) tables)
and returns the intermediate products beside the light curves."""
import numpy as np

from ..utilities.chi2_selector import get_chi2_bounds
from .absolute_zeropoint_calculation import adjust_zeropoints, calculate_zeropoints
from .normalization_calculation import calculate_coefficients
from .roi_file_preparation import prepare_roi_cutouts
from .roi_modelling import fluxes_from_model, model_roi_cutouts
from .star_photometry import do_many_stars_forward_modelling


def star_tables(star_results, star_frame_index, n_frames):
    """The per-star results of ``do_many_stars_forward_modelling`` as (S, n_frames) tables: fluxes and their uncertainties
    in the units of the stamps (the fit's value times its ``scale``, which is what the result dictionaries hold) and the
    reduced chi2 per frame; NaN where a star has no epoch in a frame.  star_frame_index[g][k]: frame of epoch k of star g."""
    S = len(star_results)
    if len(star_frame_index) != S:
        raise ValueError(f'star_frame_index must hold one index array per star ({S}), got {len(star_frame_index)}')
    fluxes, d_fluxes, chi2 = (np.full((S, int(n_frames)), np.nan) for _ in range(3))
    for g, (res, index) in enumerate(zip(star_results, star_frame_index)):
        index = np.asarray(index, dtype=np.int64)
        if index.shape != np.shape(res['fluxes']) or np.unique(index).size != index.size:
            raise ValueError(f'star {g}: star_frame_index must name one distinct frame per epoch ({len(res["fluxes"])})')
        if index.size and (index.min() < 0 or index.max() >= n_frames):
            raise ValueError(f'star {g}: frame index outside 0 .. {int(n_frames) - 1}')
        fluxes[g, index] = res['fluxes']
        d_fluxes[g, index] = res['fluxes_uncertainties']
        chi2[g, index] = res['chi2_per_frame']
    return fluxes, d_fluxes, chi2


def calibrated_light_curves(star_stacks, roi_stack, subsampling_factor, xs_pixels, ys_pixels, *, star_frame_index, n_frames,
                            catalog_mags=None, mjd=None, star_n_iter=2000, uniform_background_per_epoch=False,
                            starlet_global_background=False, fluxes_chi2_strategy=None, outlier_threshold=None,
                            psf_chi2=None, psf_chi2_strategy=None, coefficient_bounds=None, frame_columns=None,
                            frame_constraints=None, kwargs_distortion=None, roi_xy=None, frame_shape=None,
                            angles_to_north=None, ctx=None, **roi_fit_options):
    """star_stacks: per reference star (data, noisemap, psf) = (E_g, n, n), (E_g, n, n), (E_g, n ss, n ss), cleaned
    (``star_photometry.prepare_star_epochs``), in the units of the frames; copied, so the caller's arrays stay as they are.
    roi_stack: (data, noisemap, cosmics_mask, narrow_psf) of the ROI over ALL ``n_frames`` frames, same units.
    xs_pixels, ys_pixels: the point sources of the ROI, (M,) in pixels of the first kept frame's stamp, or (n_frames, M):
    row j in pixels of frame j's stamp, of which row ``kept[0]`` is used (which frame comes first is decided here, by the
    selection and ``mjd``).  star_frame_index: per star the
    frame of each of its epochs (every star keeps its own frame selection).  catalog_mags (S,): calibrated magnitudes of
    the stars, for the zero-point.  mjd (n_frames,): orders the kept frames.  angles_to_north (n_frames,).

    Stages: 1 ``do_many_stars_forward_modelling`` (star_n_iter, the two background switches); 2 ``star_tables``;
    3 ``get_chi2_bounds`` of the stars' chi2 per frame (``fluxes_chi2_strategy``) and of ``psf_chi2``
    (``psf_chi2_strategy``); 4 ``calculate_coefficients`` (``outlier_threshold``); 5 ``calculate_zeropoints`` and
    ``adjust_zeropoints`` where magnitudes are given; 6 ``prepare_roi_cutouts`` (the selection and distortion arguments);
    7 ``model_roi_cutouts`` (``roi_fit_options``: its keyword arguments, the iteration counts among them);
    8 ``fluxes_from_model`` with the kept frames' normalisation errors.

    Returns dict: fluxes, d_fluxes (M, K) calibrated light curves over the K kept frames, kept (K,), mjd (K,) or None,
    reduced_chi2 (K,), global_zeropoint, global_zeropoint_scatter (None without magnitudes), and the intermediate products
    star_results, star_fluxes, star_d_fluxes, star_chi2 (S, n_frames), fluxes_chi2_bounds, psf_chi2_bounds, normalization
    (the dict of ``calculate_coefficients``), zeropoint, zeropoint_uncertainty (n_frames,) or None, prepared (the dict of
    ``prepare_roi_cutouts``), roi_fit (of ``model_roi_cutouts``), light_curves (of ``fluxes_from_model``)."""
    per_frame_positions = np.ndim(xs_pixels) == 2 or np.ndim(ys_pixels) == 2
    if per_frame_positions:
        xs_pixels, ys_pixels = (np.asarray(v, dtype=np.float64) for v in (xs_pixels, ys_pixels))
        if xs_pixels.ndim != 2 or xs_pixels.shape != ys_pixels.shape or xs_pixels.shape[0] != int(n_frames):
            raise ValueError(f'per-frame positions must both be (n_frames, M) with n_frames = {int(n_frames)}, got '
                             f'{xs_pixels.shape} and {ys_pixels.shape}')
    stacks = [tuple(np.array(a, dtype=np.float64) for a in stack) for stack in star_stacks]
    star_results = do_many_stars_forward_modelling(stacks, subsampling_factor, n_iter=star_n_iter,
                                                   uniform_background_per_epoch=uniform_background_per_epoch,
                                                   starlet_global_background=starlet_global_background)
    star_fluxes, star_d_fluxes, star_chi2 = star_tables(star_results, star_frame_index, n_frames)
    fluxes_bounds = get_chi2_bounds(star_chi2, fluxes_chi2_strategy)
    normalization = calculate_coefficients(star_fluxes, star_d_fluxes, chi2=star_chi2, chi2_bounds=fluxes_bounds,
                                           outlier_threshold=outlier_threshold)
    zeropoint = zeropoint_uncertainty = global_zeropoint = global_scatter = None
    if catalog_mags is not None:
        zeropoint, zeropoint_uncertainty = calculate_zeropoints(star_fluxes, catalog_mags)
        global_zeropoint, global_scatter = adjust_zeropoints(zeropoint, normalization['coefficient'])
    psf_bounds = get_chi2_bounds(psf_chi2, psf_chi2_strategy) if psf_chi2 is not None else None
    data, noisemap, cosmics_mask, narrow_psf = roi_stack
    prepared = prepare_roi_cutouts(data, noisemap, cosmics_mask, narrow_psf, normalization['coefficient'],
                                   normalization['coefficient_uncertainty'], psf_chi2=psf_chi2, psf_chi2_bounds=psf_bounds,
                                   coefficient_bounds=coefficient_bounds, frame_columns=frame_columns,
                                   frame_constraints=frame_constraints, mjd=mjd, kwargs_distortion=kwargs_distortion,
                                   roi_xy=roi_xy, frame_shape=frame_shape, ctx=ctx)
    kept = prepared['kept']
    angles = None if angles_to_north is None else np.asarray(angles_to_north, dtype=np.float64)[kept]
    if per_frame_positions:      # the fit takes the sources where they are in its first epoch
        xs_pixels, ys_pixels = xs_pixels[kept[0]], ys_pixels[kept[0]]
    roi_fit = model_roi_cutouts(prepared['data'], prepared['noisemap'], prepared['psf'], subsampling_factor, xs_pixels,
                                ys_pixels, angles_to_north=angles, **roi_fit_options)
    n_sources = np.atleast_1d(np.asarray(xs_pixels)).size
    curves = fluxes_from_model(roi_fit['model'], roi_fit['kwargs_final'], roi_fit['kwargs_up'], roi_fit['kwargs_down'],
                               roi_fit['data'], roi_fit['noisemap'], n_sources, roi_fit['scale'],
                               normalization_errors=prepared['relative_normalization_error'])
    return dict(fluxes=curves['fluxes'], d_fluxes=curves['d_fluxes'], kept=kept, mjd=prepared.get('mjd'),
                reduced_chi2=curves['reduced_chi2'], global_zeropoint=global_zeropoint,
                global_zeropoint_scatter=global_scatter, star_results=star_results, star_fluxes=star_fluxes,
                star_d_fluxes=star_d_fluxes, star_chi2=star_chi2, fluxes_chi2_bounds=fluxes_bounds,
                psf_chi2_bounds=psf_bounds, normalization=normalization, zeropoint=zeropoint,
                zeropoint_uncertainty=zeropoint_uncertainty, prepared=prepared, roi_fit=roi_fit, light_curves=curves)
