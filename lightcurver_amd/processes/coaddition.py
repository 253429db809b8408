"""The deep image of the field: every registered frame of a resident set resampled onto the reference frame's grid and
combined (``FrameSet.coadd``, ``lc_frames_coadd``; DESIGN.md §5 "Co-addition of frames").  The reference has no such
step: it takes its star catalogue from Gaia.  Here the co-add gives a catalogue that is deeper than any single frame's,
free of cosmic rays and independent of the choice of the reference frame."""
import numpy as np


def _fluxes_brightest_first(table):
    """The ``flux`` column in the order ``plate_solving.table_positions`` puts the rows in."""
    if isinstance(table, dict):
        table = table['sources_table']
    flux = np.asarray(np.asarray(table)['flux'], np.float64)
    return flux[np.argsort(-flux, kind='stable')]


def relative_flux_scales(source_tables, results, reference=0):
    """Per frame the factor that brings its fluxes onto the reference frame's: 1 / median(flux_frame / flux_reference)
    over the matched ``pairs`` of ``register_frames(source_tables, reference)`` (whose rows number each table brightest
    first, as ``table_positions`` sorts it).  ``reference``: the same index, or table, that ``register_frames`` was given.
    NaN for a frame that failed or has no matched pair.  Host NumPy."""
    ref = _fluxes_brightest_first(source_tables[reference] if isinstance(reference, (int, np.integer)) else reference)
    out = np.full(len(results), np.nan)
    for k, r in enumerate(results):
        pairs = np.asarray(r['pairs'], np.int64).reshape(-1, 2)
        if not r['success'] or not len(pairs):
            continue
        flux = _fluxes_brightest_first(source_tables[k])
        with np.errstate(all='ignore'):
            out[k] = 1.0 / np.median(flux[pairs[:, 1]] / ref[pairs[:, 0]])
    return out


def coadd_frames(fs, results, frames=None, flux_scale=None, weights=None, reject_cosmics=None, **kw):
    """``FrameSet.coadd`` of the frames that ``register_frames`` solved: ``results`` is its list, one entry per frame of
    ``fs``; ``frames`` (default: all) the frames to take, of which those that failed are skipped.  flux_scale, weights:
    None, or one value per frame of the SET (as ``relative_flux_scales`` returns them), indexed like ``results``; a frame
    whose flux scale is not finite is skipped too.  The grid defaults to the reference frame's (``shape``, ``origin`` and
    everything else go to ``FrameSet.coadd``).  reject_cosmics: None, or a dict of ``cosmics_masking_params`` (``{}``: the
    defaults): ``fs.detect_cosmics(apply='nan', download=())`` then runs on the frames about to be stacked, so that a
    cosmic is missing from its frame's samples whatever ``combine`` is, with 'mean' too and with a handful of frames.  The
    planes KEEP those NaNs afterwards: a later ``cut_stamps`` sees them as the NaN rule prescribes.  Returns the dict of
    ``FrameSet.coadd`` plus ``frames``: the frames that went in."""
    K = len(results)
    take = np.arange(K) if frames is None else np.asarray(frames, np.int64).reshape(-1)
    per_set = lambda a: None if a is None else np.broadcast_to(np.asarray(a, np.float64).reshape(-1), (K,))
    g, w = per_set(flux_scale), per_set(weights)
    used = np.array([k for k in take if results[k]['success'] and (g is None or np.isfinite(g[k]))], dtype=np.int64)
    if not len(used):
        raise ValueError('coadd_frames: no registered frame to co-add')
    if reject_cosmics is not None:
        fs.detect_cosmics(np.unique(used), apply='nan', cosmics_masking_params=dict(reject_cosmics), download=())
    out = fs.coadd(used, [results[k]['transform'] for k in used], flux_scale=None if g is None else g[used],
                   weights=None if w is None else w[used], **kw)
    out['frames'] = used
    return out
