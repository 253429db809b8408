"""The arithmetic of the reference's two plate solvers that need no web service (lightcurver/processes/
alternate_plate_solving_adapt_existing_wcs.py::adapt_wcs and alternate_plate_solving_with_gaia.py::
refine_wcs_with_astroalign): one ``astroalign.find_transform`` per frame, then 2 x 2 algebra on ``crpix`` and ``cd``.  Here
every frame of a set is registered against one reference frame in one device call (``lc_register_sources``; DESIGN.md §5
"Frame registration"), and the pixel positions that ``FrameSet.cut_stamps`` and ``extract_all_stamps_of_frames`` take
follow from the transforms alone, without any WCS.  FITS headers, ``astropy.wcs`` objects and the database stay with the
caller, who passes ``wcs.wcs.crpix`` and ``wcs.wcs.cd`` (or ``pc * cdelt``) as plain arrays."""
import numpy as np

from .. import astroalign


def _matrix(transform):
    """The 3 x 3 homogeneous matrix of a ``SimilarityTransform``, a 3 x 3 array or the six numbers a, -b, tx, b, a, ty."""
    if hasattr(transform, 'params'):
        return np.asarray(transform.params, np.float64)
    m = np.asarray(transform, np.float64)
    if m.shape == (6,):
        return astroalign.SimilarityTransform.from_row(m).params
    if m.shape != (3, 3):
        raise ValueError(f'expected a transform, a 3 x 3 matrix or six numbers, got an array of shape {m.shape}')
    return m


def adapt_wcs_arrays(crpix, cd, transform):
    """``adapt_wcs``'s update of a reference WCS (alternate_plate_solving_adapt_existing_wcs.py:29-40) for a frame whose
    ``transform`` came from ``find_transform(reference_sources, frame_sources)``: the pixels are transformed actively, so
    ``crpix -> R crpix + t`` and ``cd -> R cd`` with R the scaled rotation.  Returns (crpix, cd) of the frame."""
    m = _matrix(transform)
    scaled_rotation, translation = m[:2, :2], m[:2, 2]
    return (np.dot(scaled_rotation, np.asarray(crpix, np.float64)) + translation,
            np.dot(scaled_rotation, np.asarray(cd, np.float64)))


def refine_wcs_arrays(crpix, cd, transform):
    """``refine_wcs_with_astroalign``'s update of a guessed WCS (alternate_plate_solving_with_gaia.py:71-73), where
    ``transform`` came from ``find_transform(image_positions, gaia_pixel_positions)``: through the inverse,
    ``crpix -> R' crpix + t'`` and ``cd -> R' cd``.  Returns (crpix, cd)."""
    inv = np.linalg.inv(_matrix(transform))
    return inv[:2, :2] @ np.asarray(crpix, np.float64) + inv[:2, 2], inv[:2, :2] @ np.asarray(cd, np.float64)


def table_positions(table):
    """(n, 2) float64 (x, y) of one frame's sources, brightest first: a dict of ``characterize_frames`` (its
    ``sources_table``), a structured array with x and y (ordered by its ``flux`` where it has one: the record arrays of
    ``import_frames`` are in raster order), or an (n, 2) array taken as it is."""
    if isinstance(table, dict):
        table = table['sources_table']
    t = np.asarray(table)
    if t.dtype.names:
        if 'flux' in t.dtype.names:
            t = t[np.argsort(-t['flux'], kind='stable')]
        return np.stack([t['x'], t['y']], axis=1).astype(np.float64).reshape(-1, 2)
    return np.asarray(t, np.float64).reshape(-1, 2)


def register_frames(source_tables, reference=0, max_control_points=astroalign.MAX_CONTROL_POINTS, ctx=None):
    """Registers every frame of a set against frame ``reference`` (an index into ``source_tables``, or a table of its own)
    in one device call.  ``source_tables``: per frame what ``table_positions`` takes.  Returns one dict per frame:
    transform (a ``SimilarityTransform`` from the reference's pixels to the frame's, None where the frame failed), success,
    n_matched (matched stars), pairs ((n_matched, 2) rows of the reference's and the frame's positions), status and diag as
    ``astroalign.find_transforms_batch`` gives them."""
    frames = [table_positions(t) for t in source_tables]
    if not frames:
        return []
    ref = frames[reference] if isinstance(reference, (int, np.integer)) else table_positions(reference)
    r = astroalign.find_transforms_batch(ref, frames, max_control_points, ctx=ctx)
    return [dict(transform=r['transforms'][k], success=bool(r['status'][k] == 0), n_matched=len(r['pairs'][k]),
                 pairs=r['pairs'][k], status=int(r['status'][k]), diag=r['diag'][k]) for k in range(len(frames))]


def positions_in_frames(results, positions_xy_reference):
    """The pixel positions in every frame of the (x, y) positions given in the reference frame: a list of (S, 2) arrays,
    one per result of ``register_frames``, NaN for a frame that failed.  With ``frame_index = np.repeat(range(K), S)``
    their concatenation is what ``FrameSet.cut_stamps`` takes."""
    pos = np.asarray(positions_xy_reference, np.float64).reshape(-1, 2)
    return [r['transform'](pos) if r['success'] else np.full(pos.shape, np.nan) for r in results]
