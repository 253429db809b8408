"""Which stars to use: the reference's star catalogue around the ROI (lightcurver/processes/star_querying.py), its star
names (utilities/star_naming.py) and its two selections (structure/database.py ``select_stars`` and
``select_stars_for_a_frame``), restated on arrays.  The reference queries Gaia and keeps the stars in its database; here
the catalogue is a record array in pixels of the reference frame, built from that frame's own table of sources (or passed
in by a caller who has brought a real catalogue to reference pixels), and a selection is an index into it.  Host code."""
import numpy as np

CATALOGUE_DTYPE = np.dtype([('name', 'U8'), ('x', '<f8'), ('y', '<f8'), ('flux', '<f8'), ('distance_to_roi', '<f8')])
_LETTERS = 'abcdefghijklmnopqrstuvwxyz'


def generate_star_names(n):
    """n names in the reference's order: a ... z, aa, ab, ... (every string of one letter, then of two, and so on)."""
    names = []
    for i in range(int(n)):
        name, i = '', i + 1                    # bijective base 26: 1 -> a, 26 -> z, 27 -> aa
        while i > 0:
            i, r = divmod(i - 1, 26)
            name = _LETTERS[r] + name
        names.append(name)
    return names


def _columns(sources_table):
    """(x, y, flux, flag-or-None) of a dict with a ``sources_table``, a structured array with x and y (flux and flag where
    it has them), or a plain (S, 2) / (S, 3) array of x, y(, flux)."""
    if isinstance(sources_table, dict):
        sources_table = sources_table['sources_table']
    t = np.asarray(sources_table)
    if t.dtype.names:
        names = t.dtype.names
        x, y = np.asarray(t['x'], np.float64).ravel(), np.asarray(t['y'], np.float64).ravel()
        flux = np.asarray(t['flux'], np.float64).ravel() if 'flux' in names else np.full(x.shape, np.nan)
        flag = np.asarray(t['flag']).ravel() if 'flag' in names else None
        return x, y, flux, flag
    t = np.asarray(t, np.float64)
    if t.ndim != 2 or t.shape[1] not in (2, 3):
        raise ValueError(f'expected a table of sources or an (S, 2) / (S, 3) array of x, y(, flux), got {t.shape}')
    return t[:, 0], t[:, 1], (t[:, 2] if t.shape[1] == 3 else np.full(len(t), np.nan)), None


def reference_star_catalogue(sources_table, roi_xy, roi_exclusion_radius, flux_range=None, min_isolation=None,
                             require_unflagged=True):
    """The catalogue of reference stars, from the reference frame's table of sources (``import_frames``,
    ``characterize_frames``) or from any positions with fluxes.  Sources within ``roi_exclusion_radius`` pixels of
    ``roi_xy`` are dropped (the ROI itself, and what would blend with it), the rest sorted by their distance to the ROI
    and named in that order.  Two optional cuts stand in for the Gaia quality cuts, which cannot be queried here:
    ``flux_range`` (lo, hi), inclusive, for the magnitude range, and ``min_isolation``: the least distance, in pixels, to
    every other source of the table (dropped ones included).  ``require_unflagged``: where the table has a ``flag``
    column, only sources whose flag is 0.  Rows with a non-finite position are dropped.  Returns a record array with
    name, x, y, flux, distance_to_roi (pixels)."""
    x, y, flux, flag = _columns(sources_table)
    roi = np.asarray(roi_xy, np.float64).reshape(2)
    distance = np.hypot(x - roi[0], y - roi[1])
    with np.errstate(invalid='ignore'):
        keep = np.isfinite(x) & np.isfinite(y) & (distance > float(roi_exclusion_radius))
        if require_unflagged and flag is not None:
            keep &= flag == 0
        if flux_range is not None:
            lo, hi = flux_range
            keep &= (flux >= lo) & (flux <= hi)
        if min_isolation is not None and len(x) > 1:
            d = np.hypot(x[:, None] - x[None, :], y[:, None] - y[None, :])
            np.fill_diagonal(d, np.inf)
            d[np.isnan(d)] = np.inf                       # a source without a position crowds nobody
            keep &= d.min(axis=1) >= float(min_isolation)
    index = np.flatnonzero(keep)
    index = index[np.argsort(distance[index], kind='stable')]
    out = np.zeros(len(index), CATALOGUE_DTYPE)
    out['name'] = generate_star_names(len(index))
    out['x'], out['y'], out['flux'], out['distance_to_roi'] = x[index], y[index], flux[index], distance[index]
    return out


def select_stars(catalogue, stars_to_use=None, stars_to_exclude=None, available=None):
    """The rows of ``catalogue`` (what ``reference_star_catalogue`` returns: ordered by distance to the ROI) that a step
    uses, as an index array in catalogue order.  ``stars_to_use``: None for the 10 nearest, an int for that many of the
    nearest, a list for the stars of those names.  ``stars_to_exclude``: a list of names, or a string each of whose
    characters is a name; applied after the selection, so it takes precedence (asking for the 5 nearest and excluding one
    of them leaves 4).  ``available``: one bool per star, a frame's row of the stars-in-frames table; it restricts the
    choice before the cut to the nearest, as the reference's join does in ``select_stars_for_a_frame``.  Argument types
    other than these raise RuntimeError, as in the reference."""
    names = np.asarray(catalogue['name'])
    candidates = np.arange(len(names))
    if available is not None:
        available = np.asarray(available, dtype=bool)
        if available.shape != names.shape:
            raise ValueError(f'available must hold one flag per star ({len(names)}), got {available.shape}')
        candidates = candidates[available]
    if stars_to_use is None:
        stars_to_use = 10
    if isinstance(stars_to_use, (int, np.integer)) and not isinstance(stars_to_use, bool):
        order = np.argsort(np.asarray(catalogue['distance_to_roi'], np.float64)[candidates], kind='stable')
        chosen = np.sort(candidates[order[:max(int(stars_to_use), 0)]])
    elif isinstance(stars_to_use, list):
        chosen = candidates[np.isin(names[candidates], [str(s) for s in stars_to_use])]
    else:
        raise RuntimeError(f'stars_to_use argument: expected types None, int or list, got: {type(stars_to_use)}')
    if stars_to_exclude:
        if isinstance(stars_to_exclude, str):
            stars_to_exclude = list(stars_to_exclude)
        if not isinstance(stars_to_exclude, list):
            raise RuntimeError(f'stars_to_exclude argument: expected types None, str or list, got: {type(stars_to_exclude)}')
        chosen = chosen[~np.isin(names[chosen], [str(s) for s in stars_to_exclude])]
    return chosen
