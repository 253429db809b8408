"""Absolute zero-points from the star fluxes and catalogue magnitudes: the arithmetic of the reference's
lightcurver/processes/absolute_zeropoint_calculation.py:94-100 (per frame) and roi_file_preparation.py:102-118 (one
zero-point for the normalised data), on arrays.  The catalogue magnitudes themselves (Gaia, Pan-STARRS: network queries)
and the database stay with the caller."""
import warnings

import numpy as np


def _median_and_sample_std(values, ok):
    """Per column over the entries where ``ok``: median and standard deviation with ddof = 1 (pandas' ``std``: NaN with
    fewer than two entries); NaN median where no entry is left."""
    E = values.shape[1]
    median, std = np.full(E, np.nan), np.full(E, np.nan)
    for e in range(E):
        v = values[ok[:, e], e]
        if v.size:
            median[e] = np.median(v)
        if v.size > 1:
            std[e] = np.std(v, ddof=1)
    return median, std


def calculate_zeropoints(fluxes, catalog_mags):
    """fluxes (S stars, E frames), in the units of the frames (not normalised); catalog_mags (S,).  Per frame the
    zero-point = median over the stars of ``catalog_mag + 2.5 log10(flux)`` and its uncertainty = their sample standard
    deviation, over the stars with a finite positive flux and a finite magnitude (NaN with fewer than two of them).
    -> (zeropoint (E,), zeropoint_uncertainty (E,))."""
    f = np.asarray(fluxes, dtype=np.float64)
    m = np.asarray(catalog_mags, dtype=np.float64)
    if f.ndim != 2 or m.shape != (f.shape[0],):
        raise ValueError(f'expected fluxes (S, E) and catalog_mags (S,), got {f.shape} and {m.shape}')
    with np.errstate(invalid='ignore', divide='ignore'):
        ok = np.isfinite(f) & (f > 0) & np.isfinite(m)[:, None]
        difference = m[:, None] + 2.5 * np.log10(np.where(ok, f, 1.0))
    return _median_and_sample_std(difference, ok)


def adjust_zeropoints(zeropoint, coefficient):
    """The zero-point of the NORMALISED data: median over the frames of ``zeropoint - 2.5 log10(coefficient)``, and the
    sample standard deviation of that (a statistical uncertainty), over the frames where both are finite (and the
    coefficient positive).  Warns when normalising did not lower the scatter of the zero-points, which it should with
    well-behaved data (harmless with very few frames).  -> (global_zeropoint, scatter), (None, None) without frames."""
    zp = np.asarray(zeropoint, dtype=np.float64)
    c = np.asarray(coefficient, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(zp) & np.isfinite(c) & (c > 0)
    if not ok.any():
        return None, None
    zp, c = zp[ok], c[ok]
    adjusted = zp - 2.5 * np.log10(c)
    before = np.std(zp, ddof=1) if zp.size > 1 else np.nan
    after = np.std(adjusted, ddof=1) if zp.size > 1 else np.nan
    if after > before:
        warnings.warn('the scatter of the zero-points is lower before normalising than after: not normal, investigate',
                      RuntimeWarning, stacklevel=2)
    return float(np.median(adjusted)), float(after)
