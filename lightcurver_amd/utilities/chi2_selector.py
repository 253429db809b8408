"""Bounds on the reduced chi2 of a fit (PSF or star photometry) inside which its result is used, restated from the
reference's lightcurver/utilities/chi2_selector.py:20-42 with the configuration entry and the chi2 values as arguments
(the reference reads the first from its user config and the second from its database)."""
import numpy as np


def sigma_clipped_stats(values, sigma=3.0, maxiters=5):
    """(mean, median, std) of the sample after sigma clipping: what astropy.stats.sigma_clipped_stats returns with its
    defaults (clipping about the median by ``sigma`` population standard deviations, both recomputed from the surviving
    sample at every pass, at most ``maxiters`` passes, ending early when a pass rejects nothing; values that are not
    finite never take part).  astropy is not a dependency here."""
    v = np.ravel(np.asarray(values, dtype=np.float64))
    v = v[np.isfinite(v)]
    for _ in range(int(maxiters)):
        if v.size == 0:
            break
        centre, spread = np.median(v), np.std(v)
        keep = np.abs(v - centre) <= sigma * spread
        if keep.all():
            break
        v = v[keep]
    if v.size == 0:
        return np.nan, np.nan, np.nan
    return float(np.mean(v)), float(np.median(v)), float(np.std(v))


def get_chi2_bounds(chi2_values, strategy):
    """-> (chi2_min, chi2_max).  ``strategy`` is the reference's ``psf_fit_exclude_strategy`` /
    ``fluxes_fit_exclude_strategy``: None (no bound), {'threshold': (lo, hi)} (the pair as given) or {'sigma_clip': k}
    (median -+ k std of the sigma-clipped ``chi2_values``, which only this form reads)."""
    if strategy is None:
        return -np.inf, np.inf
    if not isinstance(strategy, dict) or len(strategy) != 1:
        raise ValueError(f"chi2 strategy must be None, {{'sigma_clip': k}} or {{'threshold': (lo, hi)}}, not {strategy!r}")
    (key, val), = strategy.items()
    if key == 'threshold':
        lo, hi = val
        return lo, hi
    if key == 'sigma_clip':
        _, median, std = sigma_clipped_stats(chi2_values, sigma=float(val))
        return median - val * std, median + val * std
    raise ValueError(f"unexpected chi2 strategy {key!r}; valid: None, 'sigma_clip' or 'threshold'")
