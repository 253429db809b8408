"""Normalisation coefficient of every frame from the fluxes of the reference stars: the arithmetic of the reference's
lightcurver/processes/normalization_calculation.py:163-204 on (stars x frames) arrays instead of its database tables
(the queries, the insert and the plot stay with the caller).  Host NumPy in float64: the tables hold a few dozen stars.

Differences from the reference, both deliberate (DESIGN.md section 5 "Photometric calibration"):

* the star scalings minimise the reference's cost exactly, by one linear solve, where the reference drives SLSQP with
  finite differences to a stopping tolerance;
* a frame without a usable star gets NaN where the reference would raise from ``np.average``.
"""
import warnings

import numpy as np

MAD_TO_SIGMA = 0.6744897501960817   # scipy's median_abs_deviation(scale='normal') divides by this (norm.ppf(0.75))


def scatter_quadratic_form(fluxes, d_fluxes):
    """The matrix A (S, S) with ``cost_function_scatter_in_frame(s) = s^T A s`` (normalization_calculation.py:72-92):
    per frame the variance of s_i f_ie about its weighted mean, with the weights w_ie = 1 / d_ie (not squared, as the
    reference has it), summed over the frames; missing entries are NaN in both tables.  With p_ie = w_ie / sum_i w_ie,
    A = sum_e [diag(p_e f_e^2) - (p_e f_e)(p_e f_e)^T]."""
    present = np.isfinite(fluxes) & np.isfinite(d_fluxes)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.where(present, 1.0 / d_fluxes, 0.0)
        total = w.sum(axis=0)
        p = np.where(total > 0, w / total, 0.0)
    f = np.where(present, fluxes, 0.0)
    pf = p * f
    return np.diag((pf * f).sum(axis=1)) - pf @ pf.T


def _components(present):
    """Label of the connected component of every star, two stars being linked when a frame holds both."""
    S = present.shape[0]
    link = (present.astype(np.int64) @ present.astype(np.int64).T) > 0
    label = -np.ones(S, np.int64)
    n = 0
    for start in range(S):
        if label[start] >= 0:
            continue
        stack = [start]
        label[start] = n
        while stack:
            i = stack.pop()
            for j in np.flatnonzero(link[i] & (label < 0)):
                label[j] = n
                stack.append(j)
        n += 1
    return label


def solve_star_scalings(fluxes, d_fluxes):
    """argmin_s s^T A s under mean(s) = 1: the (S + 1) x (S + 1) KKT system [[2A, 1], [1^T, 0]] [s, lambda] = [0, S],
    solved directly (A is divided by its mean diagonal first, which moves lambda and not s).  Raises ValueError where the
    frames do not tie the stars together: the relative scaling of two groups of stars that never share a frame is not
    determined by the cost (the solve would put all the weight on a star that is alone in its frames)."""
    S = fluxes.shape[0]
    if S == 1:
        return np.ones(1)
    present = np.isfinite(fluxes) & np.isfinite(d_fluxes)
    label = _components(present)
    if label.max() > 0:
        main = np.argmax(np.bincount(label))
        apart = [int(i) for i in np.flatnonzero(label != main)]
        raise ValueError(f'singular system: the stars {apart} (row indices) share no frame with any other star of the '
                         f'main group, so their scaling is not determined; drop them or add frames that hold both')
    A = scatter_quadratic_form(fluxes, d_fluxes)
    norm = np.trace(A) / S
    if norm > 0:
        A = A / norm
    K = np.zeros((S + 1, S + 1))
    K[:S, :S] = 2.0 * A
    K[:S, S] = K[S, :S] = 1.0
    rhs = np.zeros(S + 1)
    rhs[S] = S
    try:
        sol = np.linalg.solve(K, rhs)
    except np.linalg.LinAlgError as e:
        raise ValueError('singular system: the frames do not determine the relative scalings of the stars') from e
    if not np.all(np.isfinite(sol)):
        raise ValueError('singular system: the frames do not determine the relative scalings of the stars')
    return sol[:S]


def weighted_mean_and_std(values, weights):
    """Per column: the weighted mean, the weighted population standard deviation about it (``weighted_std``,
    normalization_calculation.py:114-130) and the number of entries used; NaN entries skipped, NaN where none is left."""
    ok = np.isfinite(values) & np.isfinite(weights)
    w = np.where(ok, weights, 0.0)
    v = np.where(ok, values, 0.0)
    total = w.sum(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.where(total > 0, (v * w).sum(axis=0) / total, np.nan)
        var = np.where(total > 0, (w * (v - mean) ** 2).sum(axis=0) / total, np.nan)
    return mean, np.sqrt(var), ok.sum(axis=0)


def calculate_coefficients(fluxes, d_fluxes, chi2=None, chi2_bounds=None, outlier_threshold=None):
    """fluxes, d_fluxes (S stars, E frames) float64, NaN = "this star has no flux in this frame"; chi2 (S, E) and
    chi2_bounds (lo, hi): entries whose chi2 lies outside the bounds (inclusive, as SQL's BETWEEN) count as missing
    (``get_fluxes``, :45).  An entry is also missing where either table is not finite or the uncertainty is not positive.

    Steps (:163-204): every star's row divided by the star's median flux; one scaling per star that minimises the scatter
    of the stars within the frames under mean(s) = 1 (``solve_star_scalings``); the coefficient of a frame = mean of its
    scaled fluxes weighted by 1 / d^2, its uncertainty = the weighted population standard deviation about that mean.  A
    frame with ONE star has no scatter: its uncertainty is 0.1 x coefficient (:204; the reference tests ``== 0``, which its
    own ``np.average`` can miss by one rounding, so the count of stars decides here).  A frame with no star: NaN, NaN and
    ``n_stars_used = 0``.

    ``outlier_threshold``: the reference defines ``filter_outliers`` (:95-111, per frame |f - median| > threshold x MAD,
    MAD scaled to sigma) but never applies it - :191-192 copy the tables unfiltered - so None, the default, reproduces
    what the reference computes; a number applies that cut to the scaled fluxes before the two weighted sums.

    Returns dict: coefficient, coefficient_uncertainty (E,), star_scaling (S,), normalized_fluxes, normalized_d_fluxes
    (S, E; scaled, and cut where ``outlier_threshold`` is given), n_stars_used (E,) int."""
    f = np.array(fluxes, dtype=np.float64)
    d = np.array(d_fluxes, dtype=np.float64)
    if f.ndim != 2 or d.shape != f.shape:
        raise ValueError(f'fluxes and d_fluxes must be (S, E) tables of one shape, got {f.shape} and {d.shape}')
    missing = ~(np.isfinite(f) & np.isfinite(d))
    with np.errstate(invalid='ignore'):
        missing |= ~(d > 0)
        if chi2 is not None and chi2_bounds is not None:
            c = np.asarray(chi2, dtype=np.float64)
            if c.shape != f.shape:
                raise ValueError(f'chi2 must have the shape of fluxes {f.shape}, got {c.shape}')
            lo, hi = chi2_bounds
            missing |= ~((c >= lo) & (c <= hi))
    f[missing] = np.nan
    d[missing] = np.nan
    S, E = f.shape
    alone = np.flatnonzero(missing.all(axis=1))
    if alone.size and S > 1:
        raise ValueError(f'singular system: the stars {[int(i) for i in alone]} (row indices) have no usable flux in any '
                         f'frame and so share no frame with any other star; drop them')
    with np.errstate(invalid='ignore', divide='ignore'):
        median = np.nanmedian(f, axis=1, keepdims=True) if E else np.full((S, 1), np.nan)
        f = f / median
        d = d / median
    scaling = solve_star_scalings(f, d)
    f = f * scaling[:, None]
    d = d * scaling[:, None]
    if outlier_threshold is not None:
        with np.errstate(invalid='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)      # a frame without stars: an all-NaN column, nothing to cut
            centre = np.nanmedian(f, axis=0)
            mad = np.nanmedian(np.abs(f - centre), axis=0) / MAD_TO_SIGMA
            out = np.abs(f - centre) > float(outlier_threshold) * mad
        f[out] = np.nan
        d[out] = np.nan
    with np.errstate(divide='ignore', invalid='ignore'):
        coefficient, uncertainty, count = weighted_mean_and_std(f, 1.0 / d ** 2)
    uncertainty = np.where(count == 1, 0.1 * coefficient, uncertainty)
    return dict(coefficient=coefficient, coefficient_uncertainty=uncertainty, star_scaling=scaling,
                normalized_fluxes=f, normalized_d_fluxes=d, n_stars_used=count.astype(np.int64))
