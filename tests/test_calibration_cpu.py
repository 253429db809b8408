"""Photometric calibration on the host (DESIGN.md section 5 "Photometric calibration"): the normalisation coefficients
from a (stars x frames) flux table, the chi2 bounds, the zero-points, the frame selection of the ROI preparation and the
ROI file round trip.  No GPU: the two device calls of ``prepare_roi_cutouts`` are replaced by NumPy stand-ins here and
run for real in tests/test_calibration_gpu.py."""
import warnings

import numpy as np
import pytest

from lightcurver_amd.io.regions import read_roi_file, write_roi_file
from lightcurver_amd.processes import roi_file_preparation as rfp
from lightcurver_amd.processes.absolute_zeropoint_calculation import adjust_zeropoints, calculate_zeropoints
from lightcurver_amd.processes.normalization_calculation import calculate_coefficients
from lightcurver_amd.utilities.chi2_selector import get_chi2_bounds


def scatter_cost(s, f, d):
    """The reference's cost, straight from its formula: per frame the variance of s_i f_ie about its weighted mean with
    the weights 1 / d_ie, summed over the frames; NaN entries take no part."""
    total = 0.0
    for e in range(f.shape[1]):
        ok = np.isfinite(f[:, e]) & np.isfinite(d[:, e])
        if not ok.any():
            continue
        w = 1.0 / d[ok, e]
        v = s[ok] * f[ok, e]
        mean = np.sum(w * v) / np.sum(w)
        total += np.sum(w * (v - mean) ** 2) / np.sum(w)
    return total


def median_normalised(f, d):
    m = np.nanmedian(f, axis=1, keepdims=True)
    return f / m, d / m


def drop_entries(rng, S, E, fraction, at_least=2):
    """True where an entry is missing: ``fraction`` of them, every frame keeping ``at_least`` stars, every star a frame."""
    missing = rng.uniform(size=(S, E)) < fraction
    for e in range(E):
        while (~missing[:, e]).sum() < min(at_least, S):
            missing[rng.integers(S), e] = False
    for i in range(S):
        if missing[i].all():
            missing[i, rng.integers(E)] = False
    return missing


def test_noiseless_recovery():
    rng = np.random.default_rng(11)
    S, E = 8, 60
    F = np.exp(rng.uniform(np.log(1e3), np.log(1e5), S))
    t = rng.uniform(0.5, 1.5, E)
    f = F[:, None] * t[None, :]
    d = 0.01 * f
    missing = drop_entries(rng, S, E, 0.2)
    assert 0.1 < missing.mean() < 0.3 and ((~missing).sum(axis=0) >= 2).all()
    f[missing] = np.nan
    d[missing] = np.nan
    out = calculate_coefficients(f, d)
    ratio = out['coefficient'] / t
    assert np.max(np.abs(ratio / ratio.mean() - 1.0)) <= 1e-12
    assert np.all(out['coefficient_uncertainty'] <= 1e-12)
    assert abs(out['star_scaling'].mean() - 1.0) <= 1e-12
    assert np.array_equal(out['n_stars_used'], (~missing).sum(axis=0))
    assert np.array_equal(np.isnan(out['normalized_fluxes']), missing)


@pytest.mark.parametrize('seed', range(5))
def test_kkt_solution_is_the_minimiser(seed):
    from scipy.optimize import minimize
    rng = np.random.default_rng(100 + seed)
    S, E = int(rng.integers(2, 13)), int(rng.integers(4, 201))
    F = np.exp(rng.uniform(np.log(1e3), np.log(1e5), S))
    t = rng.uniform(0.5, 1.5, E)
    truth = F[:, None] * t[None, :]
    sigma = rng.uniform(0.005, 0.05, S)[:, None] * truth
    f = truth + sigma * rng.standard_normal((S, E))
    d = sigma * rng.uniform(0.8, 1.2, (S, E))
    missing = drop_entries(rng, S, E, 0.3 * rng.uniform())
    f[missing] = np.nan
    d[missing] = np.nan
    # (tie the stars together whatever was dropped: frame 0 holds them all)
    f[:, 0], d[:, 0] = truth[:, 0], sigma[:, 0]
    s = calculate_coefficients(f, d)['star_scaling']
    g, dg = median_normalised(f, d)
    cost = lambda x: scatter_cost(np.asarray(x), g, dg)
    res = minimize(cost, np.ones(S), constraints=({'type': 'eq', 'fun': lambda x: 1 - np.nanmean(x)}), method='SLSQP')
    x = res.x / res.x.mean()          # exactly on the constraint, like s
    assert abs(s.mean() - 1.0) <= 1e-12
    print(f'S={S} E={E} cost kkt {cost(s):.12e} slsqp {cost(x):.12e}')
    assert cost(s) <= cost(x) * (1 + 1e-12)
    # KKT: the gradient of the cost is a multiple of the constraint's, (1, ..., 1).  The cost is quadratic, so central
    # differences with a step of 1 are its exact gradient up to rounding.
    grad = np.array([(cost(s + np.eye(S)[i]) - cost(s - np.eye(S)[i])) / 2.0 for i in range(S)])
    assert np.max(np.abs(grad - grad.mean())) <= 1e-9 * np.max(np.abs(grad))


def test_noisy_recovery():
    rng = np.random.default_rng(5)
    S, E = 6, 40
    F = np.exp(rng.uniform(np.log(1e4), np.log(1e5), S))
    t = rng.uniform(0.5, 1.5, E)
    truth = F[:, None] * t[None, :]
    f = truth + np.sqrt(truth) * rng.standard_normal((S, E))
    d = np.sqrt(f)
    out = calculate_coefficients(f, d)
    ratio = out['coefficient'] / t
    scatter = np.std(ratio) / np.mean(ratio)
    predicted = np.median(1.0 / np.sqrt(np.sum((f / d) ** 2, axis=0)))
    print(f'relative scatter of coefficient / t: {scatter:.3e}, predicted {predicted:.3e}')
    assert scatter < 3 * predicted
    assert np.all(out['coefficient_uncertainty'] > 0) and np.all(out['n_stars_used'] == S)


def _table(rng, S, E, noise=0.01):
    F = np.exp(rng.uniform(np.log(1e3), np.log(1e5), S))
    t = rng.uniform(0.5, 1.5, E)
    truth = F[:, None] * t[None, :]
    return truth * (1 + noise * rng.standard_normal((S, E))), noise * truth, t


def test_one_star_gets_a_tenth_of_the_coefficient_as_uncertainty():
    f, d, t = _table(np.random.default_rng(1), 1, 12)
    out = calculate_coefficients(f, d)
    assert np.array_equal(out['star_scaling'], [1.0])
    assert np.allclose(out['coefficient'], f[0] / np.median(f[0]), rtol=1e-14)
    assert np.array_equal(out['coefficient_uncertainty'], 0.1 * out['coefficient'])
    # ... and so does a frame that keeps one star of several
    f, d, t = _table(np.random.default_rng(2), 4, 12)
    f[1:, 3] = d[1:, 3] = np.nan
    out = calculate_coefficients(f, d)
    assert out['n_stars_used'][3] == 1 and out['coefficient_uncertainty'][3] == 0.1 * out['coefficient'][3]
    assert np.all(out['coefficient_uncertainty'][np.arange(12) != 3] < 0.05)


def test_frame_without_stars_is_nan():
    f, d, t = _table(np.random.default_rng(3), 4, 10)
    f[:, 6] = d[:, 6] = np.nan
    out = calculate_coefficients(f, d)
    assert np.isnan(out['coefficient'][6]) and np.isnan(out['coefficient_uncertainty'][6]) and out['n_stars_used'][6] == 0
    others = np.arange(10) != 6
    assert np.all(np.isfinite(out['coefficient'][others])) and np.all(out['n_stars_used'][others] == 4)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        cut = calculate_coefficients(f, d, outlier_threshold=50.0)         # nothing is that far out: the same numbers
    for key in out:
        assert np.array_equal(cut[key], out[key], equal_nan=True), key


def test_chi2_bounds_turn_entries_into_nan():
    f, d, t = _table(np.random.default_rng(4), 5, 10)
    chi2 = np.ones((5, 10))
    chi2[2, 4], chi2[0, 7], chi2[1, 1] = 9.0, 0.01, np.nan
    out = calculate_coefficients(f, d, chi2=chi2, chi2_bounds=(0.5, 2.0))
    gone = np.zeros((5, 10), bool)
    gone[2, 4] = gone[0, 7] = gone[1, 1] = True
    assert np.array_equal(np.isnan(out['normalized_fluxes']), gone)
    assert np.array_equal(np.isnan(out['normalized_d_fluxes']), gone)
    assert np.array_equal(out['n_stars_used'], 5 - gone.sum(axis=0))
    # the bounds are inclusive, and without bounds the chi2 is not read
    assert not np.isnan(calculate_coefficients(f, d, chi2=chi2, chi2_bounds=(1.0, 9.0))['normalized_fluxes'][2, 4])
    assert not np.isnan(calculate_coefficients(f, d, chi2=chi2)['normalized_fluxes']).any()


def test_outlier_threshold_removes_a_planted_point_the_default_keeps():
    rng = np.random.default_rng(6)
    f, d, t = _table(rng, 6, 10)
    f[2, 5] += 10 * d[2, 5]
    kept = calculate_coefficients(f, d)
    cut = calculate_coefficients(f, d, outlier_threshold=3.0)
    assert np.isfinite(kept['normalized_fluxes'][2, 5]) and kept['n_stars_used'][5] == 6
    assert np.isnan(cut['normalized_fluxes'][2, 5]) and np.isnan(cut['normalized_d_fluxes'][2, 5])
    assert cut['n_stars_used'][5] <= 5
    # the cut coefficient of that frame sits closer to the truth than the uncut one
    r_kept, r_cut = kept['coefficient'] / t, cut['coefficient'] / t
    others = np.arange(10) != 5
    assert abs(r_cut[5] / np.mean(r_cut[others]) - 1) < abs(r_kept[5] / np.mean(r_kept[others]) - 1)


def test_disconnected_stars_raise():
    f, d, t = _table(np.random.default_rng(7), 4, 10)
    f[:2, 5:] = d[:2, 5:] = np.nan
    f[2:, :5] = d[2:, :5] = np.nan
    with pytest.raises(ValueError, match='share no frame'):
        calculate_coefficients(f, d)
    # one star alone in its frames: named
    f, d, t = _table(np.random.default_rng(8), 4, 10)
    f[3, :8] = d[3, :8] = np.nan
    f[:3, 8:] = d[:3, 8:] = np.nan
    with pytest.raises(ValueError, match=r'\[3\]'):
        calculate_coefficients(f, d)
    # a star without any flux
    f, d, t = _table(np.random.default_rng(9), 3, 6)
    f[1] = np.nan
    with pytest.raises(ValueError, match=r'\[1\]'):
        calculate_coefficients(f, d)


# ---- chi2 bounds ---------------------------------------------------------------------------------------------------
def test_chi2_bounds_strategies():
    v = np.array([0.9, 1.0, 1.1])
    assert get_chi2_bounds(v, None) == (-np.inf, np.inf)
    assert get_chi2_bounds(v, {'threshold': (0.5, 2.0)}) == (0.5, 2.0)
    lo, hi = get_chi2_bounds(v, {'sigma_clip': 2.0})
    assert np.isclose(lo, 1.0 - 2 * np.std(v)) and np.isclose(hi, 1.0 + 2 * np.std(v))
    for bad in ({'median': 3}, 'sigma_clip', {'sigma_clip': 2, 'threshold': (0, 1)}, 3.0):
        with pytest.raises(ValueError):
            get_chi2_bounds(v, bad)


def test_sigma_clip_against_the_clipping_loop():
    rng = np.random.default_rng(21)
    v = rng.normal(1.0, 0.1, 400)
    v[:12] = rng.uniform(3.0, 50.0, 12)        # planted outliers
    v[12:15] = np.nan                          # ignored
    k = 3.0
    sample = v[np.isfinite(v)]
    for _ in range(5):
        med, std = np.median(sample), np.std(sample)
        inside = (sample >= med - k * std) & (sample <= med + k * std)
        if inside.all():
            break
        sample = sample[inside]
    expected = (np.median(sample) - k * np.std(sample), np.median(sample) + k * np.std(sample))
    got = get_chi2_bounds(v.reshape(20, 20), {'sigma_clip': k})
    assert np.allclose(got, expected, rtol=1e-14, atol=0)
    assert sample.size <= 400 - 15 and 0.6 < got[0] < 0.8 and 1.2 < got[1] < 1.4      # the planted points are out


# ---- zero-points ---------------------------------------------------------------------------------------------------
def test_zeropoints_closed_form():
    rng = np.random.default_rng(31)
    S, E, ZP = 7, 15, 27.3
    F = np.exp(rng.uniform(np.log(1e3), np.log(1e5), S))
    t = rng.uniform(0.5, 1.5, E)
    mags = ZP - 2.5 * np.log10(F)
    f = F[:, None] * t[None, :]
    f[0, 2] = np.nan
    f[1, 3] = -5.0        # a negative flux has no magnitude
    zp, dzp = calculate_zeropoints(f, mags)
    assert np.allclose(zp, ZP + 2.5 * np.log10(t), rtol=0, atol=1e-12)
    assert np.all(dzp <= 1e-12)
    usable = np.where(f > 0, f, np.nan)
    coefficient = calculate_coefficients(usable, 0.01 * usable)['coefficient']
    adjusted = zp - 2.5 * np.log10(coefficient)
    assert np.max(np.abs(adjusted - adjusted[0])) <= 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        global_zp, scatter = adjust_zeropoints(zp, coefficient)
    assert abs(global_zp - adjusted[0]) <= 1e-12 and scatter <= 1e-12
    with pytest.warns(RuntimeWarning, match='scatter'):
        adjust_zeropoints(zp, coefficient[::-1] * np.linspace(0.5, 2.0, E))
    assert adjust_zeropoints(np.full(4, np.nan), np.ones(4)) == (None, None)
    assert adjust_zeropoints([], []) == (None, None)
    # fewer than two stars: no uncertainty; NaN magnitudes are skipped
    zp1, dzp1 = calculate_zeropoints(f[:1], mags[:1])
    assert np.isnan(dzp1).all() and np.isnan(zp1[2]) and np.isfinite(np.delete(zp1, 2)).all()
    mags_nan = mags.copy()
    mags_nan[4] = np.nan
    assert np.allclose(calculate_zeropoints(f, mags_nan)[0], zp, rtol=0, atol=1e-12)


# ---- frame selection of the ROI preparation ---------------------------------------------------------------------------
def _numpy_prepare_stamps(data, noisemap=None, coefficient=None, bad=None, nan_noise=1.0, noise_boost=0.0,
                          boost_whole_stamp=False, ctx=None, want=()):
    assert not boost_whole_stamp and nan_noise == 1e7 and noise_boost == 1000.0
    _numpy_prepare_stamps.calls += 1
    c = np.asarray(coefficient, dtype=np.float64)[:, None, None]
    d, s = np.array(data, dtype=np.float64) / c, np.array(noisemap, dtype=np.float64) / c
    both = np.isnan(d) & np.isnan(s)
    d[both], s[both] = 0.0, nan_noise
    s[np.asarray(bad, dtype=bool)] *= noise_boost
    return {'data': d, 'noisemap': s}


def _numpy_apply_distortion(narrow_psf, kwargs_distortion, star_xy_coordinates, ctx=None):
    _numpy_apply_distortion.calls.append((np.array(star_xy_coordinates), dict(kwargs_distortion)))
    xy = np.asarray(star_xy_coordinates).reshape(-1, 2)
    return np.stack([np.asarray(narrow_psf) * (1.0 + kwargs_distortion['shear'][0]) + p[0] for p in xy])


@pytest.fixture
def host_stand_ins(monkeypatch):
    _numpy_prepare_stamps.calls = 0
    _numpy_apply_distortion.calls = []
    monkeypatch.setattr(rfp, 'prepare_stamps', _numpy_prepare_stamps)
    monkeypatch.setattr(rfp, 'apply_distortion', _numpy_apply_distortion)


def test_prepare_roi_cutouts_selection_order_and_kept(host_stand_ins):
    rng = np.random.default_rng(41)
    E, n, P = 10, 6, 12
    data, noise = rng.uniform(1, 2, (E, n, n)), rng.uniform(0.1, 0.2, (E, n, n))
    data[1, 2, 3] = noise[1, 2, 3] = np.nan
    bad = rng.uniform(size=(E, n, n)) < 0.05
    psf = rng.uniform(size=(E, P, P))
    coefficient = np.linspace(0.6, 1.5, E)
    coefficient[2] = np.nan                      # no coefficient
    uncertainty = np.full(E, 0.01)
    uncertainty[9] = 0.2                         # outside the bound on the uncertainty
    chi2 = np.ones(E)
    chi2[4] = 7.0                                # PSF chi2 out of bounds
    seeing = np.full(E, 1.0)
    seeing[6] = 2.5                              # a frame column out of its interval
    mjd = np.array([5., 3., 1., 9., 2., 8., 4., 0., 7., 6.])
    out = rfp.prepare_roi_cutouts(data, noise, bad, psf, coefficient, uncertainty, psf_chi2=chi2, psf_chi2_bounds=(0.5, 2.0),
                                  coefficient_bounds={'coefficient': (0.65, 2.0), 'coefficient_uncertainty': (0.0, 0.1)},
                                  frame_columns={'seeing_arcseconds': seeing, 'airmass': np.ones(E)},
                                  frame_constraints={'seeing_arcseconds': (0.0, 1.1)}, mjd=mjd)
    # frames 0 (coefficient 0.6 < 0.65), 2, 4, 6, 9 are out; the rest ordered by mjd
    assert out['kept'].tolist() == [7, 1, 8, 5, 3]      # (frame 1, with the NaN pair, is row 1 of the output)
    assert _numpy_prepare_stamps.calls == 1
    k = out['kept']
    c = coefficient[k][:, None, None]
    assert np.array_equal(out['mjd'], mjd[k]) and np.array_equal(out['relative_normalization_error'], uncertainty[k])
    assert np.array_equal(out['mask'], ~bad[k]) and np.array_equal(out['psf'], psf[k])
    d, s = data[k] / c, noise[k] / c
    assert out['data'][1, 2, 3] == 0.0 and out['noisemap'][1, 2, 3] == (1e7 * 1000.0 if bad[1, 2, 3] else 1e7)
    rest = np.isfinite(d)
    assert np.array_equal(out['data'][rest], d[rest])
    assert np.array_equal(out['noisemap'][rest], np.where(bad[k], 1000.0 * s, s)[rest])
    # no bounds at all: every frame with a coefficient, in the input's order without mjd
    out = rfp.prepare_roi_cutouts(data, noise, bad, psf, coefficient, uncertainty)
    assert out['kept'].tolist() == [0, 1, 3, 4, 5, 6, 7, 8, 9] and 'mjd' not in out
    assert rfp.prepare_roi_cutouts(data, noise, bad, psf, coefficient, uncertainty,
                                   coefficient_bounds=(0.95, 1.35))['kept'].tolist() == [4, 5, 6, 7]
    with pytest.raises(KeyError):
        rfp.prepare_roi_cutouts(data, noise, bad, psf, coefficient, uncertainty, frame_constraints={'airmass': (0, 2)})
    with pytest.raises(ValueError, match='no frame'):
        rfp.prepare_roi_cutouts(data, noise, bad, psf, coefficient, uncertainty, coefficient_bounds=(5.0, 6.0))


def test_prepare_roi_cutouts_distortion_per_kept_frame(host_stand_ins):
    from lightcurver_amd.io.regions import rescale_image_coordinates
    rng = np.random.default_rng(42)
    E, n, P = 5, 4, 8
    data, noise = rng.uniform(1, 2, (E, n, n)), rng.uniform(0.1, 0.2, (E, n, n))
    psf = rng.uniform(size=(E, P, P))
    psf[3] = psf[1]                              # two frames with one PSF model and (below) one coefficient set
    kw = [{'shear': np.array([0.01 * (j + 1), 0.0, 0.0])} for j in range(E)]
    kw[3] = kw[1]
    coefficient = np.array([1.0, 1.1, np.nan, 0.9, 1.2])
    xy = rng.uniform(100, 900, (E, 2))
    out = rfp.prepare_roi_cutouts(data, noise, np.zeros((E, n, n), bool), psf, coefficient, np.full(E, 0.01),
                                  mjd=[4., 3., 2., 1., 0.], kwargs_distortion=kw, roi_xy=xy, frame_shape=(1000, 1200))
    assert out['kept'].tolist() == [4, 3, 1, 0]
    for row, j in enumerate(out['kept']):
        position = rescale_image_coordinates(xy[j], (1000, 1200))
        assert np.allclose(out['psf'][row], psf[j] * (1.0 + kw[j]['shear'][0]) + position[0], rtol=1e-6)
    # frames 3 and 1 share PSF and coefficients: one call with their two positions; the dropped frame is never resampled
    assert sorted(len(np.reshape(c[0], (-1, 2))) for c in _numpy_apply_distortion.calls) == [1, 1, 2]


# ---- ROI file --------------------------------------------------------------------------------------------------------
def test_write_roi_file_round_trip():
    rng = np.random.default_rng(51)
    K, n, P = 4, 8, 12
    prepared = dict(data=rng.uniform(size=(K, n, n)).astype(np.float32), noisemap=rng.uniform(size=(K, n, n)).astype(np.float32),
                    mask=np.ones((K, n, n), bool), psf=rng.uniform(size=(K, P, P)).astype(np.float32),
                    relative_normalization_error=rng.uniform(0.001, 0.01, K), kept=np.array([5, 2, 7, 3]),
                    mjd=np.array([1., 2., 3., 4.]))
    node = {}
    assert write_roi_file(node, prepared, subsampling_factor=2, global_zeropoint=27.1, global_zeropoint_scatter=0.02,
                          seeing=np.full(K, 1.1), angle_to_north=np.zeros(K), wcs=['w'] * K, pixel_scale=None) is node
    back = read_roi_file(node)
    for key in ('data', 'noisemap', 'psf', 'relative_normalization_error', 'mjd'):
        assert np.array_equal(back[key], prepared[key]), key
    assert np.array_equal(back['frame_id'], prepared['kept']) and back['subsampling'] == 2 and back['psf_side'] == P
    assert back['global_zeropoint'] == 27.1 and back['global_zeropoint_scatter'] == 0.02
    assert back['subsampling_factor'].shape == (K,) and 'pixel_scale' not in back and 'mask' not in node
    write_roi_file(node, prepared, subsampling_factor=np.full(K, 2), frame_id=np.arange(K))      # written again: replaced
    assert np.array_equal(read_roi_file(node)['frame_id'], np.arange(K))
    with pytest.raises(KeyError):
        write_roi_file({}, prepared, exposure=1.0)
    with pytest.raises(ValueError, match='seeing'):
        write_roi_file({}, prepared, subsampling_factor=2, seeing=np.ones(K + 1))
