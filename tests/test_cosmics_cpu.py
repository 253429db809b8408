"""Cosmic-ray detection ("Cosmic-ray detection"): hand-made cases for the NumPy restatement of the SPEC
(tests/_lacosmic.py, the checker the device kernel is compared with bit for bit), its float32 form against float64 on
synthetic star stamps, and the Python-side refusals and size range.  No GPU needed."""
import numpy as np
import pytest
import scipy.ndimage as ndi

from tests import _lacosmic as LA

DTYPES = (np.float32, np.float64)


def _flat(n=32, sky=100.0, seed=0):
    rng = np.random.default_rng(seed)
    return (sky + np.sqrt(sky + 6.5 ** 2) * rng.standard_normal((n, n))).astype(np.float32)


def _moffat(n, fwhm, flux, beta=3.0, cx=None, cy=None):
    cx = (n - 1) / 2.0 if cx is None else cx
    cy = (n - 1) / 2.0 if cy is None else cy
    a = fwhm / (2.0 * np.sqrt(2.0 ** (1.0 / beta) - 1.0))
    y, x = np.mgrid[0:n, 0:n]
    m = (1.0 + ((x - cx) ** 2 + (y - cy) ** 2) / a ** 2) ** (-beta)
    return flux * m / m.sum()


def _star(n=32, fwhm=3.0, flux=1e5, sky=100.0, seed=0):
    rng = np.random.default_rng(seed)
    clean = sky + _moffat(n, fwhm, flux, cx=(n - 1) / 2.0 + 0.3, cy=(n - 1) / 2.0 - 0.2)
    var = clean + 6.5 ** 2
    return (clean + np.sqrt(var) * rng.standard_normal((n, n))).astype(np.float32), var.astype(np.float32)


@pytest.mark.parametrize('dt', DTYPES)
def test_single_hot_pixel_on_flat_noise_is_flagged_and_cleaned(dt):
    d = _flat()
    d[16, 16] += 500.0
    r = LA.lacosmic(d, dtype=dt)
    assert np.argwhere(r['crmask']).tolist() == [[16, 16]]
    assert abs(r['clean'][16, 16] - 100.0) < 5.0          # the local mean of the sky
    assert r['iters'][0] == 2                               # iteration 2 finds nothing more and stops
    assert not LA.lacosmic(_flat(seed=2), dtype=dt)['crmask'].any()


@pytest.mark.parametrize('dt', DTYPES)
def test_track_is_flagged_with_its_grown_neighbour(dt):
    d = _flat(seed=1)
    d[10, 12:15] += 400.0        # a three-pixel track
    d[9, 13] += 60.0             # charge beside it: below sigclip, above sigfrac * sigclip
    r = LA.lacosmic(d, dtype=dt, trace=True)
    assert np.argwhere(r['crmask']).tolist() == [[9, 13], [10, 12], [10, 13], [10, 14]]
    _, SP, _ = r['trace'][0]
    assert 0.3 * 4.5 < SP[0, 9, 13] < 4.5                   # flagged by the growth alone


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('fwhm', [2.5, 3.0, 4.0])
def test_moffat_star_without_injection_has_nothing_flagged(dt, fwhm):
    for seed in range(3):
        d, var = _star(fwhm=fwhm, seed=seed)
        assert not LA.lacosmic(d, dtype=dt)['crmask'].any()
        assert not LA.lacosmic(d, invar=var, dtype=dt)['crmask'].any()
        assert not LA.lacosmic(d, invar=var, sepmed=False, dtype=dt)['crmask'].any()


@pytest.mark.parametrize('dt', DTYPES)
def test_inmask_pixel_is_never_flagged(dt):
    d = _flat()
    d[16, 16] += 500.0
    d[20, 8] += 500.0
    inmask = np.zeros(d.shape, bool)
    inmask[16, 16] = True
    r = LA.lacosmic(d, inmask=inmask, dtype=dt)
    assert np.argwhere(r['crmask']).tolist() == [[20, 8]]
    assert r['clean'][16, 16] == d[16, 16]                  # not a cosmic: left as it is


def _window_mean(d, good, i, j):
    acc, cnt = np.float32(0.0), 0
    for y in range(max(i - 2, 0), min(i + 3, d.shape[0])):
        for x in range(max(j - 2, 0), min(j + 3, d.shape[1])):
            if good[y, x]:
                acc = np.float32(acc + d[y, x])
                cnt += 1
    return np.float32(acc / np.float32(cnt)), cnt


def test_meanmask_value_by_hand():
    d = _flat()
    d[16, 16] += 800.0
    r = LA.lacosmic(d, niter=1)
    assert np.argwhere(r['crmask']).tolist() == [[16, 16]]
    want, cnt = _window_mean(d, ~r['crmask'], 16, 16)
    assert cnt == 24 and r['clean'][16, 16] == want
    # the window is clipped to the stamp (the detection never flags a pixel that close to the edge: SP = 0 on the
    # border ring the median keeps, so the clean step is checked on its own), and masked pixels do not count
    CR = np.zeros(d.shape, bool)
    CR[1, 1] = CR[0, 2] = True
    M = np.zeros(d.shape, bool)
    M[3, 0] = True
    out = LA.meanmask(d[None], CR[None], M[None])[0]
    for (i, j), n_good in (((1, 1), 13), ((0, 2), 13)):
        want, cnt = _window_mean(d, ~CR & ~M, i, j)
        assert cnt == n_good and out[i, j] == want
    assert np.array_equal(out[~CR], d[~CR])


def test_meanmask_without_good_neighbour_takes_the_stamp_median():
    d = _flat()
    d[16, 16] += 800.0
    inmask = np.zeros(d.shape, bool)
    inmask[14:19, 14:19] = True
    inmask[16, 16] = False       # the cosmic alone in a masked 5 x 5 window
    r = LA.lacosmic(d, inmask=inmask, niter=1)
    assert r['crmask'][16, 16]
    good = ~inmask & ~r['crmask']
    v = np.sort(d[good])
    assert r['clean'][16, 16] == v[(v.size - 1) // 2]


@pytest.mark.parametrize('dt', DTYPES)
def test_nan_rule(dt):
    """Off-frame pixels of a partial cutout (NaN in data and noise map), invar <= 0: masked, C = 0, never flagged;
    everything else still works and every output is finite."""
    d = _flat(seed=3)
    var = np.full(d.shape, 100.0 + 6.5 ** 2, np.float32)
    d[:, :6] = np.nan
    var[:, :6] = np.nan
    var[25, 25] = 0.0
    d[25, 25] += 900.0           # would be a cosmic, but its variance is not positive
    d[12, 20] += 500.0
    for invar in (var, None):
        r = LA.lacosmic(d, invar=invar, dtype=dt)
        hole = ~np.isfinite(d) | (False if invar is None else ~(var > 0))
        assert np.all(r['mask'][hole]) and not np.any(r['crmask'][hole])
        assert np.all(r['clean'][hole] == 0) and np.all(np.isfinite(r['clean']))
        assert r['crmask'][12, 20]
    r = LA.lacosmic(d, invar=var, dtype=dt)
    assert np.argwhere(r['crmask']).tolist() == [[12, 20]]


@pytest.mark.parametrize('dt', DTYPES)
def test_saturation_is_grown_by_two_pixels(dt):
    n = 32
    d, _ = _star(n, fwhm=3.0, flux=4e5, seed=4)
    sat = 20000.0
    core = d >= sat
    assert 1 <= core.sum() <= 9
    d[5, 5] = 3 * sat            # a lone saturated cosmic: its m5 is sky, so it is no saturated star
    d[np.argwhere(core)[0][0] + 2, np.argwhere(core)[0][1]] += 5000.0   # 2 px from the core: inside the grown mask
    r = LA.lacosmic(d, satlevel=sat, dtype=dt)
    assert np.array_equal(r['mask'], LA.dil3(LA.dil3(core)))
    assert r['crmask'][5, 5]
    assert not np.any(r['crmask'] & r['mask'])


def test_separable_and_full_medians_are_the_textbook_filters():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((2, 20, 20)).astype(np.float32)
    for k in (3, 5, 7, 9):
        h = k // 2
        full = LA.med_full(X, k)
        ref = ndi.median_filter(X, size=(1, k, k), mode='nearest')
        assert np.array_equal(full[:, h:-h, h:-h], ref[:, h:-h, h:-h])
        border = np.ones((20, 20), bool)
        border[h:-h, h:-h] = False
        assert np.array_equal(full[:, border], X[:, border])
        rows = ndi.median_filter(X, size=(1, 1, k), mode='nearest')
        rows[..., :h], rows[..., 20 - h:] = X[..., :h], X[..., 20 - h:]
        sep = ndi.median_filter(rows, size=(1, k, 1), mode='nearest')
        sep[:, :h], sep[:, 20 - h:] = rows[:, :h], rows[:, 20 - h:]
        assert np.array_equal(LA.med_sep(X, k), sep)
    assert np.array_equal(LA.med_full(X[:, :8, :8], 9), X[:, :8, :8])    # no interior: every pixel keeps its input


def test_sepmed_false_takes_the_full_median_path(monkeypatch):
    d = _flat()
    d[16, 16] += 500.0
    ref = LA.lacosmic(d, sepmed=False)
    assert np.argwhere(ref['crmask']).tolist() == [[16, 16]]

    def boom(*a, **k):
        raise AssertionError('wrong median path')
    with monkeypatch.context() as m:
        m.setattr(LA, 'med_sep', boom)
        r = LA.lacosmic(d, sepmed=False)
    assert np.array_equal(r['crmask'], ref['crmask']) and np.array_equal(r['clean'], ref['clean'])
    with monkeypatch.context() as m:
        m.setattr(LA, 'med_full', boom)
        LA.lacosmic(d, sepmed=True)
        with pytest.raises(AssertionError, match='wrong median path'):
            LA.lacosmic(d, sepmed=False)


def test_early_exit_reports_the_iteration_count():
    d = _flat()
    assert LA.lacosmic(d)['iters'][0] == 1                  # nothing found: stops after the first iteration
    d[16, 16] += 500.0
    assert LA.lacosmic(d)['iters'][0] == 2
    assert LA.lacosmic(d, niter=1)['iters'][0] == 1
    stack = np.stack([_flat(seed=7), d])
    assert LA.lacosmic(stack)['iters'].tolist() == [1, 2]
    assert LA.lacosmic(stack, niter=0)['iters'].tolist() == [0, 0]


def test_float32_against_float64_outside_the_ambiguous_set():
    """Masks of the float32 and float64 restatements over the full niter loop.  A pixel is ambiguous when SP against
    sigclip, SP / F against objlim or SP against sigfrac * sigclip lies within 1e-4 relative of the threshold, in either
    precision and any iteration, at the pixel or one of its 3 x 3 neighbours; that set is capped at 0.1 % of the
    pixels, and outside it the masks agree on every pixel."""
    from lightcurver_amd.synthetic import make_psf_dataset
    thresholds = ((0, 4.5), (1, 5.0), (0, 0.3 * 4.5))
    total = amb_total = 0
    for n in (24, 32, 64):
        for seed in (1, 2, 3):
            ds = make_psf_dataset(F=20, S=8, n=n, seed=seed)
            d = ds['data'].reshape(-1, n, n)
            nm = ds['noisemap'].reshape(-1, n, n)
            r0 = LA.lacosmic(d, invar=nm ** 2)
            assert not r0['crmask'].any()                   # nothing flagged on the unperturbed stars
            dc, hit = LA.inject_cosmics(d, nm, np.random.default_rng(seed + 100))
            r32 = LA.lacosmic(dc, invar=nm ** 2, trace=True)
            r64 = LA.lacosmic(dc, invar=nm ** 2, dtype=np.float64, trace=True)
            amb = np.zeros(dc.shape, bool)
            for r in (r32, r64):
                for active, SP, ratio in r['trace']:
                    q = (SP, ratio)
                    a = np.zeros(SP.shape, bool)
                    for which, thr in thresholds:
                        a |= np.abs(q[which] - thr) <= 1e-4 * thr
                    amb[active] |= LA.dil3(a)
            disagree = (r32['crmask'] != r64['crmask']) & ~amb
            print(f'n={n} seed={seed}: ambiguous {amb.mean():.2e}, disagreements outside {disagree.sum()}, '
                  f'injected {hit.sum()} flagged {(hit & r32["crmask"]).sum()}')
            assert not disagree.any()
            assert amb.mean() <= 1e-3
            total += amb.size
            amb_total += amb.sum()
    print(f'ambiguous share over all inputs: {amb_total / total:.2e}')
    assert amb_total / total <= 1e-3


def test_unbuilt_options_are_refused():
    from lightcurver_amd.astroscrappy import detect_cosmics
    from lightcurver_amd.processes.cutout_making import mask_cosmics_batch
    d = np.zeros((16, 16), np.float32)
    with pytest.raises(NotImplementedError, match='inbkg'):
        detect_cosmics(d, inbkg=np.zeros_like(d))
    for ct in ('median', 'medmask', 'idw'):
        with pytest.raises(NotImplementedError, match='cleantype'):
            detect_cosmics(d, cleantype=ct)
    with pytest.raises(NotImplementedError, match='fsmode'):
        detect_cosmics(d, fsmode='convolve')
    with pytest.raises(NotImplementedError, match='ccdmask'):
        mask_cosmics_batch(d[None], d[None] + 1, {}, do_mask_bad_columns=True)


def test_library_reports_the_stamp_size_range():
    from lightcurver_amd import _lib
    from lightcurver_amd.astroscrappy import supported
    lib = _lib.lib()
    assert [n for n in range(0, 200) if lib.lc_cosmics_supported(n)] == list(range(8, 129))
    assert supported(24) and supported(33) and not supported(7) and not supported(129)


@pytest.mark.parametrize('n,K,with_invar,sepmed', LA.SETTINGS_INPUTS)
def test_every_settings_case_changes_the_restatement(n, K, with_invar, sepmed):
    """The condition of the settings lists (LA.SETTINGS, LA.SETTINGS_VARIANTS): on its input every case gives another
    result than its base (the defaults, or the defaults with the one setting named in the case), in the output the
    case names: a kernel that ignored the setting would fail the device comparison of tests/test_cosmics_gpu.py."""
    cases = LA.settings_wanted(n, K, with_invar, sepmed)
    assert [c[0] for c in cases] == [c[0] for c in LA.settings_cases(n, K, with_invar, sepmed)]
    for label, d, kw, want, base in cases:
        changed = (want['crmask'] != base['crmask']).sum()
        print(f'n={n} invar={with_invar} sepmed={sepmed} {label}: crmask pixels changed {changed}, clean '
              f'{(want["clean"].view(np.uint32) != base["clean"].view(np.uint32)).sum()}, flagged {want["crmask"].sum()}, '
              f'iters {np.bincount(want["iters"]).tolist()}')
        assert LA.settings_differ(label, want, base), label
    by = {c[0]: c for c in cases}
    if 'niter 1' in by:        # some stamp's mask differs between niter 1 and niter 4
        label, d, kw, want, base = by['niter 1']
        assert (want['crmask'] != base['crmask']).reshape(K, -1).any(axis=1).any() and want['iters'].max() == 1
    label, d, kw, want, base = by['sigclip 0.5 objlim 0.5']
    assert np.all(want['iters'] == 4) and want['crmask'].sum() > 20 * base['crmask'].sum()   # the load case of meanmask


def test_settings_lists_cover_every_setting():
    """No case disappears quietly: a label is left out of an input only where LA.SETTINGS_NOT_MET names it, which is at
    n = 65 alone, so every label runs on all eight inputs of the two LDS sizes and at n = 65 at least once."""
    for key in LA.SETTINGS_INPUTS:
        other = LA.SETTINGS_VARIANTS[key]
        assert set(other) <= set(LA.SETTINGS)
        assert {label for label, spec in other.items() if spec is None} == LA.SETTINGS_NOT_MET.get(key, set()), key
        ran = LA.settings_cases(*key)
        assert [c[0] for c in ran] == [label for label in LA.SETTINGS if label not in LA.SETTINGS_NOT_MET.get(key, set())]
        for label, variant, seed in ran:
            assert variant in ('plain', 'blocks') or key[2], (key, label)     # the holes are holes of invar
            assert seed is None or seed != 10 * key[0] + key[1]
    assert all(key[0] == 65 for key in LA.SETTINGS_NOT_MET) and set(LA.SETTINGS_NOT_MET) <= set(LA.SETTINGS_INPUTS)
    at65 = set().union(*({c[0] for c in LA.settings_cases(*key)} for key in LA.SETTINGS_INPUTS if key[0] == 65))
    assert at65 == set(LA.SETTINGS)


def test_configuration_path_refuses_without_a_device():
    from lightcurver_amd.processes.cutout_making import mask_cosmics_batch, mask_cutout_batch
    d = np.ones((2, 16, 16), np.float32)
    for params, err in ((dict(cleantype='median'), NotImplementedError), (dict(sigclipp=3.0), TypeError)):
        with pytest.raises(err):
            mask_cutout_batch(d, d, False, True, params)
        with pytest.raises(err):
            mask_cutout_batch(d, d, True, True, params)
        with pytest.raises(err):
            mask_cosmics_batch(d, d, params)
