"""Bad rows and columns ("Bad rows and columns"): the NumPy restatement of the SPEC (tests/_ccdmask.py, the
checker the device kernel is compared with) against the two library calls ccdproc makes (numpy.percentile,
scipy.ndimage.median_filter), hand-made cases of every step, the restatement on synthetic star stamps in float32
against float64, and the Python-side refusals and size range.  No GPU needed."""
import numpy as np
import pytest
import scipy.ndimage as ndi

from tests import _ccdmask as CM

SIZES = (16, 24, 32, 64)


def test_restated_percentile_is_numpys():
    """Bit-equal to np.percentile for float32 input from NumPy 2 on; an older NumPy interpolates in float64, and the
    bound is then 1e-6 of max(|a|, |b|) of the two order statistics: three float32 roundings with a margin of five."""
    rng = np.random.default_rng(0)
    exact = int(np.__version__.split('.')[0]) >= 2
    for it in range(400):
        m = int(rng.integers(64, 16385))
        x = (rng.standard_normal(m) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
        for p in (69.1, 30.9):
            got, want = CM.percentile(x, p), np.percentile(x, p)
            assert got.dtype == np.float32
            if exact:
                assert want.dtype == np.float32 and got == want, (m, p, got, want)
            else:
                s = np.sort(x)
                lo = int(np.floor((m - 1) * p / 100.0))
                assert abs(float(got) - float(want)) <= 1e-6 * max(abs(s[lo]), abs(s[min(lo + 1, m - 1)]))
    stack = rng.standard_normal((5, 333)).astype(np.float32)            # along the last axis of a stack
    assert np.array_equal(CM.percentile(stack, 69.1), np.array([CM.percentile(r, 69.1) for r in stack]))


@pytest.mark.parametrize('n', [8, 9, 24, 33])
def test_restated_median_is_scipys(n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((3, n, n)).astype(np.float32)
    X[1] = np.round(X[1] * 2)                                            # ties
    for k in range(3):
        assert np.array_equal(CM.med7x7(X[k]), ndi.median_filter(X[k], size=(7, 7)))
    assert np.array_equal(CM.med7x7(X), np.stack([ndi.median_filter(x, size=(7, 7)) for x in X]))


def _column(n, *lines):
    c = np.zeros(n, bool)
    c[list(lines)] = True
    return c


@pytest.mark.parametrize('n', [8, 16])
def test_short_gaps_by_hand(n):
    """Step 5 with ngood = 5: a gap is filled when its ends are 2 .. 6 lines apart and the upper end is at line
    n - 7 or above, in the in-place order of ccdproc's loops."""
    M = np.zeros((n, n), bool)
    want = np.zeros((n, n), bool)
    M[:, 0] = _column(n, 0, 2)
    want[:, 0] = _column(n, 0, 1, 2)                          # 2 apart: filled
    M[:, 1] = _column(n, 1, 7)
    want[:, 1] = _column(n, *range(1, 8))                     # 6 apart: filled
    M[:, 2] = _column(n, 0, 7)
    want[:, 2] = _column(n, 0, 7)                             # 7 apart: not filled
    M[:, 3] = _column(n, n - 8, n - 6, n - 1)
    want[:, 3] = _column(n, *range(n - 8, n))                 # the fill from n - 8 sets n - 7, which reaches n - 1
    M[:, 4] = _column(n, n - 6, n - 1)
    want[:, 4] = _column(n, n - 6, n - 1)                     # an original pixel below n - 7 never starts
    M[:, 5] = _column(n, n - 7, n - 1)
    want[:, 5] = _column(n, *range(n - 7, n))                 # the last startable line
    M[:, 6] = _column(n, n - 6, n - 2)
    want[:, 6] = _column(n, n - 6, n - 2)
    got = CM.fill_short_gaps(M.copy())
    assert np.array_equal(got, want)
    # the literal loops of the SPEC, one column at a time
    lit = M.copy()
    for c in range(n):
        for line in range(0, n - 5 - 1):
            if lit[line, c]:
                for i in range(2, 5 + 2):
                    if lit[line + i, c]:
                        lit[line:line + i, c] = True
    assert np.array_equal(lit, want)
    # through ccdmask: NaN pixels are the flagged ones, sigma is NaN and the threshold adds nothing
    d = np.zeros((n, n), np.float32)
    d[M] = np.nan
    r = CM.ccdmask(d)
    assert np.isnan(r['sigma'][0]) and np.array_equal(r['mask4'], M) and np.array_equal(r['mask'], want)
    assert np.array_equal(CM.ccdmask(d, findbadcolumns=False)['mask'], M)


@pytest.mark.parametrize('n', [8, 16])
def test_threshold_and_reduction_by_hand(n):
    rng = np.random.default_rng(n)
    r = CM.ccdmask(np.full((n, n), 0.25, np.float32))
    assert r['sigma'][0] == 0 and not r['mask'].any() and not r['rowcol'].any()          # constant: nothing

    q = CM.quantised_stamp(n)
    r = CM.ccdmask(q)
    assert r['sigma'][0] == 0 and np.array_equal(r['R'] != 0, q != 3.0)
    assert np.array_equal(r['mask4'], r['R'] != 0) and r['mask4'].sum() == 4             # sigma = 0: every non-zero R

    noise = rng.standard_normal((n, n)).astype(np.float32)
    d = noise.copy()
    d[:, :3] = np.nan                                                                    # a partial cutout
    r = CM.ccdmask(d)
    strip = np.zeros((n, n), bool)
    strip[:, :3] = True
    assert np.isnan(r['sigma'][0]) and np.array_equal(r['mask'], strip) and np.array_equal(r['rowcol'], strip)
    assert r['bad_cols'].tolist() == [True] * 3 + [False] * (n - 3) and not r['bad_rows'].any()
    d = noise.copy()
    d[np.arange(n) % 2 == 0, 0] = np.inf                                                 # +-inf: this project's own rule
    d[n - 1, 0] = -np.inf
    r = CM.ccdmask(d)
    assert np.isnan(r['sigma'][0]) and np.array_equal(r['mask4'], ~np.isfinite(d)) and r['bad_cols'].tolist()[0]

    d = noise.copy()
    d[:n - 1, 2] += 100.0                                                                # flagged at the top end only
    r = CM.ccdmask(d)
    assert r['mask'][:n - 1, 2].all() and not r['mask'][n - 1, 2]
    assert not r['bad_cols'].any() and not r['bad_rows'].any() and not r['rowcol'].any()

    d = noise.copy()
    d[:, 5] += 100.0
    d[2, :] -= 100.0                                           # the crossing pixel cancels: a gap of one in the column
    r = CM.ccdmask(d)
    assert not r['mask4'][2, 5] and r['mask'][2, 5]
    assert np.flatnonzero(r['bad_cols']).tolist() == [5] and np.flatnonzero(r['bad_rows']).tolist() == [2]
    cross = np.zeros((n, n), bool)
    cross[:, 5] = cross[2, :] = True
    assert np.array_equal(r['rowcol'], cross)


@pytest.mark.parametrize('n', SIZES)
def test_clean_star_stamps_have_no_line(n):
    d, _ = CM.star_stamps(n)
    r = CM.ccdmask(d)
    lines = r['bad_cols'].any(axis=1) | r['bad_rows'].any(axis=1)
    print(f'n={n}: stamps with a line {lines.sum()} of {len(d)}, pixels over the threshold {r["mask4"].sum()}')
    assert r['mask4'].any()                                   # the threshold does flag the star cores
    assert not lines.any() and not r['rowcol'].any()


@pytest.mark.parametrize('n', SIZES)
def test_injected_lines_are_found(n):
    d, nm = CM.star_stamps(n)
    d, cols, rows = CM.inject_lines(d, nm, np.random.default_rng(n))
    found = CM.lines_found(CM.ccdmask(d), cols, rows)
    print(f'n={n}: injected lines found in {found.sum()} of {len(d)} stamps')
    assert found.sum() >= len(d) // 2


def test_float32_against_float64_outside_the_ambiguous_set():
    """A pixel is ambiguous when R lies within 1e-4 relative of one of its two thresholds, in either precision.  The
    masks of the threshold agree outside that set, every output agrees on the stamps without such a pixel, and the set
    is capped at 0.1 % of the pixels (the cap of the cosmics)."""
    total = amb_total = 0
    for n in SIZES:
        d, nm = CM.star_stamps(n)
        d, _, _ = CM.inject_lines(d, nm, np.random.default_rng(n))
        r32, r64 = CM.ccdmask(d), CM.ccdmask(d, dtype=np.float64)
        amb = np.zeros(d.shape, bool)
        closest = np.inf
        for r in (r32, r64):
            R, s = r['R'].astype(np.float64), r['sigma'].astype(np.float64)[:, None, None]
            for thr in (-9.0 * s, 9.0 * s):
                dist = np.abs(R - thr) / np.abs(thr)
                closest = min(closest, float(dist.min()))
                amb |= dist <= 1e-4
        disagree = (r32['mask4'] != r64['mask4']) & ~amb
        settled = ~amb.reshape(len(d), -1).any(axis=1)
        print(f'n={n}: ambiguous {amb.sum()} of {amb.size} ({amb.mean():.2e}), closest relative distance {closest:.2e}, '
              f'disagreements outside {disagree.sum()}')
        assert not disagree.any()
        for key in ('mask', 'rowcol', 'bad_cols', 'bad_rows'):
            assert np.array_equal(r32[key][settled], r64[key][settled]), key
        assert amb.mean() <= 1e-3
        total += amb.size
        amb_total += amb.sum()
    print(f'ambiguous share over all inputs: {amb_total / total:.2e}')
    assert amb_total / total <= 1e-3


def test_unbuilt_options_are_refused():
    from lightcurver_amd.ccdproc import ccdmask, ccdmask_stamps
    from lightcurver_amd.processes.cutout_making import mask_cosmics_batch
    d = np.zeros((16, 16), np.float32)
    with pytest.raises(NotImplementedError, match='byblocks'):
        ccdmask(d, byblocks=True)
    with pytest.raises(NotImplementedError, match='7 x 7'):
        ccdmask(d, ncmed=5, nlmed=5)
    with pytest.raises(NotImplementedError, match='7 x 7'):
        ccdmask_stamps(d[None], nlmed=5)
    with pytest.raises(NotImplementedError, match='rectangular'):
        ccdmask(np.zeros((16, 24), np.float32))
    with pytest.raises(NotImplementedError, match='rectangular'):
        ccdmask_stamps(np.zeros((2, 16, 24), np.float32))
    with pytest.raises(NotImplementedError, match='ccdmask'):
        mask_cosmics_batch(d[None], d[None] + 1, {}, do_mask_bad_columns=True)


def test_both_switches_off_needs_no_device():
    from lightcurver_amd.processes.cutout_making import mask_cutout_batch
    d = np.ones((3, 16, 16), np.float32)
    m = mask_cutout_batch(d, d, False, False, {})
    assert m.dtype == bool and m.shape == d.shape and not m.any()
    ms = mask_cutout_batch([d[0], np.ones((24, 24), np.float32)], [d[0], np.ones((24, 24), np.float32)], False, False)
    assert [x.shape for x in ms] == [(16, 16), (24, 24)] and not any(x.any() for x in ms)


def test_library_reports_the_stamp_size_range():
    from lightcurver_amd import _lib
    from lightcurver_amd.ccdproc import supported
    lib = _lib.lib()
    assert [n for n in range(0, 200) if lib.lc_ccdmask_supported(n)] == list(range(8, 129))
    assert supported(24) and supported(33) and not supported(7) and not supported(129)


@pytest.mark.parametrize('n,K', CM.SETTINGS_SIZES)
def test_every_settings_case_changes_the_restatement(n, K):
    """The condition of CM.settings_cases: every case gives another ``mask`` than lsigma = hsigma = 9, ngood = 5 on its
    input, so a kernel that ignored the setting would fail the device comparison of tests/test_ccdmask_gpu.py."""
    d, base, cases = CM.settings_wanted(n, K)
    assert [kw for kw, _ in cases] == CM.settings_cases(n) and len(cases) == 13
    by = {}
    for kw, want in cases:
        changed = (want['mask'] != base['mask']).sum()
        print(f'n={n} {kw}: mask pixels changed {changed}, filled {(want["mask"] & ~want["mask4"]).sum()}, lines '
              f'{want["bad_cols"].sum() + want["bad_rows"].sum()}')
        assert changed > 0, kw
        by[tuple(sorted(kw.items()))] = want
    ngood = lambda g: by[(('ngood', g),)]
    # from n - 1 on no line can start a fill: the mask of ngood 0, which is the mask of the threshold
    for g in (n - 1, n, n + 5):
        assert np.array_equal(ngood(g)['mask'], ngood(0)['mask']), g
    assert np.array_equal(ngood(0)['mask'], base['mask4'])
    # n - 2 is the last value at which the fill runs (from line 0 alone), and there it reads the last row: with the low
    # thresholds of the combined case it fills, and some of that hangs on the last row alone
    last = by[(('hsigma', 2), ('lsigma', 2), ('ngood', n - 2))]
    assert (last['mask'] & ~last['mask4']).any()
    blind = last['mask4'].copy()
    blind[:, -1, :] = False
    assert not np.array_equal(CM.fill_short_gaps(blind, n - 2)[:, :-1], last['mask'][:, :-1])
    assert not np.array_equal(last['mask'], CM.ccdmask(d, lsigma=2, hsigma=2, ngood=n - 1)['mask'])
    # a swap of the two thresholds would show: the asymmetric pair is not its mirror image
    assert not np.array_equal(by[(('hsigma', 20), ('lsigma', 3))]['mask'], CM.ccdmask(d, lsigma=20, hsigma=3)['mask'])
    assert not np.array_equal(by[(('lsigma', 3),)]['mask'], by[(('hsigma', 3),)]['mask'])
