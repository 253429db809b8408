"""The source-masking SPEC (DESIGN.md §5 "Source masking") without a device: its NumPy restatement (tests/_segment.py)
against the float64 host form ``processes/source_masking.extract``, the exactness of its fixed-point sums, the scene
generator's coverage of every path, and the size query of the library."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _segment as SG

# (n, K, seed): seeds for which the restatement stays within the 1 % cap below.  Where the two forms differ it is by
# single left-over pixels whose dist^2 / size^2 to two branches is an exact tie (size^2 = area / pi, so d1^2 / a1 =
# d2^2 / a2 happens with small integers): each form's rounding decides it.  Over seeds 1 - 6 that was 13 of 960 stamps
# at 32^2, 1 of 384 at 64^2.
SCENE_SETS = [(32, 160, 3), (32, 160, 5), (48, 64, 3), (64, 64, 1)]


def test_restatement_agrees_with_the_host_extract():
    from lightcurver_amd.processes.psf_modelling import mask_surrounding_stars
    from lightcurver_amd.processes.source_masking import extract
    total, differ = 0, []
    took = dict(split=0, deeper=0, merged=0, zero=0, central_fainter=0, nan_border=0)
    for n, K, seed in SCENE_SETS:
        d, s, kinds = SG.make_scenes(K, n, seed)
        assert set(kinds) == set(SG.SCENES)
        r = SG.segment(d, s)
        assert np.all(r['status'] == 0)
        for k in range(K):
            objects, _ = extract(d[k], s[k])
            mask = mask_surrounding_stars(d[k], s[k])
            if len(objects) != r['nobj'][k] or not np.array_equal(mask, r['mask'][k]):
                differ.append((n, seed, k, kinds[k], len(objects), int(r['nobj'][k]), int((mask != r['mask'][k]).sum())))
            p = r['paths'][k]
            took['split'] += p['split']
            took['deeper'] += p['depth'] >= 2
            took['merged'] += p['merged'] > 0
            took['zero'] += p['zero']
            took['central_fainter'] += p['central_fainter']
            took['nan_border'] += bool(np.isnan(d[k]).any() and r['nobj'][k] > 0)
        total += K
    print(f'{len(differ)} of {total} stamps differ (n, seed, stamp, kind, host objects, SPEC objects, mask pixels):')
    for row in differ:
        print('  ', row)
    print('paths taken:', took)
    assert all(v > 0 for v in took.values()), took
    assert len(differ) <= 0.01 * total


def test_each_scene_kind_takes_its_path():
    d, s, kinds = SG.make_scenes(64, 32, seed=3)
    r = SG.segment(d, s)
    by = {kind: [r['paths'][k] for k in range(64) if kinds[k] == kind] for kind in SG.SCENES}
    nobj = {kind: [int(r['nobj'][k]) for k in range(64) if kinds[k] == kind] for kind in SG.SCENES}
    assert all(p['zero'] for p in by['noise_only'])
    assert all(n == 1 for n in nobj['single'])
    assert sum(p['split'] for p in by['blend']) >= 6
    assert sum(p['depth'] >= 2 for p in by['chain']) >= 4
    assert sum(p['central_fainter'] for p in by['offcentre_bright']) >= 6
    assert any(p['merged'] for p in by['wing_fragment'])


def test_fixed_point_sums_are_exact_on_the_stated_range():
    """Every value below 2^16 quantises to q < 2^36; q x^2 < 2^48 at x <= 63; 4096 of them stay below 2^60: the int64
    sums neither overflow nor depend on the order, checked against Python's unbounded integers at the top of the range."""
    rng = np.random.default_rng(0)
    n = 64
    top = np.nextafter(np.float32(SG.SNR_LIMIT), np.float32(0))
    for snr in (np.full((n, n), top, np.float32), rng.uniform(3, 65535, (n, n)).astype(np.float32),
                rng.uniform(3, 8, (n, n)).astype(np.float32)):
        m = np.ones((n, n), bool)
        got = SG.fixed_sums(snr, m)
        q = [int(v) for v in SG.quantise(snr).ravel()]
        assert max(q) < 2 ** 36
        yy, xx = [int(v) for v in np.repeat(np.arange(n), n)], [int(v) for v in np.tile(np.arange(n), n)]
        exact = (n * n, sum(q), sum(a * x for a, x in zip(q, xx)), sum(a * y for a, y in zip(q, yy)),
                 sum(a * x * x for a, x in zip(q, xx)), sum(a * y * y for a, y in zip(q, yy)),
                 sum(a * x * y for a, x, y in zip(q, xx, yy)))
        assert got == exact and max(exact) < 2 ** 62
        perm = rng.permutation(n * n)
        qa = SG.quantise(snr).ravel()
        assert int((qa[perm] * np.asarray(xx)[perm] ** 2).sum()) == exact[4]
    # the quantisation itself: v 2^20 is exact, so q is the nearest integer of the exact product, ties to even
    v = np.array([3.0, 3.0000002, 7.9999995, 8.0, 65535.996, 2.5 * 2.0 ** -20, 3.5 * 2.0 ** -20], np.float32)
    assert SG.quantise(v).tolist() == [round(Fraction(float(x)) * 2 ** 20) for x in v]      # (round: ties to even)
    assert SG.quantise(v).tolist()[-2:] == [2, 4] and SG.quantise(v)[3] == 8 << 20
    # a detected value at or beyond the range is reported, not summed
    d = np.zeros((16, 16), np.float32)
    d[4:10, 4:10] = 1e6
    r = SG.segment_one(d, np.ones((16, 16), np.float32))
    assert r['status'] == 3 and r['mask'].all() and r['nobj'] == 0


def test_levels_are_successive_square_roots():
    for nthresh in (4, 8, 16, 32):
        lev = SG.levels(np.float32(811.5), np.float32(3.0), nthresh)
        assert len(lev) == nthresh - 1 and all(x.dtype == np.float32 for x in lev)
        want = 3.0 * (811.5 / 3.0) ** (np.arange(1, nthresh) / nthresh)
        assert np.allclose(lev, want, rtol=2e-5) and np.all(np.diff(lev) > 0)


def test_full_table_is_status_1():
    d, s = SG.crowded_stamp(64)
    r = SG.segment_one(d, s)
    assert r['status'] == 1 and r['mask'].all() and r['nobj'] == 0 and not r['segmap'].any()


def test_segment_supported_needs_no_device():
    from lightcurver_amd import _lib
    lib = _lib.lib()
    assert [n for n in range(0, 140) if lib.lc_segment_supported(n)] == list(range(8, 65))
    assert _lib.SEGMENT_MAX_OBJECTS == SG.OBJ_CAP == 32


@pytest.mark.parametrize('n,K', SG.SETTINGS_SIZES)
def test_every_settings_case_changes_the_restatement(n, K):
    """The condition of SG.SETTINGS: every case gives another segmap than its base and than the defaults on its input
    (and stays inside the tables: status 0), so a kernel that ignored the setting would fail the device comparison of
    tests/test_segment_gpu.py."""
    cases = SG.settings_wanted(n, K)
    assert len(cases) == sum(n in sizes for _, _, _, sizes in SG.SETTINGS) >= len(SG.SETTINGS) - 1
    for kw, d, s, want, base, plain in cases:
        diff = (want['segmap'] != base['segmap']).any(axis=(1, 2))
        print(f'n={n} {kw}: stamps whose segmap differs from the base {diff.sum()} of {K}, from the defaults '
              f'{(want["segmap"] != plain["segmap"]).any(axis=(1, 2)).sum()}; objects {np.bincount(want["nobj"]).tolist()}, '
              f'status {np.bincount(want["status"]).tolist()}')
        assert diff.any() and not np.array_equal(want['segmap'], plain['segmap']), kw
        assert np.all(want['status'] == 0), kw
    by = {tuple(sorted(kw.items())): (want, base) for kw, d, s, want, base, plain in cases}
    want, base = by[(('deblend_cont', 0.05),)]
    assert (want['nobj'][0::2] < base['nobj'][0::2]).any()          # 0.05 merges what 0.001 splits: the 1 % secondaries
    want, base = by[(('clean', False), ('deblend_cont', 1e-06))]
    assert (want['nobj'][1::2] > base['nobj'][1::2]).any()          # 1e-6 splits what 0.001 merges: the faint ones
    want, base = by[(('deblend_cont', 1e-05), ('minarea', 3), ('thresh', 1.5))]
    assert want['nobj'].max() >= 7
    assert all(n in sizes for _, _, _, sizes in SG.SETTINGS if sizes != (24,))
