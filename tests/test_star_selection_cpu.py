"""processes/star_selection.py: names, the catalogue around the ROI, the two selections of the reference."""
import numpy as np
import pytest

from lightcurver_amd.processes.star_selection import generate_star_names, reference_star_catalogue, select_stars

ROI = np.array([50.0, 40.0])


def table():
    """Eight sources: (x, y, flux, flag); their distances to the ROI are 3, 10, 20, 25, 30, 40, 45, 50."""
    rows = [(50.0, 43.0, 900.0, 0), (60.0, 40.0, 100.0, 0), (50.0, 20.0, 5000.0, 0), (35.0, 20.0, 700.0, 4),
            (80.0, 40.0, 50.0, 0), (50.0, 80.0, 300.0, 0), (50.0, 85.0, 400.0, 0), (100.0, 40.0, 800.0, 0)]
    t = np.zeros(len(rows), [('x', '<f8'), ('y', '<f8'), ('flux', '<f8'), ('flag', '<i4')])
    for i, r in enumerate(rows):
        t[i] = r
    return t[[4, 0, 7, 2, 6, 1, 3, 5]]                   # not in the order of the distances


def test_names():
    names = generate_star_names(26 * 27 + 1)
    assert names[:3] == ['a', 'b', 'c'] and names[25] == 'z' and names[26] == 'aa' and names[27] == 'ab'
    assert names[51] == 'az' and names[52] == 'ba' and names[26 * 27 - 1] == 'zz' and names[26 * 27] == 'aaa'
    assert generate_star_names(0) == [] and len(set(names)) == len(names)


def test_catalogue_exclusion_radius_and_ordering():
    cat = reference_star_catalogue(table(), ROI, 5.0, require_unflagged=False)
    assert cat.dtype.names == ('name', 'x', 'y', 'flux', 'distance_to_roi')
    assert cat['distance_to_roi'].tolist() == [10.0, 20.0, 25.0, 30.0, 40.0, 45.0, 50.0]
    assert cat['name'].tolist() == list('abcdefg')
    assert cat['flux'].tolist() == [100.0, 5000.0, 700.0, 50.0, 300.0, 400.0, 800.0]
    assert cat['x'].tolist() == [60.0, 50.0, 35.0, 80.0, 50.0, 50.0, 100.0]
    # the radius is exclusive of what lies on it
    assert len(reference_star_catalogue(table(), ROI, 10.0, require_unflagged=False)) == 6
    assert len(reference_star_catalogue(table(), ROI, 0.0, require_unflagged=False)) == 8
    # the flag column
    assert reference_star_catalogue(table(), ROI, 5.0)['distance_to_roi'].tolist() == [10.0, 20.0, 30.0, 40.0, 45.0, 50.0]
    # plain arrays, and a dict of characterize_frames
    t = table()
    plain = reference_star_catalogue(np.stack([t['x'], t['y'], t['flux']], axis=1), ROI, 5.0)
    assert np.array_equal(plain, cat)
    assert np.isnan(reference_star_catalogue(np.stack([t['x'], t['y']], axis=1), ROI, 5.0)['flux']).all()
    assert np.array_equal(reference_star_catalogue(dict(sources_table=t), ROI, 5.0, require_unflagged=False), cat)
    # a source without a position is dropped
    t['x'][0] = np.nan
    assert len(reference_star_catalogue(t, ROI, 5.0, require_unflagged=False)) == 6


def test_catalogue_optional_cuts():
    cat = reference_star_catalogue(table(), ROI, 5.0, flux_range=(100.0, 800.0), require_unflagged=False)
    assert cat['flux'].tolist() == [100.0, 700.0, 300.0, 400.0, 800.0] and cat['name'].tolist() == list('abcde')
    # isolation counts every source of the table: the pair 5 px apart goes, and so does the star 7 px from the dropped
    # source next to the ROI (distance 10: (60, 40) is sqrt(109) from (50, 43))
    cat = reference_star_catalogue(table(), ROI, 5.0, min_isolation=12.0, require_unflagged=False)
    assert cat['distance_to_roi'].tolist() == [20.0, 25.0, 30.0, 50.0]
    assert reference_star_catalogue(table(), ROI, 5.0, min_isolation=5.0, require_unflagged=False)['distance_to_roi'].tolist() \
        == [10.0, 20.0, 25.0, 30.0, 40.0, 45.0, 50.0]


def test_select_stars():
    rng = np.random.default_rng(2)
    xy = np.stack([ROI[0] + np.arange(1, 15) * 6.0, np.full(14, ROI[1])], axis=1)[rng.permutation(14)]
    cat = reference_star_catalogue(xy, ROI, 1.0)
    assert cat['name'].tolist() == list('abcdefghijklmn')
    names = lambda idx: cat['name'][idx].tolist()
    assert names(select_stars(cat)) == list('abcdefghij')                          # None: the 10 nearest
    assert names(select_stars(cat, 3)) == list('abc')
    assert names(select_stars(cat, 30)) == list('abcdefghijklmn')
    assert names(select_stars(cat, ['m', 'b', 'zz', 'd'])) == list('bdm')           # a list: those names, catalogue order
    assert names(select_stars(cat, 5, ['b', 'd'])) == list('ace')                   # exclusion after selection: 3 left, not 5
    assert names(select_stars(cat, 5, 'bd')) == list('ace')                         # a string: each character a name
    assert names(select_stars(cat, ['a', 'b'], ['b'])) == ['a']                     # exclusion takes precedence
    assert names(select_stars(cat, None, [])) == list('abcdefghij')
    available = np.ones(14, bool)
    available[[0, 2]] = False
    assert names(select_stars(cat, 3, available=available)) == list('bde')          # availability before the cut
    assert names(select_stars(cat, 3, 'b', available=available)) == list('de')
    assert names(select_stars(cat, ['a', 'b'], available=available)) == ['b']
    assert select_stars(cat, 0).size == 0
    with pytest.raises(RuntimeError, match='stars_to_use'):
        select_stars(cat, 'abc')
    with pytest.raises(RuntimeError, match='stars_to_use'):
        select_stars(cat, 2.0)
    with pytest.raises(RuntimeError, match='stars_to_exclude'):
        select_stars(cat, 3, ('a', 'b'))
    with pytest.raises(ValueError):
        select_stars(cat, 3, available=np.ones(3, bool))
