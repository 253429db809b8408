"""The restatement of the aperture SPEC (tests/_aperture.py, DESIGN.md §5 "Aperture sums") against closed-form geometry
and 50-digit arithmetic, and the host parts of the feature: the facade's refusals that need no library, and the default
starting fluxes of the ROI fit, which stay the pixel-centre sums."""
import math

import numpy as np
import pytest

from tests import _aperture as A

CORNER = math.pi / 12 - (math.sqrt(3) - 1) / 4     # r = 1 on a pixel centre: the diagonal neighbours
EDGE = (math.pi - 1 - 4 * CORNER) / 4               # the edge neighbours


def test_unit_circle_on_a_pixel_centre():
    assert abs(CORNER - 0.078786686) < 1e-9 and abs(EDGE - 0.456611478) < 1e-9
    f = A.fractions(5, 5, 2.0, 2.0, 1.0)
    want = np.zeros((5, 5))
    want[1:4, 1:4] = [[CORNER, EDGE, CORNER], [EDGE, 1.0, EDGE], [CORNER, EDGE, CORNER]]
    print('max deviation from the known answers', np.abs(f - want).max(), 'total - pi', f.sum() - math.pi)
    assert np.abs(f - want).max() <= 1e-14
    assert abs(f.sum() - math.pi) <= 1e-14
    for i in range(5):
        for j in range(5):
            assert abs(A.pixel_fraction(i, j, 2.0, 2.0, 1.0) - want[i, j]) <= 1e-14


def test_fractions_sum_to_the_area_of_the_circle():
    """For a circle inside the image.  Each of the (2 r + 2)^2 fractions of the box carries the closed form's error, at most
    4 x 2^-53 max(1, pi r^2) (the test below), and the float64 sum adds less than that again."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for r in [0.2, 0.3, 0.5, 1.0, 2.5, 3.0, 7.7, 20.0, 40.0] + list(np.exp(rng.uniform(np.log(0.2), np.log(40.0), 20))):
        xc, yc = rng.uniform(45, 55, 2)
        f = A.fractions(100, 100, xc, yc, r)
        assert f.min() >= 0.0 and f.max() <= 1.0
        tol = 8 * A.EPS * max(1.0, math.pi * r * r) * (2 * r + 2) ** 2
        worst = max(worst, abs(f.sum() - math.pi * r * r) / tol)
        assert abs(f.sum() - math.pi * r * r) <= tol, r
    print('worst |sum - pi r^2| / tolerance', worst)


def test_restatement_against_50_digit_arithmetic():
    cases = A.tangent_cases(100, 100)
    assert len(cases) == 200 and sum(c[5] is not None for c in cases) >= 100 and max(c[4] for c in cases) <= 64.0
    worst, rim = 0.0, 0
    for i, j, xc, yc, r, tangent in cases:
        got, want = A.pixel_fraction(i, j, xc, yc, r), A.mp_pixel_fraction(i, j, xc, yc, r)
        if tangent:
            # the edge is 1e-12 .. 1e-5 px from the circle's extreme (the centre's rounding moves it by an ulp of ~100)
            extreme = xc + r if tangent == 'x' else yc + r
            assert 5e-13 <= abs((extreme % 1) - 0.5) <= 2e-5
        rim += 0.0 < want < 1.0
        ratio = abs(got - min(max(want, 0.0), 1.0)) / (4 * A.EPS * max(1.0, math.pi * r * r))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (i, j, xc, yc, r, got, want)
    print('worst |restatement - mpmath| / (4 x 2^-53 max(1, pi r^2))', worst, '; rim pixels', rim)
    assert rim >= 100


def test_good_pixel_rule_of_the_restatement():
    d = np.ones((5, 5), np.float32)
    e = np.full((5, 5), 2.0, np.float32)
    s, se, a, b = A.aperture_sums(d, 2.0, 2.0, 1.0, e)
    assert abs(s - math.pi) < 1e-14 and abs(se - 2 * math.sqrt(math.pi)) < 1e-14 and abs(a - math.pi) < 1e-14 and b == 0
    d[2, 3] = np.nan
    e[1, 2] = np.inf
    m = np.zeros((5, 5), np.uint8)
    m[3, 2] = 1
    s, se, a, b = A.aperture_sums(d, 2.0, 2.0, 1.0, e, m)
    assert abs(a - (math.pi - 3 * EDGE)) < 1e-14 and abs(b - 2 * EDGE) < 1e-14 and abs(s - a) < 1e-14
    assert A.aperture_sums(d, 30.0, 2.0, 1.0) == (0.0, None, 0.0, 0.0)


def test_facade_refuses_without_the_library(monkeypatch):
    from lightcurver_amd import _lib, photutils as P

    def no_library(*a, **k):
        raise AssertionError('the library was touched')

    monkeypatch.setattr(_lib, 'lib', no_library)
    monkeypatch.setattr(_lib, 'default_context', no_library)
    img = np.zeros((8, 9), np.float32)
    ap = P.CircularAperture([(3.0, 4.0), (1.0, 2.0)], r=2.0)
    assert len(ap) == 2 and not ap.isscalar and P.CircularAperture((3.0, 4.0), 2.0).isscalar
    for method in ('center', 'subpixel'):
        with pytest.raises(NotImplementedError):
            P.aperture_photometry(img, ap, method=method)
    with pytest.raises(ValueError):
        P.aperture_photometry(np.zeros((2, 8, 9), np.float32), ap)
    with pytest.raises(ValueError):
        P.aperture_photometry(img, ap, error=np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError):
        P.aperture_photometry(img, ap, mask=np.zeros((9, 8), bool))
    for bad in ([1.0, 2.0, 3.0], [[1.0, 2.0, 3.0]], 5.0):
        with pytest.raises(ValueError):
            P.CircularAperture(bad, 2.0)
    for bad_r in (0.0, -1.0, np.nan, [1.0, 2.0]):
        with pytest.raises(ValueError):
            P.CircularAperture((1.0, 2.0), bad_r)
    with pytest.raises(ValueError):
        P.aperture_sums_batch(img, 0, [(1.0, 2.0)], 2.0)                      # not a (K, h, w) stack
    with pytest.raises(ValueError):
        P.aperture_sums_batch(img[None], [0, 0, 0], [(1.0, 2.0), (2.0, 3.0)], 2.0)
    with pytest.raises(ValueError):
        P.aperture_sums_batch(img[None], 1, [(1.0, 2.0)], 2.0)                # an image index outside the stack
    out = P.aperture_sums_batch(img[None], 0, np.zeros((0, 2)), 2.0)          # no aperture: no call
    assert all(out[k].shape == (0,) for k in ('sum', 'area', 'bad_area')) and out['sum_err'] is None


def test_default_starting_fluxes_stay_the_pixel_centre_sums():
    """``initial_point_source_fluxes`` with its defaults: the sum of the median stack over the pixels whose centre lies
    inside the circle, NaN counting as zero."""
    from lightcurver_amd.processes.roi_modelling import initial_point_source_fluxes
    rng = np.random.default_rng(11)
    data = rng.normal(1.0, 0.3, (5, 16, 16))
    data[2, 8, 8] = np.nan
    xs, ys, radius = [7.3, 4.6], [8.2, 4.1], 3.0
    stack = np.nanmedian(data, axis=0)
    yy, xx = np.mgrid[0:16, 0:16]
    want = [float(np.nansum(stack[(xx - x) ** 2 + (yy - y) ** 2 <= radius ** 2])) for x, y in zip(xs, ys)]
    assert initial_point_source_fluxes(data, xs, ys, radius) == want
    assert initial_point_source_fluxes(data, xs, ys, radius, method='center') == want
    with pytest.raises(ValueError):
        initial_point_source_fluxes(data, xs, ys, radius, method='subpixel')
