"""The restatement of the registration SPEC (tests/_register.py, DESIGN.md §5 "Frame registration") against itself, the
condition on the inputs of the device tests (their decision margins), and the host parts of the feature: the WCS algebra,
the positions in frames, the facade's transform and the refusals that need no device."""
import math

import numpy as np
import pytest

from tests import _register as R

CASES = R.cases()
SOLVED_WITH_TRUTH = [n for n, c in CASES.items() if c[3] is not None and c[4] == 0]


def _row(truth):
    a, b, tx, ty = truth
    return np.array([a, -b, tx, b, a, ty])


@pytest.mark.parametrize('name', SOLVED_WITH_TRUTH)
def test_restatement_recovers_the_transform(name):
    """A least-squares similarity through m >= 3 pairs whose targets are jittered by sigma errs by about sigma sqrt(4 / m)
    inside the hull of the pairs and by less than 2 sigma even at m = 3; the matched source points map to within 3 sigma
    of where the true transform puts them (the sigmas are those of R.cases())."""
    sigma = dict(n50_plain=0.1, n50_rot25=0.3, n50_rot170=0.3, n12_rot40=0.2, n6_rot10=0.1, n50_scale1p5=0.3, n50_rot90=0.5,
                 n3=0.05, n4=0.05, n5=0.05, n7_vs_50=0.1)[name]
    S, T, mm, truth, status = CASES[name]
    r = R.solved(name)
    assert r['status'] == 0 and r['diag'][3] >= 0 and len(r['pairs']) >= 3
    print(name, 'diag', r['diag'].tolist(), 'pairs', len(r['pairs']))
    got, want = r['transform'], _row(truth)
    pts = S[r['pairs'][:, 0]]
    diff = (pts @ got.reshape(2, 3)[:, :2].T + got[[2, 5]]) - (pts @ want.reshape(2, 3)[:, :2].T + want[[2, 5]])
    assert np.sqrt((diff ** 2).sum(axis=1)).max() < 3 * sigma
    # the pairs are true pairs wherever the target kept its star: the target of s lies within pixel_tol of its image
    pred = pts @ got.reshape(2, 3)[:, :2].T + got[[2, 5]]
    assert np.sqrt(((pred - T[r['pairs'][:, 1]]) ** 2).sum(axis=1)).max() < R.PIXEL_TOL
    assert (np.diff(r['pairs'][:, 0]) > 0).all()


def test_larger_list_against_smaller_and_the_inverse():
    r = R.solved('n128_vs_50')
    assert r['status'] == 0 and r['diag'][0] > r['diag'][1] and len(r['pairs']) >= 10
    a, b = r['transform'][0], r['transform'][3]
    assert abs(math.degrees(math.atan2(b, a)) + 12.0) < 0.1 and abs(math.hypot(a, b) - 1.0) < 1e-3     # the inverse of +12 degrees


def test_unrelated_target_exhausts_every_hypothesis():
    r = R.solved('unrelated')
    assert r['status'] == 1 and r['diag'][2] > 1000 and r['diag'][3] == -1 and r['diag'][4] == 0
    assert np.isnan(r['transform']).all() and len(r['pairs']) == 0


def test_statuses_two_and_three():
    assert R.solved('too_many')['status'] == 2 and R.solved('too_many')['diag'][2] > 64
    assert R.solved('two_points')['status'] == 3
    assert R.register(np.zeros((5, 2)), CASES['n5'][1])['status'] == 1          # coincident points: no triangle at all


def test_single_match_special_case():
    r = R.solved('n3')
    assert r['diag'].tolist() == [1, 1, 1, 0, 1] and r['status'] == 0 and len(r['pairs']) == 3


def test_lattice_ties_and_congruent_triangles():
    S, T = CASES['lattice'][:2]
    vs, inv = R.triangles(S)
    # every neighbourhood of a lattice point holds tied distances: the index rule decided, and still no vertex set is twice there
    assert len({frozenset(v) for v in vs.tolist()}) == len(vs)
    r = R.solved('lattice')
    assert r['diag'][2] > 20 * len(vs)              # congruent triangles in numbers
    assert r['status'] == 0


@pytest.mark.parametrize('seed', range(5))
def test_closed_form_fit_is_umeyama(seed):
    rng = np.random.default_rng(seed)
    m = int(rng.integers(3, 40))
    s = rng.uniform(0, 2000, (m, 2))
    th, sc = rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 2.0)
    M = sc * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    t = s @ M.T + rng.uniform(-100, 100, 2) + rng.normal(0, 0.5, (m, 2))
    a, b, tx, ty = R.fit(s, t)
    U = R.umeyama(s, t)
    assert np.allclose([[a, -b], [b, a]], U[:2, :2], rtol=0, atol=1e-12)
    assert np.allclose([tx, ty], U[:2, 2], rtol=0, atol=1e-8)
    assert R.fit(np.zeros((3, 2)), t[:3]) is None and R.fit(s[:0], t[:0]) is None


@pytest.mark.parametrize('name', sorted(CASES))
def test_decision_margins_of_the_device_cases(name):
    """A condition on the INPUTS of tests/test_register_gpu.py: no comparison of the restatement is closer to its
    threshold than the device's different order of summation could move it."""
    m = R.solved(name)['margins']
    print(name, m)
    assert m['radius'] >= 1e-6 and m['error'] >= 1e-6
    if name != 'lattice':            # its squared distances are exact integers: ties are ties, the rest differ by >= 1
        assert m['d2'] >= 1e-9


def test_rendered_frames_margins_and_centroid_bound():
    """The end-to-end frames: the restatement registers frames 0 - 2 on the restated tables and fails on frame 3; the
    worst centroid error of tests/_extract.extract is what DESIGN.md quotes (its bound is three times that)."""
    r = R.rendered()
    worst = R.worst_centroid_error()
    print('worst centroid error of the restated extraction: %.4f px' % worst)
    assert 0 < worst < 0.1
    for k in range(4):
        q = R.register(r['tables'][0], r['tables'][k])
        print(k, q['status'], q['diag'].tolist(), q['margins'])
        assert q['status'] == (0 if k < 3 else 1)
        assert q['margins']['radius'] >= 1e-6 and q['margins']['error'] >= 1e-6 and q['margins']['d2'] >= 1e-9
        if k < 3:
            a, b, tx, ty = q['transform'][[0, 3, 2, 5]]
            pred = np.stack([a * r['field'][:, 0] - b * r['field'][:, 1] + tx, b * r['field'][:, 0] + a * r['field'][:, 1] + ty], 1)
            ta, tb, ttx, tty = r['truth'][k]
            true = np.stack([ta * r['field'][:, 0] - tb * r['field'][:, 1] + ttx, tb * r['field'][:, 0] + ta * r['field'][:, 1] + tty], 1)
            assert np.sqrt(((pred - true) ** 2).sum(axis=1)).max() < 3 * worst


# ---- the host parts of the product ----------------------------------------------------------------------------------------

def test_wcs_helpers_are_the_references_formulas():
    from lightcurver_amd.astroalign import SimilarityTransform
    from lightcurver_amd.processes.plate_solving import adapt_wcs_arrays, refine_wcs_arrays
    th, sc = math.radians(17.0), 1.03
    a, b = sc * math.cos(th), sc * math.sin(th)
    tr = SimilarityTransform.from_row([a, -b, 12.5, b, a, -7.25])
    crpix = np.array([1023.5, 987.25])
    cd = np.array([[-7.3e-5, 1.1e-6], [1.2e-6, 7.2e-5]])
    # adapt_existing_wcs.py:29-40
    similarity = tr.params
    scaled_rotation, translation = similarity[:2, :2], similarity[:2, 2]
    got = adapt_wcs_arrays(crpix, cd, tr)
    assert np.array_equal(got[0], np.dot(scaled_rotation, crpix) + translation)
    assert np.array_equal(got[1], np.dot(scaled_rotation, cd))
    # with_gaia.py:71-73
    got = refine_wcs_arrays(crpix, cd, tr)
    assert np.allclose(got[0], tr.inverse.params[:2, :2] @ crpix + tr.inverse.translation, rtol=1e-14, atol=0)
    assert np.allclose(got[1], tr.inverse.params[:2, :2] @ cd, rtol=1e-14, atol=0)
    # the two undo each other, and the six-number row and the 3 x 3 matrix are taken too
    back = refine_wcs_arrays(*adapt_wcs_arrays(crpix, cd, tr.params), [a, -b, 12.5, b, a, -7.25])
    assert np.allclose(back[0], crpix, rtol=1e-12) and np.allclose(back[1], cd, rtol=1e-12)


def test_similarity_transform_facade():
    from lightcurver_amd.astroalign import SimilarityTransform
    th, sc = math.radians(-33.0), 0.97
    a, b = sc * math.cos(th), sc * math.sin(th)
    tr = SimilarityTransform.from_row([a, -b, 3.0, b, a, 4.0])
    assert tr.params.shape == (3, 3) and np.array_equal(tr.params[2], [0, 0, 1])
    assert abs(tr.scale - sc) < 1e-15 and abs(tr.rotation - th) < 1e-15 and np.array_equal(tr.translation, [3.0, 4.0])
    p = np.array([[10.0, 20.0], [-5.0, 0.5]])
    q = tr(p)
    assert np.allclose(q[0], [a * 10 - b * 20 + 3, b * 10 + a * 20 + 4], rtol=1e-15)
    assert np.allclose(tr.inverse(q), p, rtol=1e-13, atol=1e-13)


def test_positions_in_frames_gives_nan_for_failed_frames():
    from lightcurver_amd.astroalign import SimilarityTransform
    from lightcurver_amd.processes.plate_solving import positions_in_frames
    tr = SimilarityTransform.from_row([0.0, -1.0, 5.0, 1.0, 0.0, 6.0])
    results = [dict(transform=SimilarityTransform(), success=True), dict(transform=None, success=False),
               dict(transform=tr, success=True)]
    pos = np.array([[1.0, 2.0], [30.0, 40.0], [7.5, -2.5]])
    out = positions_in_frames(results, pos)
    assert len(out) == 3 and all(o.shape == (3, 2) for o in out)
    assert np.array_equal(out[0], pos) and np.isnan(out[1]).all()
    assert np.array_equal(out[2], np.stack([-pos[:, 1] + 5.0, pos[:, 0] + 6.0], axis=1))


def test_table_positions_orders_by_flux_and_takes_dicts():
    from lightcurver_amd.processes.plate_solving import table_positions
    t = np.zeros(3, [('x', '<f8'), ('y', '<f8'), ('flux', '<f8')])
    t['x'], t['y'], t['flux'] = [1, 2, 3], [4, 5, 6], [10.0, 30.0, 20.0]
    assert table_positions(t).tolist() == [[2, 5], [3, 6], [1, 4]]
    assert table_positions(dict(sources_table=t)).tolist() == [[2, 5], [3, 6], [1, 4]]
    assert table_positions([[1.5, 2.5]]).tolist() == [[1.5, 2.5]]


def test_refusals_need_no_device():
    from lightcurver_amd import _lib, astroalign
    l = _lib.lib()
    assert [p for p in range(0, 140) if l.lc_register_supported(p)] == list(range(3, 129))
    assert l.lc_register_supported(-1) == 0
    assert astroalign.supported(50) and not astroalign.supported(129)
    with pytest.raises(NotImplementedError):
        astroalign.find_transforms_batch([np.zeros((4, 2))], [np.zeros((4, 2))], max_control_points=129)
    with pytest.raises(NotImplementedError):
        astroalign.find_transform(np.zeros((64, 64)), np.zeros((64, 64)))            # images
    assert (astroalign.MAX_CONTROL_POINTS, astroalign.PIXEL_TOL, astroalign.MIN_MATCHES_FRACTION,
            astroalign.NUM_NEAREST_NEIGHBORS) == (50, 2, 0.8, 5)
    assert issubclass(astroalign.MaxIterError, RuntimeError)
    # a null context is refused before anything else is looked at
    assert l.lc_register_sources(None, 1, 50, None, None, None, None, None, None, None, None, None, None, None) == -1
