"""GPU parity of the registration by star triangles (lc_register_sources, lightcurver_amd.astroalign, processes.
plate_solving; DESIGN.md section 5 "Frame registration") with the NumPy restatement of its SPEC (tests/_register.py).

Every decision is the restatement's: diag (triangles of both lists, matches, the winning hypothesis, the final inliers),
status, npairs and pairs are EQUAL.  The transform differs by the order of the sums of the fits alone: sums of at most ~10^3
float64 terms differ by about 1e-13 relative with the order, which moves a matrix entry by ~1e-13 and a translation (the
entry times coordinates below 1e4, and means of such coordinates) by up to a few 1e-9 px; the bounds are 1e-11 and 1e-7 px,
a factor of 30 over that and an order of magnitude under the 1e-6 margins (tests/test_register_cpu.py) that keep the
decisions from flipping.  A problem's outputs are bit-identical whatever shares its call."""
import ctypes as C

import numpy as np
import pytest

from . import _register as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
IN_ONE_CALL = [n for n in CASES if n != 'too_many']          # that one has a max_matches of its own
MATRIX_TOL, SHIFT_TOL = 1e-11, 1e-7

_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)


def call(ctx, problems, P, max_matches=R.MAX_MATCHES, pairs=True, diag=True, ms=True, pixel_tol=R.PIXEL_TOL, K=None,
         counts=None, missing=()):
    """lc_register_sources on [(S, T)]; returns the raw outputs (sentinels where the library wrote nothing) and rc."""
    from lightcurver_amd import _lib
    n = len(problems)
    src, tgt = np.zeros((n, P, 2)), np.zeros((n, P, 2))
    ns, nt = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k, (S, T) in enumerate(problems):
        ns[k], nt[k] = len(S), len(T)
        src[k, :len(S)], tgt[k, :len(T)] = S, T
    if counts is not None:
        ns[:], nt[:] = counts
    out = dict(transform=np.full((n, 6), -7.0), pairs=np.full((n, P, 2), -7, np.int32), npairs=np.full(n, -7, np.int32),
               diag=np.full((n, 5), -7, np.int32), status=np.full(n, -7, np.int32))
    cfg = _lib.RegisterCfg(int(max_matches), float(pixel_tol), R.INVARIANT_RADIUS, R.MIN_MATCHES_FRACTION)
    t = C.c_float(-7.0)
    args = dict(src=src.ctypes.data_as(_f64p), nsrc=ns.ctypes.data_as(_i32p), tgt=tgt.ctypes.data_as(_f64p),
                ntgt=nt.ctypes.data_as(_i32p), cfg=C.byref(cfg), transform=out['transform'].ctypes.data_as(_f64p),
                pairs=out['pairs'].ctypes.data_as(_i32p) if pairs else None, npairs=out['npairs'].ctypes.data_as(_i32p),
                diag=out['diag'].ctypes.data_as(_i32p) if diag else None, status=out['status'].ctypes.data_as(_i32p),
                kernel_ms=C.byref(t) if ms else None)
    for name in missing:
        args[name] = None
    out['rc'] = _lib.lib().lc_register_sources(ctx.h, n if K is None else K, P, *args.values())
    out['kernel_ms'] = t.value
    return out


def one(out, k):
    """Problem k of a call: everything that must not depend on its neighbours, as bytes."""
    return (out['transform'][k].tobytes(), out['pairs'][k].tobytes(), int(out['npairs'][k]), out['diag'][k].tobytes(),
            int(out['status'][k]))


@pytest.fixture(scope='module')
def batch(ctx):
    out = call(ctx, [CASES[n][:2] for n in IN_ONE_CALL], 128)
    assert out['rc'] == 0 and out['kernel_ms'] > 0
    return out


def check(out, k, name):
    want = R.solved(name)
    got_t = out['transform'][k]
    print(name, 'diag', out['diag'][k].tolist(), 'want', want['diag'].tolist(), 'status', out['status'][k], 'npairs',
          out['npairs'][k], 'transform difference', np.abs(got_t - want['transform']).tolist())
    assert out['status'][k] == want['status']
    assert out['diag'][k].tolist() == want['diag'].tolist()
    npairs = int(out['npairs'][k])
    assert npairs == len(want['pairs'])
    assert out['pairs'][k, :npairs].tolist() == want['pairs'].tolist()
    assert (out['pairs'][k, npairs:] == -1).all()
    if want['status'] == 0:
        assert np.abs(got_t - want['transform'])[[0, 1, 3, 4]].max() <= MATRIX_TOL
        assert np.abs(got_t - want['transform'])[[2, 5]].max() <= SHIFT_TOL
        assert got_t[0] == got_t[4] and got_t[1] == -got_t[3]
    else:
        assert np.isnan(got_t).all()
    expected = CASES[name][4]
    assert expected is None or out['status'][k] == expected


@pytest.mark.parametrize('name', IN_ONE_CALL)
def test_cases_are_the_restatements(batch, name):
    check(batch, IN_ONE_CALL.index(name), name)


def test_too_many_matches_is_status_two(ctx):
    S, T, mm = CASES['too_many'][:3]
    out = call(ctx, [(S, T), CASES['n12_rot40'][:2]], 50, max_matches=mm)
    assert out['rc'] == 0
    check(out, 0, 'too_many')
    # its neighbour, 129 matches against a max_matches of 64, goes the same way and neither disturbs the other
    w = R.register(*CASES['n12_rot40'][:2], max_matches=mm)
    assert w['status'] == 2 and out['status'][1] == 2 and out['diag'][1].tolist() == w['diag'].tolist()


def test_a_problem_does_not_depend_on_its_call(ctx, batch):
    """All cases in one call, the same in reverse order, one call per case at P = 128 and at the smallest P that holds
    the case: bit-identical per problem."""
    problems = [CASES[n][:2] for n in IN_ONE_CALL]
    K = len(problems)
    rev = call(ctx, problems[::-1], 128)
    assert rev['rc'] == 0
    for k, name in enumerate(IN_ONE_CALL):
        assert one(rev, K - 1 - k) == one(batch, k), name
        alone = call(ctx, [problems[k]], 128)
        assert alone['rc'] == 0 and one(alone, 0) == one(batch, k), name
        P = max(3, len(problems[k][0]), len(problems[k][1]))
        small = call(ctx, [problems[k]], P)
        assert small['rc'] == 0
        npairs = int(small['npairs'][0])
        assert (small['transform'][0].tobytes(), small['pairs'][0, :npairs].tobytes(), npairs, small['diag'][0].tobytes(),
                int(small['status'][0])) == (batch['transform'][k].tobytes(), batch['pairs'][k, :npairs].tobytes(),
                                             int(batch['npairs'][k]), batch['diag'][k].tobytes(), int(batch['status'][k])), name


def test_optional_outputs(ctx, batch):
    names = ['n12_rot40', 'unrelated', 'n6_rot10']
    problems = [CASES[n][:2] for n in names]
    bare = call(ctx, problems, 128, pairs=False, diag=False, ms=False)
    assert bare['rc'] == 0 and bare['kernel_ms'] == -7.0
    assert (bare['pairs'] == -7).all() and (bare['diag'] == -7).all()
    for k, n in enumerate(names):
        j = IN_ONE_CALL.index(n)
        assert bare['transform'][k].tobytes() == batch['transform'][j].tobytes()
        assert bare['npairs'][k] == batch['npairs'][j] and bare['status'][k] == batch['status'][j]


def test_malformed_arguments_are_refused_before_any_launch(ctx):
    from lightcurver_amd import _lib
    good = [CASES['n6_rot10'][:2], CASES['n12_rot40'][:2]]

    def refused(code, **kw):
        problems = kw.pop('problems', good)
        out = call(ctx, problems, kw.pop('P', 50), **kw)
        assert out['rc'] == code, kw
        assert (out['transform'] == -7.0).all() and (out['status'] == -7).all() and (out['npairs'] == -7).all()
        assert (out['pairs'] == -7).all() and (out['diag'] == -7).all() and out['kernel_ms'] == -7.0
        assert _lib.lib().lc_last_error(ctx.h)

    refused(-1, K=0)
    refused(-1, K=-3)
    refused(-1, counts=(np.array([6, 51], np.int32), np.array([6, 12], np.int32)))
    refused(-1, counts=(np.array([6, 12], np.int32), np.array([-1, 12], np.int32)))
    for bad in (np.nan, np.inf):
        S = good[1][0].copy()
        S[11, 1] = bad
        refused(-1, problems=[good[0], (S, good[1][1])])
        T = good[0][1].copy()
        T[0, 0] = bad
        refused(-1, problems=[(good[0][0], T), good[1]])
    for name in ('src', 'nsrc', 'tgt', 'ntgt', 'cfg', 'transform', 'npairs', 'status'):
        refused(-1, missing=(name,))
    refused(-1, pixel_tol=0.0)
    refused(-1, pixel_tol=-2.0)
    refused(-1, pixel_tol=np.nan)
    refused(-1, max_matches=0)
    refused(-3, P=129, problems=[CASES['n3'][:2]])
    refused(-3, P=2, problems=[(np.zeros((2, 2)), np.zeros((2, 2)))])
    # a non-finite coordinate PAST a count is not looked at
    pad = call(ctx, good, 50)
    S = np.vstack([good[0][0], [[np.nan, np.inf]]])
    out = call(ctx, [(S, good[0][1]), good[1]], 50, counts=(np.array([6, 12], np.int32), np.array([6, 12], np.int32)))
    assert out['rc'] == 0 and one(out, 0) == one(pad, 0) and one(out, 1) == one(pad, 1)


def test_facade_has_astroaligns_shapes_and_exceptions(ctx):
    from lightcurver_amd import astroalign
    S, T = CASES['n12_rot40'][:2]
    want = R.solved('n12_rot40')
    # two rows that are not finite are dropped before the control points are taken; the pairs keep the caller's numbering
    S2 = np.vstack([[[np.nan, 1.0]], S[:5], [[2.0, np.inf]], S[5:]])
    tr, (sp, tp) = astroalign.find_transform(S2, T, ctx=ctx)
    assert isinstance(tr, astroalign.SimilarityTransform) and tr.params.shape == (3, 3)
    assert sp.shape == tp.shape == (len(want['pairs']), 2)
    assert np.array_equal(sp, S[want['pairs'][:, 0]]) and np.array_equal(tp, T[want['pairs'][:, 1]])
    assert np.abs(tr.params[:2].ravel() - want['transform'])[[0, 1, 3, 4]].max() <= MATRIX_TOL
    assert np.abs(tr.params[:2].ravel() - want['transform'])[[2, 5]].max() <= SHIFT_TOL
    assert np.sqrt(((tr(sp) - tp) ** 2).sum(axis=1)).max() < astroalign.PIXEL_TOL
    # lists of tuples, as the reference passes them
    tr2, _ = astroalign.find_transform([tuple(p) for p in S], [tuple(p) for p in T], ctx=ctx)
    assert np.array_equal(tr2.params, tr.params)
    with pytest.raises(astroalign.MaxIterError):
        astroalign.find_transform(*CASES['unrelated'][:2], ctx=ctx)
    with pytest.raises(ValueError, match='source'):
        astroalign.find_transform(S[:2], T, ctx=ctx)
    with pytest.raises(ValueError, match='target'):
        astroalign.find_transform(S, T[:2], ctx=ctx)
    # max_control_points cuts both lists: the 128-point list against 50 is then 50 against 50
    big, small = CASES['n128_vs_50'][:2]
    r = astroalign.find_transforms_batch([big, big], small, max_control_points=50, ctx=ctx)
    w = R.solved('n128_cut_to_50')
    assert r['status'].tolist() == [w['status']] * 2 and r['diag'][0].tolist() == r['diag'][1].tolist() == w['diag'].tolist()
    assert r['pairs'][0].tolist() == w['pairs'].tolist()
    # a batch never raises for a frame that fails
    r = astroalign.find_transforms_batch(S, [T, CASES['unrelated'][1], T[:2]], ctx=ctx)
    assert r['status'].tolist() == [0, 1, 3] and r['transforms'][1] is None and r['transforms'][2] is None
    assert np.array_equal(r['transforms'][0].params, tr.params) and len(r['pairs'][1]) == 0


def test_frames_to_stamps_without_a_wcs(ctx):
    """Rendered frames -> FrameSet.import_frames -> register_frames -> positions_in_frames -> cut_stamps at 32 px."""
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.plate_solving import positions_in_frames, register_frames, table_positions
    r = R.rendered()
    bound = 3 * R.worst_centroid_error()        # of the restated extraction, not of the code under test
    n = 32
    with FrameSet(r['stack'], ctx) as fs:
        imp = fs.import_frames(R.EXPTIME)
        assert (imp['ex_status'] == 0).all()
        results = register_frames(imp['objects'], reference=0, ctx=ctx)
        assert [q['success'] for q in results] == [True, True, True, False]
        tables = [table_positions(o) for o in imp['objects']]
        for k, q in enumerate(results):
            finite = tables[k][np.isfinite(tables[k]).all(axis=1)]
            ref = tables[0][np.isfinite(tables[0]).all(axis=1)]
            w = R.register(ref[:50], finite[:50])
            print(k, q['status'], q['diag'].tolist(), w['margins'])
            assert w['margins']['radius'] >= 1e-6 and w['margins']['error'] >= 1e-6 and w['margins']['d2'] >= 1e-9
            assert q['status'] == w['status'] and q['diag'].tolist() == w['diag'].tolist()
            assert q['n_matched'] == len(w['pairs'])
            if q['success']:
                got = q['transform'].params[:2].ravel()
                assert np.abs(got - w['transform'])[[0, 1, 3, 4]].max() <= MATRIX_TOL
                assert np.abs(got - w['transform'])[[2, 5]].max() <= SHIFT_TOL
        pos = positions_in_frames(results, r['field'])
        assert np.isnan(pos[3]).all()
        for k in range(3):
            a, b, tx, ty = r['truth'][k]
            true = np.stack([a * r['field'][:, 0] - b * r['field'][:, 1] + tx, b * r['field'][:, 0] + a * r['field'][:, 1] + ty], 1)
            err = np.sqrt(((pos[k] - true) ** 2).sum(axis=1)).max()
            print('frame', k, 'worst position error %.4f px, bound %.4f px' % (err, bound))
            assert err <= bound
            # frame 2 lost a quarter of its stars: cut where a star is
            here = np.array([np.sqrt(((r['centres'][k] - p) ** 2).sum(axis=1)).min() < 1.0 for p in true])
            assert here.sum() == len(r['centres'][k])
            cut = fs.cut_stamps(k, pos[k][here], n)
            centre = cut['origin'] + (n - 1) / 2.0
            # the cut rounds the position to a whole pixel (x0 = ceil(x - n / 2)): half a pixel on top of the bound
            assert np.abs(true[here] - centre).max() <= 0.5 + bound
            # and the brightest pixel of the middle of the stamp is the one that holds the star's centre
            peak = np.array([np.unravel_index(np.argmax(s[10:22, 10:22]), (12, 12)) for s in cut['data']])[:, ::-1] + 10
            assert np.abs(peak - (n - 1) / 2.0).max() <= 0.5 + bound + 0.5
