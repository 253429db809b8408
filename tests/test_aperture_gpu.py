"""GPU checks of the exact circular-aperture sums (lc_aperture_sums, lc_frames_aperture_sums, lightcurver_amd.photutils,
FrameSet.aperture_photometry, initial_point_source_fluxes(method='exact'); DESIGN.md section 5 "Aperture sums").

The device's sum against the float64 restatement (tests/_aperture.py) on the same float32 inputs must lie within
16 x 2^-53 max(1, pi r^2) sum |data| over the clipped bounding box (_aperture.bound: 2 measured for the closed form
against 50-digit arithmetic, a margin of 4 for the device's atan2 and sqrt, and float64 summation well inside); the same
for sum_err^2 with error^2, plus 4 x 2^-53 sum_err^2 for the square root, and for area and bad_area with |data| = 1.
Every test prints its worst ratio to the bound before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest

from . import _aperture as A

pytestmark = pytest.mark.gpu

CORNER = math.pi / 12 - (math.sqrt(3) - 1) / 4
EDGE = (math.pi - 1 - 4 * CORNER) / 4
SENTINEL = -777.25
OUTPUTS = ('sum', 'sum_err', 'area', 'bad_area')
_dp, _ip, _fp, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _raw(ctx, data, image, xy, r, error=None, mask=None, want=None, K=None, h=None, w=None, P=None, drop=()):
    """lc_aperture_sums through ctypes: (rc, outputs filled with SENTINEL beforehand).  ``want``: the outputs asked for
    (all, sum_err only with an error map); ``drop``: arguments passed as NULL; K, h, w, P: passed instead of the arrays' own."""
    from lightcurver_amd import _lib
    if want is None:
        want = OUTPUTS if error is not None else ('sum', 'area', 'bad_area')
    d = np.ascontiguousarray(data, np.float32)
    image = np.ascontiguousarray(image, np.int32)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    r = np.ascontiguousarray(r, np.float64)
    e = None if error is None else np.ascontiguousarray(error, np.float32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    out = {k: (np.full(len(xy), SENTINEL) if k in want else None) for k in OUTPUTS}
    args = dict(data=_p(d, _fp), image=_p(image, _ip), xy=_p(xy, _dp), r=_p(r, _dp))
    for name in drop:
        args[name] = None
    ms = C.c_float()
    rc = _lib.lib().lc_aperture_sums(
        ctx.h, d.shape[0] if K is None else K, d.shape[1] if h is None else h, d.shape[2] if w is None else w, args['data'],
        _p(e, _fp), _p(m, _u8p), len(xy) if P is None else P, args['image'], args['xy'], args['r'], _p(out['sum'], _dp),
        _p(out['sum_err'], _dp), _p(out['area'], _dp), _p(out['bad_area'], _dp), C.byref(ms))
    return rc, out


def _reference(data, image, xy, r, error=None, mask=None):
    """The restatement per aperture, and the bounds: dict of arrays sum, sum_err, area, bad_area, b_sum, b_err2, b_area."""
    ref = {k: np.zeros(len(xy)) for k in OUTPUTS + ('b_sum', 'b_err2', 'b_area')}
    for p, (k, (x, y), rr) in enumerate(zip(image, xy, r)):
        s, se, a, b = A.aperture_sums(data[k], x, y, rr, None if error is None else error[k], None if mask is None else mask[k])
        ref['sum'][p], ref['sum_err'][p], ref['area'][p], ref['bad_area'][p] = s, 0.0 if se is None else se, a, b
        ref['b_sum'][p] = A.bound(data[k], x, y, rr)
        ref['b_area'][p] = A.bound(np.ones(data[k].shape), x, y, rr)
        if error is not None:
            ref['b_err2'][p] = A.bound(error[k].astype(np.float64) ** 2, x, y, rr)
    return ref


def _ratio(diff, bound):
    """max |diff| / bound, a zero bound demanding a zero difference."""
    diff, bound = np.abs(np.atleast_1d(diff)), np.atleast_1d(bound)
    return float(np.max(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))))


def _check(label, got, ref, with_error):
    ratios = dict(sum=_ratio(got['sum'] - ref['sum'], ref['b_sum']), area=_ratio(got['area'] - ref['area'], ref['b_area']),
                  bad_area=_ratio(got['bad_area'] - ref['bad_area'], ref['b_area']))
    if with_error:
        ratios['sum_err^2'] = _ratio(got['sum_err'] ** 2 - ref['sum_err'] ** 2, ref['b_err2'] + 4 * A.EPS * ref['sum_err'] ** 2)
    print(label, 'worst ratios to the bound:', {k: round(v, 4) for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v <= 1.0, (label, k, v)


# ---- case 2: the batch every later case compares with -----------------------------------------------------------------
K2, H2, W2, P2 = 3, 24, 32, 130


def _batch_inputs():
    rng = np.random.default_rng(2024)
    data = rng.normal(50.0, 20.0, (K2, H2, W2)).astype(np.float32)
    error = rng.uniform(0.5, 3.0, (K2, H2, W2)).astype(np.float32)
    data[rng.random(data.shape) < 0.02] = np.nan
    error[0, 3, 4] = np.inf                                       # a bad error under good data
    mask = (rng.random(data.shape) < 0.02).astype(np.uint8)
    r = np.exp(rng.uniform(np.log(0.2), np.log(20.0), P2))
    xy = np.stack([rng.uniform(-3.0, W2 + 3.0, P2), rng.uniform(-3.0, H2 + 3.0, P2)], axis=1)
    image = rng.integers(0, K2, P2).astype(np.int32)
    xy[:3], r[:3] = [[-2.9, 10.0], [W2 + 2.5, H2 + 2.5], [15.0, -2.8]], [0.9, 1.1, 0.4]     # wholly outside, by construction
    return data, error, mask, image, xy, r


@pytest.fixture(scope='module')
def batch(ctx):
    data, error, mask, image, xy, r = _batch_inputs()
    ref = _reference(data, image, xy, r, error, mask)
    for v in ref.values():
        v.setflags(write=False)
    rc, got = _raw(ctx, data, image, xy, r, error, mask)
    assert rc == 0
    return dict(data=data, error=error, mask=mask, image=image, xy=xy, r=r, ref=ref, got=got)


def test_unit_circle_known_answers(ctx):
    """r = 1 on a pixel centre: centre 1, edge neighbours (pi - 1 - 4 c) / 4, diagonal neighbours c = pi / 12 - (sqrt 3 - 1) / 4,
    total pi: on a 5 x 5 image of ones, and on the nine delta images."""
    ones = np.ones((1, 5, 5), np.float32)
    rc, got = _raw(ctx, ones, [0], [[2.0, 2.0]], [1.0], error=ones)
    assert rc == 0
    b = A.bound(ones[0], 2.0, 2.0, 1.0)
    print('ones: sum - pi', got['sum'][0] - math.pi, 'bound', b)
    assert abs(got['sum'][0] - math.pi) <= b and abs(got['area'][0] - math.pi) <= b and got['bad_area'][0] == 0.0
    assert abs(got['sum_err'][0] ** 2 - math.pi) <= b + 4 * A.EPS * math.pi
    deltas = np.zeros((9, 5, 5), np.float32)
    want = []
    for q in range(9):
        di, dj = q // 3 - 1, q % 3 - 1
        deltas[q, 2 + di, 2 + dj] = 1.0
        want.append([1.0, EDGE, CORNER][abs(di) + abs(dj)])
    rc, got = _raw(ctx, deltas, np.arange(9), np.tile([2.0, 2.0], (9, 1)), np.ones(9), want=('sum',))
    assert rc == 0
    worst = _ratio(got['sum'] - np.array(want), np.full(9, 16 * A.EPS * math.pi))       # sum |data| = 1
    print('deltas: worst ratio to the bound', worst, got['sum'] - np.array(want))
    assert worst <= 1.0 and got['sum'][4] == 1.0


def test_batch_of_130_apertures_on_three_images(batch):
    """K = 3 images of 24 x 32, 130 apertures (33 workgroups, the last with two waves), r log-uniform in [0.2, 20], centres up
    to 3 px outside, 2 % NaN, 2 % masked, an error map: all four outputs."""
    ref, got = batch['ref'], batch['got']
    outside = (ref['area'] == 0) & (ref['bad_area'] == 0)
    inside = (batch['xy'][:, 0] - batch['r'] > -0.5) & (batch['xy'][:, 0] + batch['r'] < W2 - 0.5) & \
             (batch['xy'][:, 1] - batch['r'] > -0.5) & (batch['xy'][:, 1] + batch['r'] < H2 - 0.5)
    print('outside', outside.sum(), 'inside', inside.sum(), 'with bad area', (ref['bad_area'] > 0).sum())
    assert outside[:3].all() and inside.sum() >= 10 and (~inside & ~outside).sum() >= 10 and (ref['bad_area'] > 0).sum() >= 10
    for k in OUTPUTS:
        assert (got[k][:3] == 0.0).all(), k                      # a circle wholly outside the image: four zeros
        assert np.isfinite(got[k]).all(), k
    _check('batch', got, ref, True)


def test_circle_inside_one_pixel(ctx):
    """r = 0.3 on the corner (7.5, 7.5) of four pixels of one value, and at (7.2, 6.9) inside pixel (7, 7): pi r^2 d, pi r^2."""
    rng = np.random.default_rng(5)
    img = rng.normal(10.0, 3.0, (1, 16, 16)).astype(np.float32)
    d = np.float32(3.25)
    img[0, 7:9, 7:9] = d
    xy, r = np.array([[7.5, 7.5], [7.2, 6.9]]), np.array([0.3, 0.3])
    rc, got = _raw(ctx, img, [0, 0], xy, r)
    assert rc == 0
    area = math.pi * 0.3 ** 2
    for p in range(2):
        b, ba = A.bound(img[0], *xy[p], r[p]), A.bound(np.ones((16, 16)), *xy[p], r[p])
        print('r = 0.3 at', xy[p], 'sum ratio', abs(got['sum'][p] - area * float(d)) / b, 'area ratio', abs(got['area'][p] - area) / ba)
        assert abs(got['sum'][p] - area * float(d)) <= b + 2 * A.EPS * area * float(d)      # (pi r^2 d itself is rounded)
        assert abs(got['area'][p] - area) <= ba + 2 * A.EPS * area
    _check('inside one pixel', got, _reference(img, [0, 0], xy, r), False)


def test_circle_tangent_to_pixel_edges(ctx):
    """Centre (8, 8) with r = 2.5 and 2.5 +- 1e-7 (the circle touches four pixel edges), and centre (8.3, 7.6) with the
    right extreme 1e-9 inside the edge at 10.5."""
    rng = np.random.default_rng(6)
    img = rng.normal(10.0, 3.0, (1, 16, 16)).astype(np.float32)
    xy = np.array([[8.0, 8.0]] * 3 + [[8.3, 7.6]])
    r = np.array([2.5, 2.5 - 1e-7, 2.5 + 1e-7, 10.5 - 1e-9 - 8.3])
    assert 0 < 10.5 - (8.3 + r[3]) < 2e-9
    rc, got = _raw(ctx, img, [0] * 4, xy, r, error=np.abs(img))
    assert rc == 0
    _check('tangent', got, _reference(img, [0] * 4, xy, r, np.abs(img)), True)
    ba = A.bound(np.ones((16, 16)), 8.0, 8.0, 2.5)
    assert abs(got['area'][0] - math.pi * 6.25) <= ba + 2 * A.EPS * math.pi * 6.25
    assert got['area'][1] < got['area'][0] < got['area'][2]


def test_circle_larger_than_the_image(ctx):
    """r = 64 at the centre of a 16 x 16 image: every pixel whole."""
    rng = np.random.default_rng(7)
    img = rng.normal(10.0, 3.0, (1, 16, 16)).astype(np.float32)
    rc, got = _raw(ctx, img, [0], [[7.5, 7.5]], [64.0])
    assert rc == 0
    total = float(np.sum(img.astype(np.float64)))
    b = A.bound(img[0], 7.5, 7.5, 64.0)
    print('r = 64: sum - total', got['sum'][0] - total, 'bound', b, 'area', got['area'][0])
    assert abs(got['sum'][0] - total) <= b and got['area'][0] == 256.0 and got['bad_area'][0] == 0.0
    _check('larger than the image', got, _reference(img, [0], np.array([[7.5, 7.5]]), np.array([64.0])), False)


def test_results_do_not_depend_on_the_list(ctx, batch):
    """The list reversed, and five apertures each alone (one of them on a stack that holds only its image): the bits of the
    batch."""
    data, error, mask, image, xy, r, got = (batch[k] for k in ('data', 'error', 'mask', 'image', 'xy', 'r', 'got'))
    rc, rev = _raw(ctx, data, image[::-1], xy[::-1], r[::-1], error, mask)
    assert rc == 0
    for k in OUTPUTS:
        assert rev[k][::-1].tobytes() == got[k].tobytes(), k
    for p in (0, 7, 64, 128, 129):
        rc, one = _raw(ctx, data, image[p:p + 1], xy[p:p + 1], r[p:p + 1], error, mask)
        assert rc == 0
        for k in OUTPUTS:
            assert one[k].tobytes() == got[k][p:p + 1].tobytes(), (p, k)
    p, k = 129, int(image[129])
    rc, one = _raw(ctx, data[k:k + 1], [0], xy[p:p + 1], r[p:p + 1], error[k:k + 1], mask[k:k + 1])
    assert rc == 0 and all(one[key].tobytes() == got[key][p:p + 1].tobytes() for key in OUTPUTS)


def test_only_the_sum_requested(ctx, batch):
    data, error, mask, image, xy, r, got = (batch[k] for k in ('data', 'error', 'mask', 'image', 'xy', 'r', 'got'))
    rc, only = _raw(ctx, data, image, xy, r, error, mask, want=('sum',))
    assert rc == 0 and only['sum'].tobytes() == got['sum'].tobytes()
    rc, plain = _raw(ctx, data, image, xy, r, want=('sum',))                 # no error map, no mask
    assert rc == 0
    ref = _reference(data, image, xy, r)
    worst = _ratio(plain['sum'] - ref['sum'], ref['b_sum'])
    print('sum alone, no error, no mask: worst ratio', worst)
    assert worst <= 1.0


def test_refusals_leave_the_outputs_untouched(ctx):
    from lightcurver_amd import _lib
    INVALID, UNSUPPORTED = -1, -3
    img = np.ones((2, 8, 9), np.float32)
    xy, r, image = np.array([[3.0, 4.0], [5.0, 2.0]]), np.array([2.0, 1.5]), np.array([0, 1], np.int32)

    def refused(code, what, **kw):
        args = dict(data=img, image=image, xy=xy, r=r)
        args.update({k: kw.pop(k) for k in list(kw) if k in args})
        rc, out = _raw(ctx, args['data'], args['image'], args['xy'], args['r'], **kw)
        assert rc == code, (what, rc)
        assert all(v is None or (v == SENTINEL).all() for v in out.values()), what

    for name in ('K', 'h', 'w', 'P'):
        refused(INVALID, name + ' = 0', **{name: 0})
        refused(INVALID, name + ' < 0', **{name: -1})
    for name in ('data', 'image', 'xy', 'r'):
        refused(INVALID, 'no ' + name, drop=(name,))
    refused(INVALID, 'no sum', want=('area',))
    refused(INVALID, 'sum_err without an error map', want=OUTPUTS)
    refused(INVALID, 'image index -1', image=np.array([0, -1], np.int32), want=('sum',))
    refused(INVALID, 'image index K', image=np.array([2, 0], np.int32), want=('sum',))
    for bad in (np.nan, np.inf, -np.inf):
        refused(INVALID, f'x = {bad}', xy=np.array([[3.0, 4.0], [bad, 2.0]]), want=('sum',))
        refused(INVALID, f'y = {bad}', xy=np.array([[3.0, bad], [5.0, 2.0]]), want=('sum',))
    for bad in (np.nan, np.inf, 0.0, -1.0):
        refused(INVALID, f'r = {bad}', r=np.array([2.0, bad]), want=('sum',))
    refused(UNSUPPORTED, 'K h w = 2^31', K=2 ** 11, h=2 ** 10, w=2 ** 10, want=('sum',))
    rc, out = _raw(ctx, img, image, xy, r, error=img)                       # and the call the refusals vary is sound
    assert rc == 0 and not any((v == SENTINEL).any() for v in out.values())

    # lc_frames_aperture_sums
    from lightcurver_amd.frames import FrameSet
    lib = _lib.lib()
    t, rms = np.array([10.0, 20.0], np.float32), np.array([1.0, 2.0], np.float32)

    def frames_call(fs, code, what, P=2, frame=image, xy=xy, r=r, t=t, rms=rms, with_error=1, want=OUTPUTS, null_set=False):
        out = {k: (np.full(2, SENTINEL) if k in want else None) for k in OUTPUTS}
        rc = lib.lc_frames_aperture_sums(None if null_set else fs.h, P, _p(frame, _ip), _p(xy, _dp), _p(r, _dp), _p(t, _fp),
                                         _p(rms, _fp), with_error, _p(out['sum'], _dp), _p(out['sum_err'], _dp),
                                         _p(out['area'], _dp), _p(out['bad_area'], _dp), None)
        assert rc == code, (what, rc)
        if code:
            assert all(v is None or (v == SENTINEL).all() for v in out.values()), what
        return out

    with FrameSet(img, ctx) as fs:
        frames_call(fs, INVALID, 'no frame set', null_set=True)
        frames_call(fs, INVALID, 'P = 0', P=0)
        frames_call(fs, INVALID, 'P < 0', P=-1)
        for name in ('frame', 'xy', 'r'):
            frames_call(fs, INVALID, 'no ' + name, **{name: None})
        frames_call(fs, INVALID, 'no sum', want=('area',))
        frames_call(fs, INVALID, 'sum_err without with_error', with_error=0)
        frames_call(fs, INVALID, 'frame index -1', frame=np.array([0, -1], np.int32))
        frames_call(fs, INVALID, 'frame index K', frame=np.array([2, 0], np.int32))
        for bad in (np.nan, np.inf):
            frames_call(fs, INVALID, f'x = {bad}', xy=np.array([[bad, 4.0], [5.0, 2.0]]))
            frames_call(fs, INVALID, f'r = {bad}', r=np.array([2.0, bad]))
        for bad in (0.0, -2.0):
            frames_call(fs, INVALID, f'r = {bad}', r=np.array([bad, 1.0]))
        frames_call(fs, INVALID, 'with_error on a raw set without exptime', t=None)
        frames_call(fs, INVALID, 'with_error on a raw set without rms', rms=None)
        for bad in (np.nan, np.inf, 0.0, -5.0):
            frames_call(fs, INVALID, f'exptime = {bad}', t=np.array([10.0, bad], np.float32))
            frames_call(fs, INVALID, f'exptime = {bad}, no error asked', t=np.array([bad, 10.0], np.float32), with_error=0,
                        want=('sum', 'area', 'bad_area'))
        out = frames_call(fs, 0, 'sound')
        assert not any((v == SENTINEL).any() for v in out.values())
        out = frames_call(fs, 0, 'sound without an error', t=None, rms=None, with_error=0, want=('sum',))
        assert not (out['sum'] == SENTINEL).any()


# ---- case 9: the resident frame set -----------------------------------------------------------------------------------
def _scene():
    rng = np.random.default_rng(31)
    h, w = 64, 96
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = rng.normal(20.0, 2.0, (2, h, w))
    stars = [(12.3, 14.8, 900.0), (25.1, 70.2, 1500.0), (50.7, 30.9, 700.0), (40.2, 85.5, 1200.0), (8.8, 50.1, 600.0)]
    for k in range(2):
        for cy, cx, a in stars:
            frames[k] += a * np.exp(-((x - cx - 0.4 * k) ** 2 + (y - cy + 0.3 * k) ** 2) / (2 * 1.7 ** 2))
    frames = frames.astype(np.float32)
    frames[0, 13, 15] = np.nan                                    # under the first star
    xy = np.array([[cx, cy] for cy, cx, _ in stars] + [[2.2, 3.1], [94.6, 61.9], [47.5, 31.5]])
    return frames, xy


@pytest.mark.parametrize('imported', [False, True])
def test_frame_set(ctx, imported):
    """On a raw set and on an imported one: the sums have the bits of aperture_sums_batch on planes(); with the error, sum_err
    agrees with the one from the noise maps of the 32-pixel stamps cut around the apertures (the shifted centres round
    differently, so within the bound and not to the bit)."""
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.photutils import aperture_sums_batch
    frames, xy = _scene()
    S = len(xy)
    pos = np.concatenate([xy, xy + [0.4, -0.3]])
    index = np.repeat([0, 1], S).astype(np.int32)
    r = np.concatenate([np.linspace(2.0, 6.5, S), np.full(S, 3.0)])
    t, rms = np.array([30.0, 12.5], np.float32), np.array([2.0, 2.2], np.float32)
    with FrameSet(frames, ctx) as fs:
        if imported:
            imp = fs.import_frames(t)
            assert fs.imported and (imp['ex_status'] == 0).all()
            given = {}
        else:
            given = dict(exptimes=t, background_rms=rms)
        planes = fs.planes()
        got = fs.aperture_photometry(index, pos, r)
        want = aperture_sums_batch(planes, index, pos, r, ctx=ctx)
        assert got['sum_err'] is None
        for k in ('sum', 'area', 'bad_area'):
            assert got[k].tobytes() == want[k].tobytes(), k
        assert (got['bad_area'] > 0).any() == (not imported or bool(np.isnan(planes).any()))
        err = fs.aperture_photometry(index, pos, r, with_error=True, **given)
        for k in ('sum', 'area', 'bad_area'):
            assert err[k].tobytes() == got[k].tobytes(), k
        st = fs.cut_stamps(index, pos, 32, **given)
    shifted = pos - st['origin']
    ref = aperture_sums_batch(st['data'], np.arange(2 * S), shifted, r, error=st['noisemap'], ctx=ctx)
    b2 = np.array([A.bound(st['noisemap'][s].astype(np.float64) ** 2, shifted[s, 0], shifted[s, 1], r[s]) for s in range(2 * S)])
    worst = _ratio(err['sum_err'] ** 2 - ref['sum_err'] ** 2, b2 + 4 * A.EPS * ref['sum_err'] ** 2)
    print('imported' if imported else 'raw', 'sum_err^2 against the stamps: worst ratio to the bound', worst)
    assert (err['sum_err'] > 0).all() and worst <= 1.0
    # and against the restatement on the stamps themselves
    _check('stamps', ref, _reference(st['data'], np.arange(2 * S), shifted, r, st['noisemap']), True)


def test_photutils_facade(ctx):
    """The reference's call shape on a 2-D stack; NaN where an unmasked NaN pixel has overlap and for an aperture outside
    the image, finite once the pixel is masked."""
    from lightcurver_amd.photutils import CircularAperture, aperture_photometry
    rng = np.random.default_rng(8)
    cube = rng.normal(5.0, 1.0, (5, 20, 20)).astype(np.float32)
    stack = np.nanmedian(cube, axis=0)
    positions = [(9.3, 10.2), (4.1, 15.7), (40.0, 3.0), (0.2, 0.4)]
    table = aperture_photometry(stack, CircularAperture(positions, 3.0))
    assert list(table['id']) == [1, 2, 3, 4] and 'aperture_sum_err' not in table
    assert np.array_equal(table['xcenter'], [p[0] for p in positions]) and np.array_equal(table['ycenter'], [p[1] for p in positions])
    xy, r = np.array(positions), np.full(4, 3.0)
    ref = _reference(stack[None], [0] * 4, xy, r)
    assert math.isnan(table['aperture_sum'][2])                                            # outside the image
    keep = [0, 1, 3]
    assert _ratio(table['aperture_sum'][keep] - ref['sum'][keep], ref['b_sum'][keep]) <= 1.0
    one = aperture_photometry(stack, CircularAperture(positions[0], 3.0))
    assert one['aperture_sum'].shape == (1,) and one['aperture_sum'][0] == table['aperture_sum'][0]
    bad = stack.copy()
    bad[10, 9] = np.nan
    err = np.full(stack.shape, 0.5, np.float32)
    table = aperture_photometry(bad, CircularAperture(positions, 3.0), error=err)
    assert np.isnan(table['aperture_sum'][[0, 2]]).all() and np.isfinite(table['aperture_sum'][[1, 3]]).all()
    assert np.isnan(table['aperture_sum_err'][[0, 2]]).all() and np.isfinite(table['aperture_sum_err'][[1, 3]]).all()
    mask = np.isnan(bad)
    table = aperture_photometry(bad, CircularAperture(positions, 3.0), error=err, mask=mask)
    refm = _reference(bad[None], [0] * 4, xy, r, err[None], mask[None])
    assert np.isfinite(table['aperture_sum'][keep]).all() and math.isnan(table['aperture_sum'][2])
    assert _ratio(table['aperture_sum'][keep] - refm['sum'][keep], refm['b_sum'][keep]) <= 1.0
    assert _ratio(table['aperture_sum_err'][keep] ** 2 - refm['sum_err'][keep] ** 2,
                  refm['b_err2'][keep] + 4 * A.EPS * refm['sum_err'][keep] ** 2) <= 1.0
    assert table['aperture_sum'][0] < ref['sum'][0]                                        # the masked pixel does not count


def test_exact_starting_fluxes_of_the_roi_fit(ctx):
    """initial_point_source_fluxes(method='exact') is the restatement applied to np.nanmedian of the float32 data (five
    epochs: the median is an order statistic), and model_roi_cutouts(aperture_method='exact') starts stage 1 from it."""
    from lightcurver_amd.processes.roi_modelling import initial_point_source_fluxes, model_roi_cutouts
    from lightcurver_amd.synthetic import make_roi_dataset
    E, M, n, ss = 5, 2, 16, 2
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=21)
    off = (n - 1) / 2.0
    xs, ys = ds['truth']['c_x'] + off + 0.2, ds['truth']['c_y'] + off - 0.1
    data = np.array(ds['data'], np.float32)
    data[1, 3, 3] = np.nan
    got = initial_point_source_fluxes(data, xs, ys, 3.0, method='exact', ctx=ctx)
    stack = np.nanmedian(data, axis=0)
    assert stack.dtype == np.float32 and len(got) == M
    ref = _reference(stack[None], [0] * M, np.stack([xs, ys], axis=1), np.full(M, 3.0))
    worst = _ratio(np.array(got) - ref['sum'], ref['b_sum'])
    centre = initial_point_source_fluxes(data, xs, ys, 3.0)
    print('exact', got, 'pixel-centre', centre, 'worst ratio to the bound', worst)
    assert worst <= 1.0 and not np.allclose(got, centre, rtol=1e-6)
    full, noise = ds['data'] * ds['scale'], ds['noisemap'] * ds['scale']
    out = model_roi_cutouts(full, noise, ds['psf'], ss, xs, ys, aperture_method='exact', roi_deconv_translations_iters=5,
                            roi_deconv_all_iters=5)
    want = initial_point_source_fluxes(np.array(full, np.float64) / out['scale'], xs, ys, 3.0, method='exact', ctx=ctx)
    assert out['initial_a'] == want and len(out['loss_history']) == 5
    assert out['initial_a'] != initial_point_source_fluxes(np.array(full, np.float64) / out['scale'], xs, ys, 3.0)
