"""GPU parity of the source extraction of whole frames (lc_extract_frames, lc_import_frames; DESIGN.md §5 "Source
extraction of frames") against the NumPy restatement of the SPEC (tests/_extract.py).

Bit for bit: segmap, mask, nobj, status, every integer field, peak, cpeak, x, y, a, b.  theta within 1e-12 (the device's
atan2 is not correctly rounded); flux within 1e-10 of the sum of |D| over the object (2^18 terms of 2^-53 each, the order
of the sum differs from the checker's).  Every table is the same in two runs."""
import ctypes as C

import numpy as np
import pytest

from tests import _background as B
from tests import _extract as E

pytestmark = pytest.mark.gpu

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope='module')
def ctx():
    from lightcurver_amd import _lib
    return _lib.Context(0)


def _raw(ctx, frames, var, thresh, minarea, filt, max_objects=4096, check=True, **override):
    """lc_extract_frames through ctypes with sentinels in every output; returns (rc, outputs)."""
    from lightcurver_amd import _lib
    d = _lib.f32(frames)
    K, h, w = d.shape
    v = _lib.f32(var)
    plane = v if v.ndim == 3 else None
    scalar = None if v.ndim == 3 else np.ascontiguousarray(np.broadcast_to(v.reshape(-1), (K,)), np.float32)
    out = dict(objects=np.full((K, max(max_objects, 1)), 0x55, np.uint8).repeat(96, axis=1).view(_lib.EXTRACT_OBJECT_DTYPE),
               nobj=np.full(K, -9, np.int32), segmap=np.full(d.shape, -9, np.int32), mask=np.full(d.shape, 9, np.uint8),
               status=np.full(K, -9, np.int32))
    cfg = _lib.ExtractCfg(thresh, minarea, filt)
    ms = C.c_float()
    a = dict(K=K, h=h, w=w, data=_lib.ptr(d), var=_lib.ptr(plane), scalar=_lib.ptr(scalar), cfg=C.byref(cfg),
             max_objects=max_objects, objects=out['objects'].ctypes.data_as(C.c_void_p), nobj=out['nobj'].ctypes.data_as(_i32p),
             segmap=out['segmap'].ctypes.data_as(_i32p), mask=out['mask'].ctypes.data_as(_u8p),
             status=out['status'].ctypes.data_as(_i32p))
    a.update(override)
    rc = _lib.lib().lc_extract_frames(ctx.h, a['K'], a['h'], a['w'], a['data'], a['var'], a['scalar'], a['cfg'],
                                      a['max_objects'], a['objects'], a['nobj'], a['segmap'], a['mask'], a['status'],
                                      C.byref(ms))
    if check:
        ctx.check(rc, 'lc_extract_frames')
    return rc, out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_frame(got, k, want, data, what=''):
    """Frame k of a device result against the restatement ``want`` of that frame."""
    assert got['status'][k] == want['status'], what
    assert got['nobj'][k] == want['nobj'], what
    assert np.array_equal(got['segmap'][k], want['segmap']), what
    assert np.array_equal(got['mask'][k], want['mask']), what
    n = len(want['objects'])
    t, r = got['objects'][k, :n], want['objects']
    for f in E.EXACT_FIELDS:
        assert _same_bits(t[f], r[f]), (what, f, t[f][:5], r[f][:5])
    both = np.isnan(t['theta']) & np.isnan(r['theta'])
    assert (both | (np.abs(t['theta'] - r['theta']) <= 1e-12)).all(), what
    absd = np.abs(np.where(np.isfinite(data), data, 0).astype(np.float64))
    for i in range(n):
        o = r[i]
        box = absd[o['ymin']:o['ymax'] + 1, o['xmin']:o['xmax'] + 1]
        inside = want['segmap'][o['ymin']:o['ymax'] + 1, o['xmin']:o['xmax'] + 1] == i + 1
        assert abs(t['flux'][i] - o['flux']) <= 1e-10 * box[inside].sum(), (what, i)
    rest = got['objects'][k, n:]
    assert not rest.view(np.uint8).any(), what          # rows past the objects are zero


def _check_call(ctx, frames, var, thresh, minarea, filt, max_objects=4096, what=''):
    rc, got = _raw(ctx, frames, var, thresh, minarea, filt, max_objects)
    rc, again = _raw(ctx, frames, var, thresh, minarea, filt, max_objects)
    assert _same_bits(got['objects'], again['objects']) and np.array_equal(got['segmap'], again['segmap'])
    wants = []
    v = np.asarray(var, np.float32)
    for k in range(len(frames)):
        vk = v[k] if v.ndim == 3 else np.broadcast_to(v.reshape(-1), (len(frames),))[k]
        want = E.extract(frames[k], vk, thresh, minarea, filt, max_objects)
        _check_frame(got, k, want, frames[k], f'{what} frame {k}')
        wants.append(want)
    return got, wants


# ---- exact patterns: filter 0 and the scalar variance 1 make the detection plane the pattern ---------------------------------

@pytest.mark.parametrize('shape', [(1, 1), (1, 70), (70, 1), (37, 53), (257, 129)])
def test_patterns(ctx, shape):
    """Every pattern as a frame of one call: nothing, everything, the checkerboard (one component), isolated pixels (the
    most components), the serpentine (the longest label path), staircases through tile corners, nested rings and the
    component that touches all four borders.  Then the isolated pixels with minarea 2: none is left."""
    h, w = shape
    frames = np.stack([E.pattern_frame(E.pattern(kind, h, w)) for kind in E.PATTERNS])
    got, wants = _check_call(ctx, frames, 1.0, 5.0, 1, 0, what=str(shape))
    by = dict(zip(E.PATTERNS, wants))
    assert by['nothing']['nobj'] == 0 and by['everything']['nobj'] == 1 and by['everything']['objects']['npix'][0] == h * w
    assert by['serpentine']['nobj'] == 1 and (by['checkerboard']['nobj'] == 1 or min(h, w) == 1)
    assert by['isolated']['nobj'] == ((h + 1) // 2) * ((w + 1) // 2)
    if min(h, w) > 30:
        assert by['rings']['nobj'] > 5 and by['four_borders']['nobj'] == 1
    got, wants = _check_call(ctx, frames, 1.0, 5.0, 2, 0, what=f'{shape} minarea 2')
    assert wants[E.PATTERNS.index('isolated')]['nobj'] == 0 and wants[E.PATTERNS.index('isolated')]['ncomp'] > 0


def test_patterns_differ_per_frame(ctx):
    frames = np.stack([E.pattern_frame(E.pattern(kind, 130, 197)) for kind in ('serpentine', 'staircases', 'rings')])
    got, wants = _check_call(ctx, frames, 1.0, 5.0, 1, 0)
    assert [x['nobj'] for x in wants][0] == 1 and wants[1]['nobj'] > 20 and wants[2]['nobj'] > 20


def test_minarea_at_below_and_above_a_size(ctx):
    frames = E.pattern_frame(E.pattern('rings', 37, 53))[None]
    sizes = sorted(set(E.extract(frames[0], 1.0, 5.0, 1, 0)['objects']['npix'].tolist()))
    s = sizes[len(sizes) // 2]
    counts = [_check_call(ctx, frames, 1.0, 5.0, m, 0)[1][0]['nobj'] for m in (s - 1, s, s + 1)]
    assert counts[0] == counts[1] > counts[2]


# ---- capacities, flags, refusals --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('transpose', [False, True])
def test_large_and_range_flags(ctx, transpose):
    d = np.zeros((8, 600), np.float32)
    d[2, 10:523] = 10.0          # 513 pixels: LARGE
    d[5, 10:522] = 10.0          # 512 pixels: not
    d[7, 3] = 1e9                # snr 1e9: RANGE
    d = d.T.copy() if transpose else d
    got, wants = _check_call(ctx, d[None], 1.0, 5.0, 1, 0)
    flags = sorted(wants[0]['objects']['flag'].tolist())
    assert flags == sorted([E.FLAG_LARGE, 0, E.FLAG_RANGE | E.FLAG_EDGE])


def test_invalid_pixels(ctx):
    """NaN, infinite and non-positive variances and NaN data make a pixel invalid: weight 0 in its neighbours' sums."""
    rng = np.random.default_rng(5)
    sub, var = E.scene(96, 150, 12, 21)
    sub, var = sub.copy(), var.copy()
    idx = rng.integers(0, sub.size, 400)
    var.ravel()[idx[:100]] = np.nan
    var.ravel()[idx[100:200]] = 0.0
    var.ravel()[idx[200:250]] = -1.0
    var.ravel()[idx[250:300]] = np.inf
    sub.ravel()[idx[300:350]] = np.nan
    sub.ravel()[idx[350:]] = np.inf
    for filt in (1, 0):
        got, wants = _check_call(ctx, sub[None], var[None], 3.0, 5, filt)
        assert wants[0]['nobj'] > 3
    bright = wants[0]['objects'][np.argmax(wants[0]['objects']['npix'])]
    sub[bright['ypeak'], bright['xpeak']] = np.nan          # an invalid pixel inside an object: detected through its neighbours
    got, wants = _check_call(ctx, sub[None], var[None], 3.0, 5, 1)
    assert wants[0]['det'][bright['ypeak'], bright['xpeak']]


def test_more_objects_than_the_table_holds(ctx):
    frames = np.stack([E.pattern_frame(E.pattern(kind, 37, 53)) for kind in ('rings', 'isolated', 'four_borders')])
    got, wants = _check_call(ctx, frames, 1.0, 5.0, 1, 0, max_objects=7)
    assert [x['status'] for x in wants] == [1, 1, 0] and wants[1]['nobj'] == 19 * 27
    assert got['segmap'][1].max() == 19 * 27 and len(wants[1]['objects']) == 7


def test_argument_refusals(ctx):
    from lightcurver_amd import _lib
    d = np.zeros((1, 8, 8), np.float32)
    bad = lambda **kw: _raw(ctx, d, 1.0, kw.pop('thresh', 3.0), kw.pop('minarea', 5), kw.pop('filt', 1), check=False, **kw)[0]
    assert bad() == 0
    assert bad(K=0) == -1 and bad(h=0) == -1 and bad(w=-1) == -1 and bad(max_objects=0) == -1
    assert bad(thresh=0.0) == -1 and bad(thresh=float('nan')) == -1 and bad(minarea=0) == -1 and bad(filt=2) == -1
    assert bad(data=None) == -1 and bad(scalar=None) == -1 and bad(nobj=None) == -1 and bad(status=None) == -1
    assert bad(cfg=None) == -1
    assert b'lc_extract_frames' in _lib.lib().lc_last_error(ctx.h)
    assert bad(objects=None) == 0 and bad(segmap=None, mask=None) == 0
    assert bad(h=65536, w=65536, data=_lib.ptr(d)) == -3          # refused before anything is read


# ---- scenes: filter 1 and a variance plane -----------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,K', [((200, 300), 4), ((512, 512), 2)])
def test_scenes(ctx, shape, K):
    h, w = shape
    pairs = [E.scene(h, w, 25 if h < 300 else 60, 30 + k) for k in range(K)]
    frames, var = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    got, wants = _check_call(ctx, frames, var, 3.0, 10, 1, what=str(shape))
    objs = np.concatenate([x['objects'] for x in wants])
    assert (objs['flag'] & E.FLAG_EDGE).any() and not (objs['flag'] & E.FLAG_EDGE).all()
    assert all(x['ncomp'] > x['nobj'] > 10 for x in wants)          # small components are dropped
    assert ((objs['xmin'] // 64 != objs['xmax'] // 64) & (objs['ymin'] // 16 != objs['ymax'] // 16)).any()


def test_one_large_frame(ctx):
    sub, var = E.fast_scene(2048, 2048, 400, 77)
    got, wants = _check_call(ctx, sub[None], var[None], 3.0, 10, 1)
    assert wants[0]['nobj'] > 350


def test_the_references_own_test_of_extract_stars(ctx):
    from lightcurver_amd.processes.star_extraction import extract_stars
    t = extract_stars(np.random.default_rng(0).random((100, 100)), 1.0, 3, 10, ctx=ctx)
    assert len(t) == 0
    for col in ('xcentroid', 'ycentroid', 'flag', 'a', 'b', 'flux', 'npix'):
        assert col in t.dtype.names


def test_extract_with_sep_signature(ctx):
    """err, var, no variance and mask of ``sep.extract``; status 1 makes it call once more with the true count."""
    from lightcurver_amd import sep
    sub, var = E.scene(96, 150, 12, 21)
    want = E.extract(sub, var, 3.0, 10, 1)
    got, seg = sep.extract(sub, 3.0, var=var, minarea=10, segmentation_map=True, ctx=ctx)
    assert got.dtype.names == sep.OBJECT_FIELDS and np.array_equal(seg, want['segmap'])
    for f in ('x', 'y', 'a', 'b', 'npix', 'peak', 'cpeak', 'xmin', 'xmax', 'ymin', 'ymax', 'xpeak', 'ypeak', 'flag'):
        assert _same_bits(got[f], want['objects'][f]), f
    err = np.sqrt(var)
    e = sep.extract(sub, 3.0, err=err, minarea=10, ctx=ctx)
    assert _same_bits(e['x'], E.extract(sub, err * err, 3.0, 10, 1)['objects']['x'])
    assert _same_bits(sep.extract(sub, 30.0, ctx=ctx)['x'], E.extract(sub, 1.0, 30.0, 5, 1)['objects']['x'])
    m = np.zeros(sub.shape, bool)
    m[:, 70:] = True
    masked = E.extract(sub, np.where(m, np.nan, var), 3.0, 10, 1)
    assert _same_bits(sep.extract(sub, 3.0, var=var, mask=m, minarea=10, ctx=ctx)['x'], masked['objects']['x'])
    assert 0 < masked['nobj'] < want['nobj']
    small = sep.extract(sub, 3.0, var=var, minarea=10, max_objects=2, ctx=ctx)
    assert len(small) == want['nobj'] and _same_bits(small['x'], want['objects']['x'])


# ---- lc_import_frames ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(512, 512), (333, 257)])
@pytest.mark.parametrize('mask_sources_first', [False, True])
def test_import_frames_against_the_separate_calls(ctx, shape, mask_sources_first):
    """Every output of the fused entry, doubles included, has the bits of subtract_background (or the two-pass form),
    the variance in np.float32 by the frozen formula, and sep.extract."""
    from lightcurver_amd import sep
    from lightcurver_amd.processes import background_estimation as BE
    from lightcurver_amd.processes.frame_importation import import_frames
    h, w = shape
    frames = np.stack([B.scene(h, w, 40, 50 + k) for k in range(2)])
    exptimes = np.array([30.0, 12.5], np.float32)
    r = import_frames(frames, exptimes, 10, mask_sources_first, 3, 10, segmentation_map=True, ctx=ctx)
    assert (r['status'] == 0).all() and (r['ex_status'] == 0).all() and (r['nobj'] > 10).all()
    for k in range(2):
        if mask_sources_first:
            sub, bkg = BE.subtract_background_masking_sources(frames[k], ctx=ctx)
        else:
            sub, bkg = BE.subtract_background(frames[k], ctx=ctx)
        assert _same_bits(r['sub'][k], sub)
        assert _same_bits(r['mesh_back'][k], bkg.mesh_back[0]) and _same_bits(r['mesh_rms'][k], bkg.mesh_rms[0])
        assert np.float32(bkg.globalback) == r['globalback'][k] and np.float32(bkg.globalrms) == r['globalrms'][k]
        var = E.variance_map(sub, bkg.globalrms, exptimes[k])
        objects, seg = sep.extract(sub, 3, var=var, minarea=10, segmentation_map=True, ctx=ctx)
        assert np.array_equal(seg, r['segmap'][k]) and len(objects) == r['nobj'][k]
        for f in sep.OBJECT_FIELDS:
            assert _same_bits(objects[f], r['objects'][k][f]), f
    if mask_sources_first:          # the second pass changed the sky
        plain = import_frames(frames, exptimes, 10, False, 3, 10, ctx=ctx)
        assert not _same_bits(plain['sub'], r['sub'])


def test_two_pass_sky_against_the_restatement(ctx):
    """subtract_background_masking_sources: the mask has the bits of the restatement's extraction (thresh 2, minarea 10,
    the scalar variance globalrms^2) of the first pass's sub, and the second pass those of the restated sky with it."""
    from lightcurver_amd.processes import background_estimation as BE
    frame = B.scene(130, 195, 40, 3)
    sub1, bkg1 = BE.subtract_background(frame, ctx=ctx)
    rms = np.float32(bkg1.globalrms)
    want_mask = E.extract(sub1, rms * rms, 2, 10, 1)['mask']
    subs, bkgs, masks = BE.subtract_background_masking_sources_batch(frame[None], ctx=ctx)
    assert np.array_equal(masks[0], want_mask) and 0 < want_mask.mean() < 0.5
    want = B.background(frame, mask=want_mask, bw=13, bh=13)
    print('pixels of sub that differ from the restatement:', int((subs[0] != want['sub']).sum()), 'largest difference',
          float(np.abs(subs[0] - want['sub']).max()), 'mesh values that differ:',
          int((bkgs[0].mesh_back[0] != want['mesh_back']).sum()))
    assert _same_bits(subs[0], want['sub'].astype(np.float32))
    assert np.float32(bkgs[0].globalrms) == np.float32(want['globalrms'])
    sub, bkg = BE.subtract_background_masking_sources(frame, ctx=ctx)
    assert _same_bits(sub, subs[0])


def test_characterize_frames_of_mixed_shapes_and_the_seeing(ctx):
    """Frames of two shapes in one list; the seeing of Gaussians of known width is the one the SPEC's own moments give
    (the restatement's catalogue of the same sub and variance through the same table and estimate_seeing)."""
    from lightcurver_amd.processes.frame_characterization import estimate_seeing
    from lightcurver_amd.processes.frame_importation import characterize_frames
    from lightcurver_amd.processes.star_extraction import sources_table_from_objects
    sigma = 2.0
    frames = [E.gaussian_scene(200, 300, 40, sigma, 1)[0] + 20.0, E.gaussian_scene(160, 180, 30, sigma, 2)[0] + 20.0,
              E.gaussian_scene(200, 300, 40, sigma, 3)[0] + 20.0]
    exptimes = [20.0, 30.0, 40.0]
    res = characterize_frames(frames, exptimes, ctx=ctx)
    assert len(res) == 3
    for f, t, r in zip(frames, exptimes, res):
        assert r['image_sub'].shape == f.shape and abs(r['bkg'].globalback - 20.0) < 1.0
        var = E.variance_map(r['image_sub'], r['bkg'].globalrms, t)
        want = sources_table_from_objects(E.extract(r['image_sub'], var, 3, 10, 1)['objects'])
        assert _same_bits(want['FWHM'], r['sources_table']['FWHM']) and len(want) >= 20
        assert r['seeing_pixels'] == float(estimate_seeing(want))
        assert r['ellipticity'] == float(np.nanmedian(want['ellipticity']))
        print(f'seeing {r["seeing_pixels"]:.3f} px for Gaussians of FWHM {2.3548 * sigma:.3f} px, {len(want)} sources')
        assert 0.5 * 2.3548 * sigma < r['seeing_pixels'] < 2.0 * 2.3548 * sigma
