"""GPU parity of the de-blended, cleaned source extraction of whole frames (lc_extract_frames_deblended and the imports
that take it; DESIGN.md §5 "De-blending and cleaning of frame objects") against the NumPy restatement of the SPEC
(tests/_deblend.py), with the tolerances of tests/test_extract_gpu.py: segmap, mask, nobj, status, every integer field,
peak, cpeak, x, y, a, b bit for bit; theta within 1e-12; flux within 1e-10 of the sum of |D| over the object.  Every
result is the same in two runs.  No input here is invalid: the capacity cases are answered with a flag or a status."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _deblend as D
from tests import _extract as E
from tests.test_extract_gpu import _check_frame, _same_bits

pytestmark = pytest.mark.gpu

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
SEP = dict(deblend_nthresh=32, deblend_cont=0.005, clean=True)


@pytest.fixture(scope='module')
def ctx():
    from lightcurver_amd import _lib
    return _lib.Context(0)


def _raw(ctx, frames, var, thresh, minarea, filt, deblend, max_objects=4096, entry='lc_extract_frames_deblended'):
    """The entry through ctypes with sentinels in every output."""
    from lightcurver_amd import _lib
    d = _lib.f32(frames)
    K, h, w = d.shape
    v = _lib.f32(var)
    plane = v if v.ndim == 3 else None
    scalar = None if v.ndim == 3 else np.ascontiguousarray(np.broadcast_to(v.reshape(-1), (K,)), np.float32)
    out = dict(objects=np.full((K, max_objects), 0x55, np.uint8).repeat(96, axis=1).view(_lib.EXTRACT_OBJECT_DTYPE),
               nobj=np.full(K, -9, np.int32), segmap=np.full(d.shape, -9, np.int32), mask=np.full(d.shape, 9, np.uint8),
               status=np.full(K, -9, np.int32))
    cfg = _lib.ExtractCfg(thresh, minarea, filt)
    s = dict(SEP, **deblend)
    dcfg = _lib.DeblendCfg(s['deblend_nthresh'], s['deblend_cont'], int(s['clean']), 1.0)
    ms = C.c_float()
    head = (ctx.h, K, h, w, _lib.ptr(d), _lib.ptr(plane), _lib.ptr(scalar), C.byref(cfg))
    tail = (max_objects, out['objects'].ctypes.data_as(C.c_void_p), out['nobj'].ctypes.data_as(_i32p),
            out['segmap'].ctypes.data_as(_i32p), out['mask'].ctypes.data_as(_u8p), out['status'].ctypes.data_as(_i32p),
            C.byref(ms))
    if entry == 'lc_extract_frames':
        ctx.check(_lib.lib().lc_extract_frames(*head, *tail), entry)
    else:
        ctx.check(_lib.lib().lc_extract_frames_deblended(*head, C.byref(dcfg), *tail), entry)
    return out


def _check_call(ctx, frames, var, thresh, minarea, filt, deblend, max_objects=4096, wants=None, what=''):
    frames = np.asarray(frames, np.float32)
    got = _raw(ctx, frames, var, thresh, minarea, filt, deblend, max_objects)
    again = _raw(ctx, frames, var, thresh, minarea, filt, deblend, max_objects)
    for name in got:
        assert _same_bits(got[name], again[name]), (what, name)
    v = np.asarray(var, np.float32)
    s = dict(SEP, **deblend)
    out = []
    for k in range(len(frames)):
        vk = v[k] if v.ndim == 3 else np.broadcast_to(v.reshape(-1), (len(frames),))[k]
        want = wants[k] if wants else D.extract(frames[k], vk, thresh, minarea, filt, s['deblend_nthresh'],
                                                 s['deblend_cont'], s['clean'], max_objects)
        _check_frame(got, k, want, frames[k], f'{what} frame {k}')
        out.append(want)
    return got, out


@functools.lru_cache(maxsize=None)
def _mosaic(cols):
    return D.mosaic(3, cols, 32, {8: 1, 6: 2}[cols])


# ---- the mosaics of the stamp scenes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('cols', [8, 6])
@pytest.mark.parametrize('settings', ['sep', 'merge'])
def test_mosaics(ctx, cols, settings):
    """96 x 256 and 96 x 192: splits to a depth of 2 and more at sep's defaults; clean merges at minarea 15, cont 0.001."""
    d, v = _mosaic(cols)
    s = {} if settings == 'sep' else D.MERGE_SETTINGS
    got, (want,) = _check_call(ctx, d[None], v[None], 3.0, s.get('minarea', 5), 1,
                               dict(deblend_cont=s.get('deblend_cont', 0.005)), what=f'{cols} {settings}')
    assert want['paths']['split'] >= 9 and want['paths']['depth'] >= 2
    assert (want['paths']['merged'] > 0) == (settings == 'merge')


@pytest.mark.parametrize('deblend', [dict(deblend_nthresh=4), dict(deblend_nthresh=8), dict(deblend_nthresh=16),
                                     dict(deblend_cont=1e-5), dict(clean=False), dict(deblend_cont=1e-5, clean=False)],
                         ids=lambda s: '-'.join(f'{k}={v}' for k, v in s.items()))
def test_settings_on_a_mosaic(ctx, deblend):
    d, v = _mosaic(8)
    got, (want,) = _check_call(ctx, d[None], v[None], 3.0, 5, 1, deblend, what=str(deblend))
    assert want['paths']['split'] > 0


# ---- hand-made frames -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', D.HAND_MADE)
def test_hand_made(ctx, name):
    """The blend across tile and block borders, boxes of 64 and 65 pixels, more than 32 leaves, the clean chain, children
    of 1 and 2 pixels, the blend on the frame edge, noise alone."""
    img, s = D.hand_made(name)
    want = D.hand_made_wanted(name)
    got, _ = _check_call(ctx, img[None], 1.0, s['thresh'], s['minarea'], s['filt'], dict(clean=s.get('clean', True)),
                         wants=[want], what=name)
    flags, p = got['objects']['flag'][0, :want['nobj']], want['paths']
    if name == 'box64':
        assert want['parents'][0]['region'].shape[1] == 64 and p['split'] == 1 and not (flags & 8).any()
    if name == 'box65':
        assert want['parents'][0]['region'].shape[1] == 65 and p['nodeblend_size'] == 1 and flags[0] & 8
    if name == 'overflow':
        assert p['nodeblend_capacity'] == 1 and want['nobj'] == 1 and flags[0] & 8 and got['status'][0] == 0
    if name == 'chain':
        assert p['chain'] == 1 and p['merged'] == 2 and want['nobj'] == 1
    if name == 'small_children':
        assert sorted(want['objects']['npix'])[:2] == [1, 2]
    if name == 'straddle':
        o = want['objects']
        assert p['split'] == 1 and o['xmin'].min() < 64 <= o['xmax'].max() and o['ymin'].min() < 16 <= o['ymax'].max()
    if name == 'edge_blend':
        assert p['split'] == 2 and (flags & 4).sum() >= 3
    if name == 'noise_only':
        assert want['nobj'] == 0


@pytest.mark.parametrize('shape', [(1, 1), (1, 300), (65, 17), (257, 129)])
def test_frame_shapes(ctx, shape):
    d, v = _mosaic(8)
    h, w = shape
    d, v = np.tile(d, (3, 2))[:h, :w], np.tile(v, (3, 2))[:h, :w]
    minarea = 1 if h == 1 else 5
    _check_call(ctx, d[None], v[None], 3.0, minarea, 1, dict(deblend_cont=0.001), what=str(shape))


def test_frames_that_differ_in_one_call(ctx):
    """K = 3: a blend, the chain and the parent that is kept whole, padded to one shape."""
    frames = np.zeros((3, 80, 300), np.float32)
    for k, name in enumerate(('straddle', 'chain', 'overflow')):
        img, _ = D.hand_made(name)
        frames[k, :img.shape[0], :img.shape[1]] = img
    got, wants = _check_call(ctx, frames, 1.0, 3.0, 5, 0, {})
    assert [x['nobj'] for x in wants] == [2, 1, 1] and wants[2]['paths']['nodeblend_capacity'] == 1


@functools.lru_cache(maxsize=None)
def _pairs():
    return D.pairs_scene(512, 512, 60, 12, 3)


def test_scene_with_pairs(ctx):
    sub, var, _ = _pairs()
    got, (want,) = _check_call(ctx, sub[None], var[None], 3.0, 10, 1, {})
    assert want['paths']['split'] >= 7


# ---- the table's capacity, the limit without de-blending ------------------------------------------------------------------

def test_a_table_that_is_too_small(ctx):
    from lightcurver_amd import sep
    d, v = _mosaic(8)
    full = D.extract(d, v, 3.0)
    cap = full['nobj'] // 2
    got, (want,) = _check_call(ctx, d[None], v[None], 3.0, 5, 1, {}, max_objects=cap)
    assert got['status'][0] == 1 and got['nobj'][0] == full['nobj'] and np.array_equal(got['segmap'][0], full['segmap'])
    r = sep.extract_frames(d[None], v[None], 3.0, max_objects=cap, segmentation_map=True, ctx=ctx, deblend=True)
    assert r['status'][0] == 0 and len(r['objects'][0]) == full['nobj']
    for f in E.EXACT_FIELDS:
        assert _same_bits(r['objects'][0][f], full['objects'][f]), f


def test_without_deblending_it_is_lc_extract_frames(ctx):
    """SPEC item 7, on the mosaic, the pairs and the two parents that are kept whole: everything but bit 8 is equal."""
    d, v = _mosaic(8)
    sub, var, _ = _pairs()
    off = dict(deblend_cont=1.0, clean=False)
    for frames, vv, minarea, filt in ((d[None], v[None], 5, 1), (sub[None], var[None], 10, 1),
                                      (D.hand_made('box65')[0][None], 1.0, 5, 0), (D.hand_made('overflow')[0][None], 1.0, 5, 0)):
        a = _raw(ctx, frames, vv, 3.0, minarea, filt, off)
        b = _raw(ctx, frames, vv, 3.0, minarea, filt, off, entry='lc_extract_frames')
        assert (a['objects']['flag'] & ~8 == b['objects']['flag']).all()
        a['objects']['flag'] &= ~8
        for name in a:
            assert _same_bits(a[name], b[name]), name
    assert _raw(ctx, D.hand_made('box65')[0][None], 1.0, 3.0, 5, 0, off)['objects']['flag'][0, 0] == 8


# ---- the imports ------------------------------------------------------------------------------------------------------------

def test_imports_against_the_separate_calls(ctx):
    from lightcurver_amd import sep
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.frame_importation import import_frames
    sub, _, _ = _pairs()
    stack = np.stack([sub[:256, :256], sub[256:, 256:]]) + np.float32(20.0)
    t = np.array([30.0, 45.0], np.float32)
    plain = import_frames(stack, t, n_boxes=4, ctx=ctx)
    r = import_frames(stack, t, n_boxes=4, segmentation_map=True, ctx=ctx, deblend=True)
    assert _same_bits(r['sub'], plain['sub']) and _same_bits(r['globalrms'], plain['globalrms'])
    var = np.stack([E.variance_map(r['sub'][k], r['globalrms'][k], t[k]) for k in range(2)])
    sepa = sep.extract_frames(r['sub'], var, 3, 10, segmentation_map=True, ctx=ctx, deblend=True)
    assert np.array_equal(r['segmap'], sepa['segmap']) and np.array_equal(r['nobj'], sepa['nobj'])
    assert (r['nobj'] > plain['nobj']).all()
    with FrameSet(stack, ctx=ctx) as fs:
        f = fs.import_frames(t, n_boxes=4, deblend=True)
        assert fs.imported
    for k in range(2):
        assert _same_bits(r['objects'][k], sepa['objects'][k]) and _same_bits(f['objects'][k], sepa['objects'][k])
    # the source mask of the two-pass sky is not de-blended: with it, the catalogue is again that of the separate call
    two = import_frames(stack, t, n_boxes=4, mask_sources_first=True, ctx=ctx, deblend=True)
    var = np.stack([E.variance_map(two['sub'][k], two['globalrms'][k], t[k]) for k in range(2)])
    sepa = sep.extract_frames(two['sub'], var, 3, 10, ctx=ctx, deblend=True)
    for k in range(2):
        assert _same_bits(two['objects'][k], sepa['objects'][k])


def test_extract_stars_finds_both_stars_of_a_pair(ctx):
    from lightcurver_amd.processes.star_extraction import extract_stars
    from lightcurver_amd import sep
    sub, var, pairs = _pairs()
    want = D.extract(sub, var, 3.0, minarea=10)
    objects, segmap = sep.extract_deblended(sub, 3.0, var=var, minarea=10, segmentation_map=True, ctx=ctx)
    assert np.array_equal(segmap, want['segmap'])
    whole = E.extract(sub, var, 3.0, 10)['segmap']
    split = 0
    for (ax, ay), (bx, by) in np.rint(pairs).astype(int):
        a, b = want['segmap'][ay, ax], want['segmap'][by, bx]
        if a > 0 and b > 0 and a != b and whole[ay, ax] == whole[by, bx]:
            split += 1
            assert (objects['npix'][a - 1], objects['npix'][b - 1]) == (want['objects']['npix'][a - 1], want['objects']['npix'][b - 1])
    assert split >= 6
    with_, without = extract_stars(sub, var, 3, 10, ctx=ctx, deblend=True), extract_stars(sub, var, 3, 10, ctx=ctx)
    assert len(with_) > len(without)
    noise = np.random.default_rng(1).normal(0, 1, (64, 64)).astype(np.float32)
    empty = extract_stars(noise, 1.0, 5, 10, ctx=ctx, deblend=True)
    assert len(empty) == 0 and 'FWHM' in empty.dtype.names


def test_error_codes(ctx):
    """As lc_segment_stamps: -3 for what is not built, -1 for what is invalid; nothing is launched."""
    from lightcurver_amd import _lib
    d = np.zeros((1, 8, 8), np.float32)
    one = np.ones(1, np.float32)
    cfg = _lib.ExtractCfg(3.0, 5, 1)
    nobj, status = np.zeros(1, np.int32), np.zeros(1, np.int32)

    def rc(dcfg):
        return _lib.lib().lc_extract_frames_deblended(ctx.h, 1, 8, 8, _lib.ptr(d), None, _lib.ptr(one), C.byref(cfg),
                                                      C.byref(dcfg) if dcfg is not None else None, 16, None,
                                                      nobj.ctypes.data_as(_i32p), None, None, status.ctypes.data_as(_i32p), None)

    assert rc(_lib.DeblendCfg(32, 0.005, 1, 1.0)) == 0
    assert rc(_lib.DeblendCfg(32, 0.005, 1, 0.5)) == -3 and rc(_lib.DeblendCfg(5, 0.005, 1, 1.0)) == -3
    assert rc(_lib.DeblendCfg(64, 0.005, 1, 1.0)) == -3
    assert rc(_lib.DeblendCfg(32, -0.1, 1, 1.0)) == -1 and rc(_lib.DeblendCfg(32, float('nan'), 1, 1.0)) == -1
    assert rc(None) == -1
    assert b'deblend' in _lib.lib().lc_last_error(ctx.h)
