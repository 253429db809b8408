"""The restatement of the de-blended extraction (tests/_deblend.py; DESIGN.md §5 "De-blending and cleaning of frame
objects") against the float64 host form (processes/source_masking.py), its own invariants, and the interface of
lc_extract_frames_deblended as far as it can be checked without a device."""
import ctypes
import functools
import re

import numpy as np
import pytest

from tests import _deblend as D
from tests import _extract as E
from tests.test_extract_cpu import _header, _struct_fields

# (name, frame, variance, settings): the mosaics at sep's defaults and at the merge-producing settings, the scene with pairs
INPUTS = (('mosaic 3 x 8', lambda: D.mosaic(3, 8, 32, 1), {}),
          ('mosaic 3 x 8 merge', lambda: D.mosaic(3, 8, 32, 1), D.MERGE_SETTINGS),
          ('mosaic 3 x 6', lambda: D.mosaic(3, 6, 32, 2), {}),
          ('mosaic 3 x 6 merge', lambda: D.mosaic(3, 6, 32, 2), D.MERGE_SETTINGS),
          ('pairs 512', lambda: D.pairs_scene(512, 512, 60, 12, 3)[:2], dict(minarea=10)))
TIE_RATE = 0.02          # parents the host form may split differently: exact ties of left-over pixels


@functools.lru_cache(maxsize=None)
def _restated(i):
    name, make, s = INPUTS[i]
    d, v = make()
    return d, v, dict(dict(minarea=5, deblend_cont=0.005), **s), D.extract(d, v, 3.0, **s)


def _partition(masks_or_sets, shape=None):
    out = set()
    for m in masks_or_sets:
        yy, xx = m if isinstance(m, tuple) else np.nonzero(m)
        out.add(frozenset(zip(yy.tolist(), xx.tolist())))
    return out


def test_restatement_against_the_float64_host_form():
    """Per parent source_masking._deblend on the parent's box, then source_masking.clean on the leaves of all parents of
    the frame.  Measured on these inputs: 0 of 138 parents differ (61 of them are split), and no frame differs after clean."""
    from lightcurver_amd.processes import source_masking as M
    parents = differ = 0
    for i in range(len(INPUTS)):
        d, v, s, r = _restated(i)
        d64, n64 = d.astype(np.float64), np.sqrt(v.astype(np.float64))
        ok = np.isfinite(d64) & np.isfinite(n64) & (n64 > 0)
        snr = M.matched_filter_snr(np.where(ok, d64, 0.0), np.where(ok, n64, np.inf))
        cont = float(np.float32(s['deblend_cont']))
        leaves, same = [], True
        for p in r['parents']:
            host = M._deblend(snr[p['sl']], p['region'], 3.0, 32, cont, s['minarea'])
            parents += 1
            if len(host) != len(p['leaves']) or _partition(host) != _partition(p['leaves']):
                differ += 1
                same = False
            for m in host:
                full = np.zeros(d.shape, bool)
                full[p['sl']] = m
                leaves.append(full)
        print(INPUTS[i][0], 'parents', len(r['parents']), 'differ so far', differ)
        if same:            # the frame-level clean on equal leaves: the same survivors
            assert _partition(M.clean(leaves, snr, 3.0, s['minarea'])) == _partition(r['sets']), INPUTS[i][0]
    assert parents >= 80 and differ <= TIE_RATE * parents, (differ, parents)


def test_clean_targets_without_the_not_yet_merged_condition():
    """SPEC item 5 (c): every object picks its target on its own; item 6 of "Source masking" as it stands, faintest first
    with the condition, gives the same targets, on every input and on the chain."""
    results = [_restated(i)[3] for i in range(len(INPUTS))] + [D.hand_made_wanted(n) for n in D.HAND_MADE]
    for r in results:
        assert r['targets'] == r['sequential_targets']
    assert sum(r['paths']['merged'] for r in results) >= 5 and D.hand_made_wanted('chain')['paths']['chain'] == 1


def test_every_path_occurs():
    paths = [_restated(i)[3]['paths'] for i in range(len(INPUTS))] + [D.hand_made_wanted(n)['paths'] for n in D.HAND_MADE]
    assert max(p['split'] for p in paths) >= 9 and max(p['depth'] for p in paths) >= 3
    for name in ('merged', 'chain', 'nodeblend_size', 'nodeblend_capacity'):
        assert any(p[name] for p in paths), name
    # the hand-made frames are what their names say
    want = {n: D.hand_made_wanted(n) for n in D.HAND_MADE}
    assert want['box64']['parents'][0]['region'].shape[1] == 64 and want['box64']['nobj'] == 2
    assert want['box65']['parents'][0]['region'].shape[1] == 65 and list(want['box65']['objects']['flag']) == [8]
    assert want['overflow']['parents'][0]['region'].shape == (64, 64) and list(want['overflow']['objects']['flag']) == [8]
    assert sorted(want['small_children']['objects']['npix']) == [1, 2, 37]
    assert want['noise_only']['nobj'] == 0 and want['chain']['nobj'] == 1 and want['chain']['base']['nobj'] == 3
    o = want['straddle']['objects']
    assert len(o) == 2 and o['xmin'].min() < 64 <= o['xmax'].max() and o['ymin'].min() < 16 <= o['ymax'].max()
    first = int(o['first'][1])          # the second child starts where a block of 256 pixels and four tiles meet, or near
    assert (o['flag'] == 0).all() and abs(first - 19 * 256) < 3 * 300
    assert (want['edge_blend']['objects']['flag'] & 4).sum() >= 3


def test_without_deblending_it_is_the_plain_extraction():
    for i in (0, 4):
        d, v, s, _ = _restated(i)
        a = D.extract(d, v, 3.0, minarea=s['minarea'], deblend_cont=1.0, clean=False)
        b = E.extract(d, v, 3.0, s['minarea'])
        assert a['nobj'] == b['nobj'] and np.array_equal(a['segmap'], b['segmap'])
        assert a['objects'].tobytes() == b['objects'].tobytes()
    img, s = D.hand_made('box65')
    a = D.extract(img, np.float32(1), 3.0, 5, 0, deblend_cont=1.0, clean=False)
    assert list(a['objects']['flag']) == [8] and list(E.extract(img, np.float32(1), 3.0, 5, 0)['objects']['flag']) == [0]


# ---- the interface -------------------------------------------------------------------------------------------------------

def test_struct_and_prototypes_match_the_header():
    from lightcurver_amd import _lib
    kinds = {'float': ctypes.c_float, 'int32_t': ctypes.c_int32}
    declared = _struct_fields('lc_deblend_cfg')
    assert [(n, kinds[t]) for n, t in declared] == list(_lib.DeblendCfg._fields_)
    assert [n for n, _ in declared] == ['deblend_nthresh', 'deblend_cont', 'clean', 'clean_param']
    assert ctypes.sizeof(_lib.DeblendCfg) == 16
    ctype = {'int': ctypes.c_int, 'float *': _lib.fp, 'const float *': _lib.fp, 'lc_ctx *': _lib.vp, 'lc_frames *': _lib.vp,
             'uint8_t *': ctypes.POINTER(ctypes.c_uint8), 'int32_t *': _lib.ip, 'lc_extract_object *': _lib.vp,
             'const lc_extract_cfg *': ctypes.POINTER(_lib.ExtractCfg),
             'const lc_deblend_cfg *': ctypes.POINTER(_lib.DeblendCfg),
             'const lc_background_cfg *': ctypes.POINTER(_lib.BackgroundCfg)}
    for name, parent, after in (('lc_extract_frames_deblended', 'lc_extract_frames', 'cfg'),
                                ('lc_import_frames_deblended', 'lc_import_frames', 'ecfg'),
                                ('lc_frames_import_deblended', 'lc_frames_import', 'ecfg')):
        args = {}
        for n in (name, parent):
            m = re.search(r'\bint\s+' + n + r'\s*\(([^;]*)\)\s*;', _header())
            assert m, n
            args[n] = [a.strip() for a in m.group(1).split(',')]
        res, proto = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(proto) == len(args[name]), name
        for a, p in zip(args[name], proto):
            assert ctype[re.sub(r'\w+$', '', a).strip()] is p, (name, a)
        # the parent's arguments, with dcfg after its catalogue settings
        at = [re.search(r'\w+$', a).group(0) for a in args[parent]].index(after) + 1
        assert args[name][:at] + args[name][at + 1:] == args[parent] and args[name][at] == 'const lc_deblend_cfg *dcfg', name
        assert hasattr(_lib.lib(), name)
    assert '#define LC_EXTRACT_FLAG_NODEBLEND 8' in _header()


def test_python_refusals_and_defaults():
    import inspect
    from lightcurver_amd import sep
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.frame_importation import characterize_frames, import_frames
    from lightcurver_amd.processes.star_extraction import extract_stars
    img = np.zeros((40, 40), np.float32)
    assert sep.FLAG_NODEBLEND == 8
    with pytest.raises(NotImplementedError, match='clean_param'):
        sep.extract_deblended(img, 3.0, clean_param=0.5)
    with pytest.raises(NotImplementedError, match='deblend_nthresh'):
        sep.extract_deblended(img, 3.0, deblend_nthresh=5)
    with pytest.raises(NotImplementedError, match='deblend_nthresh'):
        sep.extract_frames(img[None], 1.0, 3.0, deblend=dict(deblend_nthresh=64))
    with pytest.raises(ValueError, match='deblend_cont'):
        sep.extract_deblended(img, 3.0, deblend_cont=-0.1)
    with pytest.raises(ValueError, match='deblend_cont'):
        sep.extract_deblended(img, 3.0, deblend_cont=np.nan)
    with pytest.raises(TypeError):
        sep.extract_frames(img[None], 1.0, 3.0, deblend=dict(contrast=0.1))
    with pytest.raises(NotImplementedError, match='filter_kernel'):
        sep.extract_deblended(img, 3.0, filter_kernel=np.ones((5, 5)))
    with pytest.raises(ValueError):
        sep.extract_deblended(img, 0.0)
    # sep's defaults on the new function; today's behaviour as the default of every new keyword
    p = inspect.signature(sep.extract_deblended).parameters
    assert (p['deblend_nthresh'].default, p['deblend_cont'].default, p['clean'].default, p['clean_param'].default,
            p['minarea'].default) == (32, 0.005, True, 1.0, 5)
    assert list(p)[:7] == list(inspect.signature(sep.extract).parameters)[:7]
    assert inspect.signature(sep.extract_frames).parameters['deblend'].default is None
    for f in (extract_stars, import_frames, characterize_frames, FrameSet.import_frames):
        assert inspect.signature(f).parameters['deblend'].default is False, f
    assert sep.deblend_cfg(None) is None and sep.deblend_cfg(False) is None
    c = sep.deblend_cfg(True)
    assert (c.deblend_nthresh, c.clean, c.clean_param) == (32, 1, 1.0) and c.deblend_cont == np.float32(0.005)
    c = sep.deblend_cfg(dict(deblend_cont=1.0, clean=False))
    assert (c.deblend_nthresh, c.deblend_cont, c.clean) == (32, 1.0, 0)
    # a missing context is refused before anything else, as by the other entries
    assert sep._lib.lib().lc_extract_frames_deblended(None, 1, 4, 4, None, None, None, None, None, 1, None, None, None,
                                                     None, None, None) == -1


def test_an_empty_catalogue_keeps_every_column():
    """What extract_stars(deblend=True) makes of a frame without sources (the reference's own test of extract_stars)."""
    from lightcurver_amd import sep
    from lightcurver_amd.processes.star_extraction import sources_table_from_objects
    want = D.hand_made_wanted('noise_only')
    t = sources_table_from_objects(sep.objects_view(want['objects']))
    assert len(t) == 0
    for col in ('xcentroid', 'ycentroid', 'flag', 'a', 'b', 'flux', 'npix', 'FWHM', 'ellipticity', 'elongation'):
        assert col in t.dtype.names
