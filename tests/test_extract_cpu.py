"""Source extraction of frames without a GPU: the restatement of the SPEC (tests/_extract.py) against an independent
float64 host form, the host-side pieces around the kernels (sources table, seeing, refusals) and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import _extract as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'seeing_golden.npz')


# ---- the restatement against a float64 host form ---------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [11, 12, 13])
def test_restatement_against_float64_host_form(seed):
    """Detection bits agree on every pixel whose float64 snr is further from thresh than the float32 bound of the
    nine-tap sums, 16 2^-24 sum k |dw| / sqrt(den2).  Objects without such a pixel inside or on their rim are the same
    pixel sets in both, equal in number, with x, y, a, b within 1e-3 pixels (the 2^-10 quantisation of the weights).
    At most 2 % of the objects may have to be left out."""
    thresh, minarea = 3.0, 10
    sub, var = E.scene(512, 512, 60, seed)
    R = E.extract(sub, var, thresh, minarea, filt=1)
    H = E.host_form(sub, var, thresh, minarea)
    unsure = np.abs(H['snr'] - thresh) <= H['bound']
    assert (R['det'] == H['det'])[~unsure].all()
    near = ndimage.binary_dilation(unsure, structure=E.EIGHT)
    assert R['nobj'] >= 40
    sizes = np.bincount(H['lab'].ravel(), minlength=H['ncomp'] + 1)
    host_objects = [c for c in range(1, H['ncomp'] + 1) if sizes[c] >= minarea]
    host_kept = [c for c in host_objects
                 if not near[ndimage.binary_dilation(H['lab'] == c, structure=E.EIGHT)].any()]
    kept, worst = 0, 0.0
    for num, o in enumerate(R['objects'], start=1):
        m = R['segmap'] == num
        if near[ndimage.binary_dilation(m, structure=E.EIGHT)].any():
            continue
        kept += 1
        c = H['lab'][o['ypeak'], o['xpeak']]
        assert c in host_kept and np.array_equal(H['lab'] == c, m)
        yy, xx = np.nonzero(m)
        x, y, a, b = E.host_moments(H['snr'], yy, xx)
        worst = max(worst, abs(o['x'] - x), abs(o['y'] - y), abs(o['a'] - a), abs(o['b'] - b))
    left_out = R['nobj'] - kept
    fwhm = 2 * np.sqrt(np.log(2) * (R['objects']['a'] ** 2 + R['objects']['b'] ** 2))
    print(f'seed {seed}: {R["nobj"]} objects of {R["ncomp"]} components, {left_out} left out, '
          f'{int(unsure.sum())} unsure pixels, worst moment difference {worst:.2e}, median FWHM {np.median(fwhm):.2f}')
    assert kept == len(host_kept)
    assert worst < 1e-3
    assert left_out <= 0.02 * R['nobj']


def test_restatement_patterns_and_flags():
    """The pattern frames are what the device tests believe them to be, and the flags of the SPEC."""
    for (h, w) in ((37, 53), (70, 1), (1, 70)):
        for kind in E.PATTERNS:
            det = E.pattern(kind, h, w)
            r = E.extract(E.pattern_frame(det), 1.0, 5.0, minarea=1, filt=0)
            assert np.array_equal(r['det'], det), kind
    h, w = 37, 53
    n = lambda kind, minarea: E.extract(E.pattern_frame(E.pattern(kind, h, w)), 1.0, 5.0, minarea, 0)
    assert n('checkerboard', 1)['nobj'] == 1 and n('serpentine', 1)['nobj'] == 1 and n('four_borders', 1)['nobj'] == 1
    assert n('isolated', 1)['nobj'] == 19 * 27 and n('isolated', 2)['nobj'] == 0
    assert n('rings', 1)['nobj'] > 5 and n('staircases', 1)['nobj'] > 5
    o = n('four_borders', 1)['objects'][0]
    assert o['flag'] == E.FLAG_EDGE and (o['xmin'], o['xmax'], o['ymin'], o['ymax']) == (0, w - 1, 0, h - 1)
    # LARGE: a side of 513 but not of 512; RANGE: 2^16 and above
    d = np.zeros((8, 600), np.float32)
    d[2, 10:523] = 10.0
    d[5, 10:522] = 10.0
    d[7, 3] = 1e9
    r = E.extract(d, 1.0, 5.0, 1, 0)
    assert list(r['objects']['flag']) == [E.FLAG_LARGE, 0, E.FLAG_RANGE | E.FLAG_EDGE]
    assert np.isnan(r['objects']['x'][[0, 2]]).all() and r['objects']['x'][1] == 10 + 511 / 2
    assert list(r['objects']['npix']) == [513, 512, 1]
    # minarea at, below and above a component's size; max_objects
    d = E.pattern_frame(E.pattern('rings', 21, 21))
    sizes = sorted(E.extract(d, 1.0, 5.0, 1, 0)['objects']['npix'])
    assert E.extract(d, 1.0, 5.0, sizes[1], 0)['nobj'] == len(sizes) - 1
    assert E.extract(d, 1.0, 5.0, sizes[1] + 1, 0)['nobj'] == len(sizes) - 2
    r = E.extract(d, 1.0, 5.0, 1, 0, max_objects=2)
    assert r['status'] == 1 and len(r['objects']) == 2 and r['nobj'] == len(sizes) and r['segmap'].max() == len(sizes)


# ---- estimate_seeing ----------------------------------------------------------------------------------------------------

def test_estimate_seeing_against_the_reference_function():
    """Golden values recorded from the reference's own function (tests/golden/make_seeing_golden.py).  The reference's
    branch for an empty window of +-1 around the refined peak cannot be reached with finite values (the fullest bin of
    the second histogram is 0.4 wide and holds values), so its case is the nearest input: values on the outer edges."""
    from lightcurver_amd.processes.frame_characterization import estimate_seeing
    g = np.load(GOLDEN)
    names = sorted({k.split('__')[0] for k in g.files})
    assert set(names) >= {'clear_peak', 'peak_first_bin', 'peak_last_bin', 'narrow_window_edges', 'few', 'one', 'ten', 'none'}
    for name in names:
        fwhm, want = g[f'{name}__fwhm'], float(g[f'{name}__seeing'])
        got = estimate_seeing({'FWHM': fwhm})
        assert float(got) == want, name
    assert float(g['none__seeing']) == -1.0 and len(g['none__fwhm']) == 0
    assert len(g['clear_peak__fwhm']) > 10 and 1 <= len(g['few__fwhm']) <= 10 and len(g['ten__fwhm']) == 10
    # the cases sit where their names say: the peak of the first histogram
    for name, where in (('peak_first_bin', 0), ('peak_last_bin', 9)):
        f = g[f'{name}__fwhm']
        hist, _ = np.histogram(f, bins=10, range=(1.5, min(30.0, 3.0 * max(np.median(f), 1.5))))
        assert int(np.argmax(hist)) == where and len(f) > 10 and float(g[f'{name}__seeing']) == np.median(f)


# ---- the sources table ----------------------------------------------------------------------------------------------------

def _catalogue():
    """Fourteen round objects, a streak (row 4) and an unmeasured object (the last row)."""
    from lightcurver_amd import sep
    o = np.zeros(16, sep.OBJECT_DTYPE)
    n = np.arange(16)
    o['x'], o['y'] = 10.25 * (n + 1), 5.0 + n
    o['a'], o['b'] = 2.0 + 0.01 * n, 1.9
    o['a'][4], o['b'][4] = 9.0, 1.0
    o['flux'] = 100.0 + 10.0 * ((7 * n) % 16)          # all different ...
    o['flux'][9] = o['flux'][2]                        # ... but for one pair
    o['flux'][4] = 5000.0
    o['npix'] = 30 + n
    o['flag'][3] = 4
    for f in ('x', 'y', 'a', 'b', 'theta'):
        o[f][15] = np.nan
    o['flux'][15], o['flag'][15] = 7000.0, 1
    return o


def test_sources_table_from_objects():
    from lightcurver_amd.processes.star_extraction import sources_table_from_objects
    o = _catalogue()
    t = sources_table_from_objects(o)
    for col in ('xcentroid', 'ycentroid', 'flag', 'a', 'b', 'flux', 'npix', 'elongation', 'FWHM', 'ellipticity', 'x', 'y'):
        assert col in t.dtype.names
    # the cut: the streak is above median + 3 std of the fifteen measured elongations, the NaN row fails every comparison
    el = o['a'][:15] / o['b'][:15]
    cut = np.median(el) + 3 * np.std(el)
    assert el[4] > cut and (np.delete(el, 4) < cut).all()
    assert len(t) == 14 and not np.isnan(t['a']).any() and 9.0 not in t['a'] and 7000.0 not in t['flux']
    # brightest first, equal fluxes in the catalogue's order
    kept = np.delete(np.arange(15), 4)
    order = kept[np.argsort(-o['flux'][kept], kind='stable')]
    assert np.array_equal(t['npix'], o['npix'][order]) and (np.diff(t['flux']) <= 0).all()
    pair = np.nonzero(t['flux'] == o['flux'][2])[0]
    assert list(t['npix'][pair]) == [32, 39]
    assert np.array_equal(t['xcentroid'], t['x']) and np.array_equal(t['ycentroid'], t['y'])
    assert np.array_equal(t['elongation'], t['a'] / t['b'])
    assert np.array_equal(t['FWHM'], 2 * (np.log(2) * (t['a'] ** 2 + t['b'] ** 2)) ** 0.5)
    assert np.array_equal(t['ellipticity'], 1 - t['b'] / t['a'])
    assert sorted(t['flag']) == [0] * 13 + [4] and t['npix'].dtype == np.int32


def test_sources_table_of_an_empty_catalogue(recwarn):
    from lightcurver_amd import sep
    from lightcurver_amd.processes.frame_characterization import estimate_seeing
    from lightcurver_amd.processes.star_extraction import sources_table_from_objects
    t = sources_table_from_objects(np.zeros(0, sep.OBJECT_DTYPE))
    assert len(t) == 0 and len(recwarn) == 0
    # the reference's own test of extract_stars, at the level of the table
    for col in ('xcentroid', 'ycentroid', 'flag', 'a', 'b', 'flux', 'npix', 'FWHM', 'ellipticity', 'elongation'):
        assert col in t.dtype.names
    assert estimate_seeing(t) == -1.0
    # a catalogue of unmeasured objects alone is empty as well
    o = np.zeros(2, sep.OBJECT_DTYPE)
    for n in ('x', 'y', 'a', 'b', 'theta'):
        o[n] = np.nan
    assert len(sources_table_from_objects(o)) == 0 and len(recwarn) == 0


# ---- ABI and refusals -------------------------------------------------------------------------------------------------------

def _header():
    text = open(os.path.join(ROOT, 'include', 'lcmi.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def _struct_fields(name):
    m = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*' + name + r'\s*;', _header())
    assert m, name
    fields = []
    for decl in m.group(1).split(';'):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(',')]
    return fields


def test_structs_and_prototypes_match_the_header():
    from lightcurver_amd import _lib
    kinds = {'float': ctypes.c_float, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double}
    for name, cls, size in (('lc_extract_cfg', _lib.ExtractCfg, 12), ('lc_extract_object', _lib.ExtractObject, 96)):
        declared = _struct_fields(name)
        assert [(n, kinds[t]) for n, t in declared] == list(cls._fields_), name
        assert ctypes.sizeof(cls) == size
    assert [n for n, _ in _lib.ExtractObject._fields_] == ['first', 'npix', 'xmin', 'xmax', 'ymin', 'ymax', 'xpeak', 'ypeak',
                                                           'flag', 'pad', 'peak', 'cpeak', 'x', 'y', 'a', 'b', 'theta', 'flux']
    assert _lib.EXTRACT_OBJECT_DTYPE.itemsize == 96 and _lib.EXTRACT_OBJECT_DTYPE == E.OBJECT_DTYPE
    assert [_lib.EXTRACT_OBJECT_DTYPE.fields[n][1] for n, _ in _lib.ExtractObject._fields_] == \
        [getattr(_lib.ExtractObject, n).offset for n, _ in _lib.ExtractObject._fields_]
    ctype = {'int': ctypes.c_int, 'float *': _lib.fp, 'const float *': _lib.fp, 'lc_ctx *': _lib.vp,
             'uint8_t *': ctypes.POINTER(ctypes.c_uint8), 'int32_t *': _lib.ip, 'lc_extract_object *': _lib.vp,
             'const lc_extract_cfg *': ctypes.POINTER(_lib.ExtractCfg),
             'const lc_background_cfg *': ctypes.POINTER(_lib.BackgroundCfg)}
    for name in ('lc_extract_supported', 'lc_extract_frames', 'lc_import_frames'):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', _header())
        args = [a.strip() for a in m.group(1).split(',')]
        res, proto = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(proto) == len(args), name
        for a, p in zip(args, proto):
            assert ctype[re.sub(r'\w+$', '', a).strip()] is p, (name, a)
    s = _lib.lib().lc_extract_supported
    assert s(1, 1) == 1 and s(2048, 2048) == 1 and s(46340, 46340) == 1 and s(46341, 46341) == 0
    assert s(0, 5) == 0 and s(5, 0) == 0 and s(-1, 5) == 0 and s(1, 2 ** 31 - 1) == 1 and s(2, 2 ** 30) == 0


def test_python_refuses_what_is_not_built():
    from lightcurver_amd import sep
    from lightcurver_amd.processes.background_estimation import subtract_background
    img = np.zeros((40, 40), np.float32)
    with pytest.raises(NotImplementedError, match='de-blending'):
        sep.extract(img, 3.0, deblend_cont=0.005)
    with pytest.raises(NotImplementedError, match='cleaning'):
        sep.extract(img, 3.0, clean=True)
    with pytest.raises(NotImplementedError, match='filter_kernel'):
        sep.extract(img, 3.0, filter_kernel=np.ones((3, 3)))
    with pytest.raises(NotImplementedError, match='filter_kernel'):
        sep.extract(img, 3.0, filter_kernel=np.ones((5, 5)))
    with pytest.raises(ValueError):
        sep.extract(img, 0.0)
    with pytest.raises(ValueError):
        sep.extract(img, 3.0, minarea=0)
    with pytest.raises(ValueError):
        sep.extract(img, 3.0, err=1.0, var=1.0)
    with pytest.raises(ValueError):
        sep.extract(img[0], 3.0)
    with pytest.raises(ValueError):
        sep.extract_frames(img, 1.0, 3.0)
    assert 'deblend_cont=0.005' in sep.extract.__doc__ and 'clean=True' in sep.extract.__doc__
    # the one-pass function keeps its refusal: the two-pass form is a function of its own
    with pytest.raises(NotImplementedError, match='mask='):
        subtract_background(img, mask_sources_first=True)
