"""The NumPy restatement of the sky-background SPEC (tests/_background.py, DESIGN.md §5 "Sky background") against what
can be pinned without a GPU and without sep: its spline against scipy's natural cubic spline, its filter against scipy's
median filter, the merge-path form of the two-ended walk against the serial walk, the reference's own test of
subtract_background, the paths the test scenes take, and the float32-against-float64 figures that set the bounds of
tests/test_background_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.interpolate import CubicSpline
from scipy.ndimage import median_filter

from tests import _background as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy_map(mesh, h, w, bw, bh):
    """scipy's natural cubic spline through the nodes at (k + 0.5) b - 0.5, along y, then along x per image line."""
    ny, nx = mesh.shape
    node = np.repeat(mesh, h, axis=0)
    if ny > 1:
        yn = (np.arange(ny) + 0.5) * bh - 0.5
        node = CubicSpline(yn, mesh, axis=0, bc_type='natural', extrapolate=True)(np.arange(h, dtype=np.float64))
    if nx == 1:
        return np.repeat(node, w, axis=1)
    xn = (np.arange(nx) + 0.5) * bw - 0.5
    return CubicSpline(xn, node, axis=1, bc_type='natural', extrapolate=True)(np.arange(w, dtype=np.float64))


@pytest.mark.parametrize('ny,nx', [(1, 1), (1, 3), (2, 2), (3, 2), (2, 9), (3, 3), (9, 9), (9, 1)])
def test_spline_equals_scipys_natural_cubic_spline(ny, nx):
    rng = np.random.default_rng(100 * ny + nx)
    bw, bh = 7, 5
    h, w = (ny - 1) * bh + 2, (nx - 1) * bw + 3           # a partial last mesh on both axes
    assert B.grid(h, w, bw, bh) == (ny, nx) and h % bh and w % bw
    mesh = rng.normal(0.0, 1.0, (ny, nx))
    got = B.spline_map(mesh, h, w, bw, bh, np.float64)
    want = _scipy_map(mesh, h, w, bw, bh)
    err = np.abs(got - want).max()
    print(f'ny {ny} nx {nx}: largest difference from scipy {err:.2e}')
    assert err < 1e-12
    # float32 evaluation of the same spline: a few roundings of values of order 1 (cubes of |B| <= 1.5 in the last piece)
    err32 = np.abs(B.spline_map(mesh, h, w, bw, bh, np.float32) - want).max()
    assert err32 < 64 * np.finfo(np.float32).eps * max(1.0, np.abs(mesh).max())


def test_filter_equals_scipys_median_in_the_interior_and_shrinks_at_the_edge():
    rng = np.random.default_rng(5)
    v = rng.normal(0.0, 1.0, (7, 9)).astype(np.float32)
    got = B.median_filter(v, 3, 3)
    assert np.array_equal(got[1:-1, 1:-1], median_filter(v, size=(3, 3))[1:-1, 1:-1])
    assert np.array_equal(B.median_filter(v, 1, 1), v)
    # hand cases: a corner keeps its value, an edge mesh takes the median of its three along the edge
    a = np.array([[9, 1, 5, 7], [2, 8, 3, 4], [6, 0, 11, 10]], np.float32)
    f = B.median_filter(a, 3, 3)
    assert f[0, 0] == 9 and f[0, 3] == 7 and f[2, 0] == 6 and f[2, 3] == 10
    assert f[0, 1] == 5 and f[0, 2] == 5 and f[2, 1] == 6 and f[2, 2] == 10
    assert f[1, 0] == 6 and f[1, 3] == 7
    assert f[1, 1] == 5 and f[1, 2] == 5           # medians of 0 1 2 3 5 6 8 9 11 and of 0 1 3 4 5 7 8 10 11
    one_row = np.array([[3, 1, 2, 5]], np.float32)
    assert np.array_equal(B.median_filter(one_row, 3, 3), [[3, 2, 2, 5]])
    # the global values: even counts take the mean of the two middle values, a zero rms median falls to the positive ones
    gb, gr = B.global_values(np.array([[1, 4], [2, 8]], np.float32), np.array([[0, 0], [0, 3]], np.float32))
    assert gb == 3 and gr == 3
    gb, gr = B.global_values(np.array([[1, 4, 2]], np.float32), np.array([[0, 2, 4]], np.float32))
    assert gb == 2 and gr == 2


HAND_HISTOGRAMS = [
    [5],                                  # a single bin
    [0],
    [0, 0, 0, 0],                         # nothing but empty bins
    [0, 0, 7, 0, 0],                      # a single occupied bin
    [3, 3],
    [1, 1, 1, 1, 1, 1],                   # ties at every step
    [2, 0, 0, 2, 0, 0, 2],                # ties across empty bins
    [0, 0, 0, 9],
    [9, 0, 0, 0],
    [1, 2, 3, 4, 5, 4, 3, 2, 1],
    [4, 0, 4, 0, 4, 0, 4, 0],
    [10, 1, 1, 1, 1, 1, 1, 1, 1, 2],
]


def _walks_agree(histo, lcut, hcut):
    histo = np.asarray(histo, np.int64)
    want = B.walk_serial(histo, lcut, hcut) if hcut >= lcut else (lcut, hcut, 0, 0)
    got = B.walk_merge(np.cumsum(histo), lcut, hcut)
    assert got == want, (histo.tolist(), lcut, hcut, got, want)


def test_merge_path_walk_equals_the_serial_walk():
    for hst in HAND_HISTOGRAMS:
        n = len(hst)
        for lcut in range(n):
            for hcut in range(lcut - 1, n):
                _walks_agree(hst, lcut, hcut)
    rng = np.random.default_rng(11)
    for i in range(1000):
        n = int(rng.integers(1, 200))
        kind = i % 4
        if kind == 0:
            hst = rng.poisson(rng.uniform(0.2, 30.0), n)
        elif kind == 1:
            hst = rng.integers(0, 3, n)                           # many ties and empty bins
        elif kind == 2:
            hst = np.where(rng.random(n) < 0.1, rng.integers(1, 50, n), 0)   # mostly empty
        else:
            x = np.arange(n)
            hst = rng.poisson(200.0 * np.exp(-0.5 * ((x - n / 2) / max(n / 8, 1)) ** 2))
        _walks_agree(hst, 0, n - 1)
        lcut = int(rng.integers(0, n))
        _walks_agree(hst, lcut, int(rng.integers(lcut, n)))


def test_mode_with_either_walk_is_the_same_number():
    s = B.scene(130, 195, 40, 3)
    for box in (65, 13):
        a = B.background(s, bw=box, bh=box, maps=False, walk='merge')
        b = B.background(s, bw=box, bh=box, maps=False, walk='serial')
        assert np.array_equal(a['raw_back'], b['raw_back']) and np.array_equal(a['raw_rms'], b['raw_rms'])


def test_the_references_own_pin():
    """tests/test_processes/test_background_estimation.py of the reference: a normal(100, 5) frame, n_boxes = 10."""
    img = np.random.default_rng(1).normal(100.0, 5.0, (100, 100))
    box = min(img.shape) // 10
    r = B.background(img, bw=box, bh=box, fw=3, fh=3)
    print('globalback', r['globalback'], 'globalrms', r['globalrms'])
    assert abs(r['globalback'] - 100.0) < 10.0
    assert abs(r['globalrms'] - 5.0) < 0.5
    assert abs(r['sub'].mean()) < 0.5 and r['sub'].shape == img.shape


def test_scenes_take_the_paths_they_are_there_for():
    s = B.scene(130, 195, 40, 3)
    p = B.background(s, bw=65, bh=65, maps=False)['paths']
    assert p['capped'] > 0 and B.grid(130, 195, 65, 65) == (2, 3)
    p = B.background(s, bw=13, bh=13, maps=False)['paths']
    print('box 13: mode', p['mode'], 'median', p['median'])
    assert p['mode'] > 0 and p['median'] > 0 and p['capped'] == 0
    p = B.background(s, bw=8, bh=8, maps=False)['paths']
    assert p['partial_x'] and p['partial_y']
    p = B.background(np.full((12, 12), 7.0, np.float32), bw=12, bh=12, maps=False)['paths']
    assert p['mean'] == 1 and p['single_x'] and p['single_y']
    m = np.zeros((130, 195), bool)
    m[:30, :50] = True
    r = B.background(s, mask=m, bw=13, bh=13, maps=False)
    assert r['paths']['bad'] > 0 and r['paths']['filled'] == r['paths']['bad'] and np.isfinite(r['mesh_back']).all()
    r = B.background(s, mask=np.ones_like(m), bw=13, bh=13)
    assert r['status'] == B.LC_ERR_NONFINITE and np.isnan(r['globalrms']) and np.isnan(r['sub']).all()


def test_a_mesh_of_one_level_is_the_moments_of_its_pixels():
    """One pixel inside the cuts gives one level and no round of the mode: the result is the mean of step 3, not a bin
    index.  One-pixel meshes are their pixels, and a one-pixel corner mesh (h % box = w % box = 1) stays with the sky."""
    f = B.scene(33, 50, 3, 22)
    r = B.background(f, bw=1, bh=1, fw=1, fh=1)
    assert r['paths']['single'] == 33 * 50
    assert np.array_equal(r['mesh_back'], f) and np.all(r['mesh_rms'] == 0) and r['globalrms'] == 0
    assert np.abs(r['sub']).max() <= 2e-5 * np.abs(f).max()
    st = B.backstat(np.array([42.5], np.float32), 1)
    assert st['nlevels'] == 1 and B.backguess(B.backhisto(np.array([42.5], np.float32), st), st) == (42.5, 0.0, 'single')
    # two pixels inside the cuts make two levels, and the rounds run
    st = B.backstat(np.array([42.5, 43.5], np.float32), 2)
    assert st['nlevels'] == 2 and B.backguess(B.backhisto(np.array([42.5, 43.5], np.float32), st), st)[2] != 'single'
    frame, box, sky, sigma = B.one_pixel_corner_frame()
    r = B.background(frame, bw=box, bh=box)
    assert r['paths']['single'] == 1 and r['raw_back'][-1, -1] == frame[-1, -1] and r['mesh_back'][-1, -1] == frame[-1, -1]
    assert np.abs(r['mesh_back'] - sky).max() < 5 * sigma          # five sigma of one pixel, the weakest mesh
    assert np.abs(r['back'][-box:, -box:] - sky).max() < 5 * sigma
    assert abs(r['globalback'] - sky) < 0.1 * sky and abs(r['globalrms'] - sigma) < 0.1 * sigma


def test_bad_meshes_take_the_nearest_good_ones():
    nan = np.float32(np.nan)
    b = np.array([[1, nan, 3], [nan, nan, 7], [5, 9, nan]], np.float32)
    r = b * 2
    fb, fr, filled = B.fill_bad(b, r)
    assert filled == 4
    assert fb[0, 1] == 2 and fb[1, 0] == 3 and fb[2, 2] == 8          # (1 + 3) / 2, (1 + 5) / 2, (7 + 9) / 2
    assert fb[1, 1] == 8                                              # only 7 and 9 at distance 1
    assert np.array_equal(fr, fb * 2)


@pytest.mark.parametrize('case', B.UNEQUAL_CASES)
def test_unequal_mesh_sides_cannot_be_swapped_unnoticed(case):
    """The condition of B.UNEQUAL_CASES: with the sides swapped, or one side used for both, the grid has another shape,
    and the swapped restatement's globalback is far outside four times the precision figure, the device's bound."""
    h, w, bw, bh, nstars, seed, K, shape = case
    assert bw != bh and B.grid(h, w, bw, bh) == shape
    assert len({shape, B.grid(h, w, bh, bw), B.grid(h, w, bw, bw), B.grid(h, w, bh, bh)}) == 4
    frames, wants = B.unequal_wanted(case)
    assert frames.shape == (K, h, w)
    bound = 4.0 * B.precision_figures()['mesh_back']
    for frame, want in zip(frames, wants):
        assert want['status'] == 0 and want['mesh_back'].shape == shape and want['mesh_rms'].shape == shape
        swapped = B.background(frame, bw=bh, bh=bw, maps=False)
        off = abs(float(swapped['globalback']) - float(want['globalback'])) / float(want['globalrms'])
        print(f'{h} x {w} in {bw} x {bh}: grid {shape}, swapped {swapped["mesh_back"].shape}; globalback '
              f'{want["globalback"]:.4f}, swapped {swapped["globalback"]:.4f}: {off:.3g} of globalrms (the device bound '
              f'{bound:.3g})')
        assert off > 10 * bound
        # the map through these mesh values: against scipy's spline with the nodes of these sides
        got = B.spline_map(want['mesh_back'], h, w, bw, bh, np.float64)
        ref = _scipy_map(want['mesh_back'].astype(np.float64), h, w, bw, bh)
        assert np.abs(got - ref).max() < 1e-11 * np.abs(want['mesh_back']).max()
    p = wants[0]['paths']
    assert p['single_y'] == (shape[0] == 1) and not p['single_x']
    if (bw, bh) in ((13, 65), (65, 13)):
        r = B.background(frames[0], mask=B.unequal_mask(h, w), bw=bw, bh=bh, maps=False)
        assert r['status'] == 0 and r['paths']['bad'] >= 3 and r['paths']['filled'] == r['paths']['bad']


def test_precision_figures():
    """Float32 steps against all-float64 over the test scenes, in units of each frame's globalrms: the figures of the
    DESIGN.md section, and four times them the parity bounds of the device tests."""
    fig = B.precision_figures()
    print('float32 against float64: mesh back %.3g, mesh rms %.3g of globalrms; map %.3g of the largest mesh value'
          % (fig['mesh_back'], fig['mesh_rms'], fig['map']))
    # a handful of float32 roundings of numbers of the size of the sky (some 100) over an rms of some 3
    assert 0 < fig['mesh_back'] < 1e-3 and 0 < fig['mesh_rms'] < 1e-3 and 0 < fig['map'] < 2e-5


def _declared(name):
    text = open(os.path.join(ROOT, 'include', 'lcmi.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', text)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def test_supported_needs_no_device_and_prototypes_match_the_header():
    from lightcurver_amd import _lib
    lib = _lib.lib()
    s = lib.lc_background_supported
    assert s(2048, 2048, 204, 204, 3, 3) == 1 and s(100, 100, 10, 10, 1, 1) == 1 and s(1, 1, 1, 1, 3, 3) == 1
    assert s(33, 50, 1, 1, 3, 3) == 1
    assert s(100, 100, 10, 10, 5, 5) == 0 and s(100, 100, 10, 10, 3, 1) == 0 and s(100, 100, 10, 10, 2, 2) == 0
    assert s(100, 100, 0, 10, 3, 3) == 0 and s(0, 100, 10, 10, 3, 3) == 0
    assert s(100, 257, 1, 100, 3, 3) == 0            # 257 meshes along x
    assert s(64, 64, 1, 1, 3, 3) == 0                # 4096 meshes in all
    assert s(256, 8, 1, 1, 3, 3) == 1 and s(8, 256, 1, 1, 3, 3) == 1
    ctype = {'int': ctypes.c_int, 'float *': _lib.fp, 'const float *': _lib.fp, 'lc_ctx *': _lib.vp,
             'const uint8_t *': ctypes.POINTER(ctypes.c_uint8), 'int32_t *': _lib.ip,
             'const lc_background_cfg *': ctypes.POINTER(_lib.BackgroundCfg)}
    for name in ('lc_background_supported', 'lc_background_frames', 'lc_background_map'):
        args = _declared(name)
        res, proto = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(proto) == len(args), name
        for a, p in zip(args, proto):
            kind = re.sub(r'\w+$', '', a).strip()
            assert ctype[kind] is p, (name, a)
    assert [f for f, _ in _lib.BackgroundCfg._fields_] == ['bw', 'bh', 'fw', 'fh', 'fthresh']
    assert ctypes.sizeof(_lib.BackgroundCfg) == 20


def test_python_refuses_what_is_not_built():
    from lightcurver_amd import sep
    from lightcurver_amd.processes.background_estimation import subtract_background
    img = np.zeros((40, 40), np.float32)
    with pytest.raises(NotImplementedError):
        sep.Background(img, bw=8, bh=8, fw=5, fh=5)
    with pytest.raises(NotImplementedError):
        sep.Background(img, bw=8, bh=8, fthresh=1.0)
    with pytest.raises(NotImplementedError):
        sep.Background(np.zeros((64, 64), np.float32), bw=1, bh=1)
    with pytest.raises(NotImplementedError, match='mask='):
        subtract_background(img, mask_sources_first=True)
