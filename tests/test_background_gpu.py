"""GPU parity of the sky background of whole frames (lc_background_frames, lc_background_map; DESIGN.md §5 "Sky
background") against the NumPy restatement of the SPEC (tests/_background.py), with square meshes and with bw != bh.

Bounds.  Mesh values and global values: 4 x the float32-against-float64 figure of the restatement over the test scenes
(``_background.precision_figures``, measured again here, not a number written down), in units of the frame's globalrms:
the project's standing margin for reassociated sums.  The map is judged alone, against the float64 spline through the
device's own mesh values, at the project's 2e-5 of the largest |mesh value|; sub + back gives the data back to one
rounding."""
import ctypes as C

import numpy as np
import pytest

from tests import _background as B

pytestmark = pytest.mark.gpu

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)


def _sides(box):
    return tuple(box) if isinstance(box, tuple) else (box, box)


def _call(ctx, frames, box, mask=None, fw=3, want=('sub', 'back', 'mesh_back', 'mesh_rms', 'status')):
    """lc_background_frames through ctypes, with the outputs of ``want`` and null pointers for the others.  box: the
    side of square meshes, or (bw, bh)."""
    from lightcurver_amd import _lib
    d = _lib.f32(frames)
    K, h, w = d.shape
    bw, bh = _sides(box)
    ny, nx = B.grid(h, w, bw, bh)
    out = dict(sub=np.full(d.shape, -7.0, np.float32), back=np.full(d.shape, -7.0, np.float32),
               mesh_back=np.full((K, ny, nx), -7.0, np.float32), mesh_rms=np.full((K, ny, nx), -7.0, np.float32),
               status=np.full(K, 99, np.int32))
    out = {k: v for k, v in out.items() if k in want}
    gb, gr = np.empty(K, np.float32), np.empty(K, np.float32)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    cfg = _lib.BackgroundCfg(bw, bh, fw, fw, 0.0)
    ms = C.c_float()
    st = out.get('status')
    ctx.check(_lib.lib().lc_background_frames(
        ctx.h, K, h, w, _lib.ptr(d), None if m is None else m.ctypes.data_as(_u8p), C.byref(cfg), _lib.ptr(out.get('sub')),
        _lib.ptr(out.get('back')), _lib.ptr(out.get('mesh_back')), _lib.ptr(out.get('mesh_rms')), _lib.ptr(gb),
        _lib.ptr(gr), None if st is None else st.ctypes.data_as(_i32p), C.byref(ms)), 'lc_background_frames')
    out.update(globalback=gb, globalrms=gr, kernel_ms=ms.value)
    return out


@pytest.fixture(scope='module')
def bounds():
    fig = B.precision_figures()
    return dict(back=4.0 * fig['mesh_back'], rms=4.0 * fig['mesh_rms'])


def _check_meshes(got, k, want, bounds, what=''):
    """Frame k of the device result against the restatement of that frame."""
    unit = float(want['globalrms'])
    assert got['status'][k] == want['status'], what
    if want['status'] != 0:
        for key in ('mesh_back', 'mesh_rms', 'globalback', 'globalrms'):
            assert np.isnan(got[key][k]).all(), (what, key)
        return
    db = np.abs(got['mesh_back'][k].astype(np.float64) - want['mesh_back']).max()
    dr = np.abs(got['mesh_rms'][k].astype(np.float64) - want['mesh_rms']).max()
    dgb, dgr = abs(float(got['globalback'][k]) - want['globalback']), abs(float(got['globalrms'][k]) - want['globalrms'])
    print(f'{what} frame {k}: mesh back {db:.3g}, mesh rms {dr:.3g}, globalback {dgb:.3g}, globalrms {dgr:.3g} '
          f'(globalrms {unit:.4g}; bounds {bounds["back"] * unit:.3g}, {bounds["rms"] * unit:.3g})')
    assert np.isfinite(got['mesh_back'][k]).all() and np.isfinite(got['mesh_rms'][k]).all(), what
    assert db <= bounds['back'] * unit and dgb <= bounds['back'] * unit, what
    assert dr <= bounds['rms'] * unit and dgr <= bounds['rms'] * unit, what


def _check_map(got, k, frame, box, what=''):
    """back and sub of frame k against the float64 spline through the device's own mesh values."""
    h, w = frame.shape
    mesh = got['mesh_back'][k]
    want = B.spline_map(mesh, h, w, *_sides(box), np.float64)
    scale = np.abs(mesh).max()
    err = np.abs(got['back'][k] - want).max()
    print(f'{what} frame {k}: map {err / max(scale, 1e-300):.3g} of the largest mesh value')
    assert err <= 2e-5 * scale, what
    assert np.array_equal(got['sub'][k], frame - got['back'][k]), what
    # sub + back == D to the one rounding of the subtraction (the sum taken exactly)
    exact = got['sub'][k].astype(np.float64) + got['back'][k].astype(np.float64) - frame.astype(np.float64)
    assert np.all(np.abs(exact) <= 0.5 * np.spacing(np.abs(got['sub'][k])).astype(np.float64)), what


def _frames(h, w, K, seed, nstars):
    return np.stack([B.scene(h, w, nstars, seed + k) for k in range(K)])


# (h, w, box, K, nstars, seed, the path the case is there for)
CASES = [
    (130, 195, 65, 2, 40, 3, lambda p: p['capped'] > 0),
    (130, 195, 13, 3, 40, 3, lambda p: p['mode'] > 0 and p['median'] > 0),
    (67, 45, 8, 2, 6, 6, lambda p: p['partial_x'] and p['partial_y']),
    (16, 64, 16, 1, 2, 8, lambda p: p['single_y'] and not p['single_x']),
    (12, 12, 12, 1, 0, 9, lambda p: p['single_x'] and p['single_y']),
]


def test_the_references_test_image(ctx, bounds):
    frame = B.reference_test_frame()
    got = _call(ctx, frame[None], 10)
    want = B.background(frame, bw=10, bh=10, maps=False)
    assert want['paths']['mode'] + want['paths']['median'] == 100
    _check_meshes(got, 0, want, bounds, 'reference frame')
    _check_map(got, 0, frame, 10, 'reference frame')
    assert abs(got['globalback'][0] - 100.0) < 10.0 and abs(got['globalrms'][0] - 5.0) < 0.5


@pytest.mark.parametrize('h,w,box,K,nstars,seed,path', CASES)
def test_parity_with_the_restatement(ctx, bounds, h, w, box, K, nstars, seed, path):
    frames = _frames(h, w, K, seed, nstars)
    got = _call(ctx, frames, box)
    for k in range(K):
        want = B.background(frames[k], bw=box, bh=box, maps=False)
        if k == 0:
            assert path(want['paths']), want['paths']
        _check_meshes(got, k, want, bounds, f'{h} x {w} box {box}')
        _check_map(got, k, frames[k], box, f'{h} x {w} box {box}')
    if K > 1:
        assert not np.array_equal(frames[0], frames[1])
        # a frame of the batch is its own K = 1 call, bit for bit
        k = K - 1
        one = _call(ctx, frames[k:k + 1], box)
        for key in ('sub', 'back', 'mesh_back', 'mesh_rms', 'globalback', 'globalrms', 'status'):
            assert np.array_equal(one[key][0], got[key][k]), key


@pytest.mark.parametrize('case', B.UNEQUAL_CASES)
def test_unequal_mesh_sides(ctx, bounds, case):
    """bw != bh through lc_background_frames, lc_background_map alone and the sep mirror.  With the sides swapped, or one
    used for both, the grid has another shape and the global values are far outside the bounds
    (tests/test_background_cpu.py asserts that), so a kernel that did either fails here."""
    from lightcurver_amd import sep
    h, w, bw, bh, nstars, seed, K, shape = case
    frames, wants = B.unequal_wanted(case)
    got = _call(ctx, frames, (bw, bh))
    assert got['mesh_back'].shape == got['mesh_rms'].shape == (K,) + shape
    for k in range(K):
        _check_meshes(got, k, wants[k], bounds, f'{h} x {w} in {bw} x {bh}')
        _check_map(got, k, frames[k], (bw, bh), f'{h} x {w} in {bw} x {bh}')
    if K > 1:
        one = _call(ctx, frames[K - 1:], (bw, bh))
        for key in ('sub', 'back', 'mesh_back', 'mesh_rms', 'globalback', 'globalrms', 'status'):
            assert np.array_equal(one[key][0], got[key][K - 1]), key
    # lc_background_map on its own, through mesh values that are not the device's: the restatement's, back and rms
    for key in ('mesh_back', 'mesh_rms'):
        mesh = np.stack([wt[key] for wt in wants]).astype(np.float32)
        maps = sep.background_map(mesh, h, w, bw, bh, ctx=ctx)
        assert maps.shape == (K, h, w) and maps.dtype == np.float32
        for k in range(K):
            err = np.abs(maps[k] - B.spline_map(mesh[k], h, w, bw, bh, np.float64)).max()
            print(f'{h} x {w} in {bw} x {bh}: lc_background_map of {key} {err / np.abs(mesh[k]).max():.3g} of the largest value')
            assert err <= 2e-5 * np.abs(mesh[k]).max(), key
    # the sep mirror
    bkg = sep.Background(frames[0], bw=bw, bh=bh, ctx=ctx)
    assert bkg.mesh_back.shape == (1,) + shape and np.array_equal(bkg.mesh_back[0], got['mesh_back'][0])
    assert bkg.globalback == float(got['globalback'][0]) and bkg.globalrms == float(got['globalrms'][0])
    assert np.array_equal(bkg.back(), got['back'][0]) and np.array_equal(frames[0] - bkg, got['sub'][0])
    want_rms = B.spline_map(got['mesh_rms'][0], h, w, bw, bh, np.float64)
    assert bkg.rms().shape == (h, w) and np.abs(bkg.rms() - want_rms).max() <= 2e-5 * got['mesh_rms'][0].max()
    if K > 1:
        stack = sep.Background(frames, bw=bw, bh=bh, ctx=ctx)
        assert np.array_equal(stack.globalback, got['globalback']) and np.array_equal(frames - stack, got['sub'])
    if (bw, bh) in ((13, 65), (65, 13)):        # the masked case: whole meshes bad and filled, scattered pixels
        mask = B.unequal_mask(h, w)
        want = B.background(frames[0], mask=mask, bw=bw, bh=bh, maps=False)
        assert want['paths']['filled'] >= 3
        masked = _call(ctx, frames[:1], (bw, bh), mask=mask[None])
        _check_meshes(masked, 0, want, bounds, f'masked, {bw} x {bh}')
        _check_map(masked, 0, frames[0], (bw, bh), f'masked, {bw} x {bh}')
        assert not np.array_equal(masked['mesh_back'], got['mesh_back'][:1])
        mirror = sep.Background(frames[0], mask=mask, bw=bw, bh=bh, ctx=ctx)
        assert np.array_equal(mirror.mesh_back[0], masked['mesh_back'][0])


def test_one_pixel_meshes_constant_and_integer_frames(ctx, bounds):
    rng = np.random.default_rng(21)
    # one-pixel meshes: one level in every mesh, no round of the mode, 1650 meshes
    f = B.scene(33, 50, 3, 22)
    want = B.background(f, bw=1, bh=1, maps=False)
    assert want['paths']['single'] == 33 * 50
    got = _call(ctx, f[None], 1)
    _check_meshes(got, 0, want, bounds, 'one-pixel meshes')
    _check_map(got, 0, f, 1, 'one-pixel meshes')
    # without the filter every mesh is its pixel, its rms 0, the map the frame and sub 0 to the map's bound
    raw = _call(ctx, f[None], 1, fw=1)
    assert np.array_equal(raw['mesh_back'][0], f) and np.all(raw['mesh_rms'][0] == 0) and raw['globalrms'][0] == 0
    assert raw['globalback'][0] == np.float32(B.sorted_median(np.sort(f.ravel())))
    assert np.abs(raw['sub'][0]).max() <= 2e-5 * np.abs(f).max()
    # a constant frame and a frame of small integers (pixels on bin edges, ties in the walk): exact sums, so equal values
    const = np.full((40, 56), 7.0, np.float32)
    ints = rng.integers(0, 4, (40, 56)).astype(np.float32)
    frames = np.stack([const, ints])
    got = _call(ctx, frames, 8)
    for k, name in enumerate(('constant', 'small integers')):
        want = B.background(frames[k], bw=8, bh=8, maps=False)
        _check_meshes(got, k, want, bounds, name)
        assert np.array_equal(got['mesh_back'][k], want['mesh_back']) and np.array_equal(got['mesh_rms'][k], want['mesh_rms'])
        _check_map(got, k, frames[k], 8, name)
    assert B.background(const, bw=8, bh=8, maps=False)['paths']['mean'] == 35
    assert got['globalrms'][0] == 0 and got['globalback'][0] == 7.0


def test_a_one_pixel_corner_mesh_is_its_pixel(ctx, bounds):
    """h % box = w % box = 1, as 2041 x 2041 pixels have at n_boxes = 10: the corner mesh holds one pixel, one level, and no
    round of the mode runs.  The mesh is that pixel, and the corner of the map stays with the sky."""
    frame, box, sky, sigma = B.one_pixel_corner_frame()
    want = B.background(frame, bw=box, bh=box, maps=False)
    assert want['paths']['single'] == 1
    got = _call(ctx, frame[None], box)
    _check_meshes(got, 0, want, bounds, 'corner mesh')
    _check_map(got, 0, frame, box, 'corner mesh')
    assert got['mesh_back'][0, -1, -1] == frame[-1, -1]          # the filter leaves a corner alone
    # every mesh within five sigma of one pixel (the weakest mesh is one pixel) of the sky, and the map's corner with it
    assert np.abs(got['mesh_back'][0] - sky).max() < 5 * sigma
    assert np.abs(got['back'][0][-box:, -box:] - sky).max() < 5 * sigma
    assert abs(got['globalback'][0] - sky) < 0.1 * sky and abs(got['globalrms'][0] - sigma) < 0.1 * sigma


def test_masked_meshes_and_a_frame_without_a_good_mesh(ctx, bounds):
    frames = _frames(130, 195, 3, 3, 40)
    mask = np.zeros(frames.shape, np.uint8)
    mask[0, :30, :50] = 1                    # whole meshes bad: filled from their neighbours
    for x0, n in ((104, 85), (117, 84)):     # of 169 pixels 84 good: bad; 85 good: kept
        blk = np.zeros(169, np.uint8)
        blk[:n] = 200
        mask[0, 52:65, x0:x0 + 13] = blk.reshape(13, 13)
    mask[1] = 1                              # not one good mesh
    got = _call(ctx, frames, 13, mask=mask)
    wants = [B.background(frames[k], mask=mask[k], bw=13, bh=13, maps=False) for k in range(3)]
    assert np.isnan(wants[0]['raw_back'][4, 8]) and np.isfinite(wants[0]['raw_back'][4, 9])
    assert wants[0]['paths']['filled'] >= 7 and wants[1]['status'] == B.LC_ERR_NONFINITE and wants[2]['paths']['bad'] == 0
    for k in range(3):
        _check_meshes(got, k, wants[k], bounds, 'masked')
    assert got['status'].tolist() == [0, B.LC_ERR_NONFINITE, 0]
    assert np.isnan(got['sub'][1]).all() and np.isnan(got['back'][1]).all()
    _check_map(got, 0, frames[0], 13, 'masked')
    # the frames beside the bad one are what they are alone
    alone = _call(ctx, frames[2:3], 13)
    for key in ('sub', 'back', 'mesh_back', 'mesh_rms', 'globalback', 'globalrms'):
        assert np.array_equal(alone[key][0], got[key][2]), key


def test_non_finite_pixels_are_masked_pixels(ctx):
    f = B.scene(67, 45, 6, 6)
    rng = np.random.default_rng(31)
    holes = rng.random(f.shape) < 0.03
    holes[:8, :8] = True                      # a whole mesh of them
    g = f.copy()
    g[holes] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(holes.sum()))
    assert np.isnan(g).any() and np.isposinf(g).any() and np.isneginf(g).any()
    a = _call(ctx, g[None], 8)
    b = _call(ctx, f[None], 8, mask=holes[None])
    for key in ('mesh_back', 'mesh_rms', 'globalback', 'globalrms', 'back', 'status'):
        assert np.array_equal(a[key], b[key]), key
    assert np.isfinite(a['mesh_back']).all() and np.isfinite(a['back']).all()
    assert np.array_equal(a['sub'][0][~holes], b['sub'][0][~holes]) and not np.isfinite(a['sub'][0][holes]).any()


def test_a_large_frame(ctx, bounds):
    """1000 x 1500 pixels in meshes of 100: 250 workgroups of the map, every mesh at the level cap."""
    f = B.scene(1000, 1500, 20, 41)
    got = _call(ctx, f[None], 100)
    want = B.background(f, bw=100, bh=100, maps=False)
    assert want['paths']['capped'] == 150
    _check_meshes(got, 0, want, bounds, '1000 x 1500')
    _check_map(got, 0, f, 100, '1000 x 1500')


def test_optional_outputs(ctx):
    frames = _frames(67, 45, 2, 6, 6)
    full = _call(ctx, frames, 8)
    keys = ('sub', 'back', 'mesh_back', 'mesh_rms', 'status')
    for bits in range(1 << len(keys)):
        want = tuple(k for i, k in enumerate(keys) if bits >> i & 1)
        part = _call(ctx, frames, 8, want=want)
        for k in want + ('globalback', 'globalrms'):
            assert np.array_equal(part[k], full[k]), (want, k)


def test_filter_sizes_and_argument_checks(ctx, bounds):
    from lightcurver_amd import _lib
    f = B.scene(67, 45, 6, 6)
    got = _call(ctx, f[None], 8, fw=1)
    _check_meshes(got, 0, B.background(f, bw=8, bh=8, fw=1, fh=1, maps=False), bounds, 'no filter')
    assert not np.array_equal(got['mesh_back'], _call(ctx, f[None], 8)['mesh_back'])
    lib, d = _lib.lib(), _lib.f32(f)
    gb, gr = np.empty(1, np.float32), np.empty(1, np.float32)

    def rc(K=1, h=67, w=45, cfg=(8, 8, 3, 3, 0.0)):
        c = _lib.BackgroundCfg(*cfg)
        return lib.lc_background_frames(ctx.h, K, h, w, _lib.ptr(d), None, C.byref(c), None, None, None, None,
                                        _lib.ptr(gb), _lib.ptr(gr), None, None)
    assert rc() == 0
    assert rc(K=0) == -1 and rc(h=0) == -1 and rc(cfg=(0, 8, 3, 3, 0.0)) == -1 and rc(cfg=(8, 8, 3, 3, float('nan'))) == -1
    assert rc(cfg=(8, 8, 5, 5, 0.0)) == -3 and rc(cfg=(8, 8, 3, 1, 0.0)) == -3 and rc(cfg=(8, 8, 3, 3, 0.5)) == -3
    assert rc(cfg=(1, 1, 3, 3, 0.0)) == -3          # 67 x 45 one-pixel meshes: more than 2048


def test_python_mirror_of_sep(ctx):
    from lightcurver_amd import sep
    from lightcurver_amd.processes.background_estimation import subtract_background, subtract_background_batch
    frames = _frames(130, 195, 3, 3, 40)
    direct = _call(ctx, frames, 13)
    bkg = sep.Background(frames[0], bw=13, bh=13, ctx=ctx)
    assert isinstance(bkg.globalback, float) and bkg.globalrms == float(direct['globalrms'][0])
    assert np.array_equal(frames[0] - bkg, direct['sub'][0])            # image - bkg as the reference writes it
    assert np.array_equal(bkg.back(), direct['back'][0]) and np.array_equal(np.asarray(bkg), direct['back'][0])
    assert (frames[0].astype(np.float64) - bkg).dtype == np.float64
    want_rms = B.spline_map(direct['mesh_rms'][0], 130, 195, 13, 13, np.float64)
    assert bkg.rms().shape == (130, 195) and np.abs(bkg.rms() - want_rms).max() <= 2e-5 * direct['mesh_rms'][0].max()
    copy = frames[0].copy()
    bkg.subfrom(copy)
    assert np.array_equal(copy, direct['sub'][0])
    m = np.zeros(frames[0].shape)
    m[:30, :50] = 0.7
    assert sep.Background(frames[0], mask=m, maskthresh=0.8, bw=13, bh=13, ctx=ctx).globalback == bkg.globalback
    masked = sep.Background(frames[0], mask=m, maskthresh=0.5, bw=13, bh=13, ctx=ctx)
    assert np.array_equal(masked.mesh_back[0], _call(ctx, frames[:1], 13, mask=(m > 0.5)[None])['mesh_back'][0])
    # a stack is one call and equals its per-frame calls
    stack = sep.Background(frames, bw=13, bh=13, ctx=ctx)
    assert stack.globalrms.shape == (3,) and np.array_equal(stack.globalrms, direct['globalrms'])
    assert np.array_equal(frames - stack, direct['sub'])
    # the reference's step function: box = min(shape) // n_boxes
    sub, b = subtract_background(frames[1], n_boxes=10, ctx=ctx)
    assert np.array_equal(sub, direct['sub'][1]) and b.globalrms == float(direct['globalrms'][1])
    assert np.array_equal(b.back(), direct['back'][1])
    # mixed shapes: one call per shape, results in the order of the input
    small = B.scene(67, 45, 6, 6)
    subs, bkgs = subtract_background_batch([frames[0], small, frames[2]], n_boxes=10, ctx=ctx)
    assert np.array_equal(subs[0], direct['sub'][0]) and np.array_equal(subs[2], direct['sub'][2])
    assert np.array_equal(subs[1], subtract_background(small, ctx=ctx)[0]) and subs[1].shape == (67, 45)
    assert bkgs[2].globalback == float(direct['globalback'][2])


def test_chain_into_the_noise_maps_of_the_stamps(ctx):
    """subtract_background -> bkg.globalrms -> prepare_stamps(rms=, exptime=) on stamps cut from the subtracted frame,
    against the reference's formula (cutout_making.py:43-51) in NumPy with the same rms, at the bound of
    tests/test_prep_gpu.py for the noise map (2e-6)."""
    from lightcurver_amd.processes.background_estimation import subtract_background
    from lightcurver_amd.processes.preprocessing import prepare_stamps
    frame = B.scene(130, 195, 40, 3)
    sub, bkg = subtract_background(frame, ctx=ctx)
    exptime = 60.0
    corners = [(5, 7), (40, 100), (90, 150), (98, 163)]
    stamps = np.stack([sub[y:y + 32, x:x + 32] for y, x in corners])
    out = prepare_stamps(stamps, rms=np.full(4, bkg.globalrms, np.float32), exptime=np.full(4, exptime, np.float32), ctx=ctx)
    electrons = exptime * stamps.astype(np.float64)
    noise = ((exptime * float(np.float32(bkg.globalrms))) ** 2 + np.abs(electrons)) ** 0.5
    noise[noise < 1e-7] = 1e-7
    want = noise.astype(np.float32) / exptime
    assert np.abs(out['noisemap'] - want).max() <= 2e-6 * np.abs(want).max()
    assert np.array_equal(out['data'], stamps)
