"""GPU parity of the resident frame set and the stamp cutting (lc_frames_*, lightcurver_amd.frames.FrameSet; DESIGN.md
section 5 "Stamp cutting").  The cut and n_inside have the bits of the NumPy restatement (tests/_cutout.py); the noise map
has the bits of lc_prepare_stamps on the same stamps and lies within 2e-6 (the bound of tests/test_prep_gpu.py) of the
float64 formula; the mask is that of mask_cutout_batch on the same stamps and noise maps; lc_frames_import gives every
output of lc_import_frames.  Everything refused is refused on the host."""
import ctypes as C

import numpy as np
import pytest

from oracle import prep as op

from . import _cutout as R
from . import _extract as E

pytestmark = pytest.mark.gpu

H, W = 40, 56                  # not square, the width no multiple of 64
SIZES = (8, 17, 32, 128)
EXPTIMES = np.array([30.0, 12.5, 300.0], np.float32)
RMS = np.array([3.0, 5.5, 0.0], np.float32)


def _make_frames():
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = rng.normal(0.0, 4.0, (3, H, W))                       # negative pixels throughout
    for k, (cy, cx) in enumerate([(12.3, 14.8), (25.1, 40.2), (30.7, 9.9)]):
        frames[k] += 900.0 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * 1.8 ** 2))
    frames[0, 20, 30] += 4000.0                                    # single hot pixels: cosmics
    frames[1, 8, 12] += 6000.0
    frames[1, 9, 12] += 5000.0
    frames[0, :, 22] += 700.0                                      # a bad column and a bad row
    frames[1, 17, :] -= 600.0
    frames[2, 4:22, 30:52] = 0.0                                   # all zero with rms 0: the 1e-7 clamp
    frames = frames.astype(np.float32)
    frames[0, 5, 7] = frames[1, 39, 55] = frames[2, 0, 0] = frames[2, 21, 3] = np.nan
    return frames


@pytest.fixture(scope='module')
def frames():
    return _make_frames()


@pytest.fixture(scope='module')
def frameset(ctx, frames):
    from lightcurver_amd.frames import FrameSet
    with FrameSet(frames, ctx) as fs:
        yield fs


def _origins(n):
    """[(frame, x0, y0)] by construction, the frames out of order."""
    big = n > min(H, W)
    o = [(-3, -2), (W - n + 3, -2), (-3, H - n + 2), (W - n + 3, H - n + 2),      # the four corners
         (W - 1, H - 1), (-(n - 1), -(n - 1)),                                     # a single pixel inside
         (W - 1, -(n - 1)), (-(n - 1), H - 1)]
    if big:
        o += [(-30, -40), (-36, -44), (-72, -88)]                                  # larger than the frame on all sides
    else:
        o += [(5, 3), (5, 3),                                                      # inside, twice
              (0, 4), (W - n, 4), (6, 0), (6, H - n),                              # flush with each border
              (-3, 4), (W - n + 3, 4), (6, -2), (6, H - n + 2),                    # over each edge
              (0, 0), (W - n, H - n)]
    order = [2, 0, 1, 1, 0, 2, 2, 1]
    out = [(order[i % len(order)], x0, y0) for i, (x0, y0) in enumerate(o)]
    if big:
        out += [out[8]]                                                            # two identical stamps
    else:
        out[9] = out[8]
        out += [(2, 33, 6)]                                                        # in the all-zero region of frame 2
    return out


def _classes(stamps, n):
    c = set()
    for s, (k, x0, y0) in enumerate(stamps):
        x1, y1 = x0 + n, y0 + n
        in_x, in_y = 0 <= x0 and x1 <= W, 0 <= y0 and y1 <= H
        if 0 < x0 and x1 < W and 0 < y0 and y1 < H:
            c.add('inside')
        if in_y and in_x:
            c |= {name for name, hit in (('flush left', x0 == 0), ('flush right', x1 == W), ('flush bottom', y0 == 0),
                                         ('flush top', y1 == H)) if hit}
        if in_y:
            c |= {name for name, hit in (('over left', x0 < 0 and x1 < W), ('over right', x0 > 0 and x1 > W)) if hit}
        if in_x:
            c |= {name for name, hit in (('over bottom', y0 < 0 and y1 < H), ('over top', y0 > 0 and y1 > H)) if hit}
        for name, hit in (('corner bl', x0 < 0 and y0 < 0), ('corner br', x1 > W and y0 < 0), ('corner tl', x0 < 0 and y1 > H),
                          ('corner tr', x1 > W and y1 > H)):
            if hit and not (x0 < 0 and x1 > W) and not (y0 < 0 and y1 > H):
                c.add(name)
        if x0 < 0 and x1 > W and y0 < 0 and y1 > H:
            c.add('larger')
        if (min(W, x1) - max(0, x0)) * (min(H, y1) - max(0, y0)) == 1:
            c.add('one pixel high' if x0 > 0 else 'one pixel low')
        if any(stamps[q] == stamps[s] for q in range(s)):
            c.add('identical')
    frames_used = [k for k, _, _ in stamps]
    if any(a > b for a, b in zip(frames_used, frames_used[1:])):
        c.add('out of order')
    return c


ALWAYS = {'one pixel high', 'one pixel low', 'identical', 'out of order'}
SMALL = ALWAYS | {'inside', 'flush left', 'flush right', 'flush bottom', 'flush top', 'over left', 'over right',
                  'over bottom', 'over top', 'corner bl', 'corner br', 'corner tl', 'corner tr'}


def _positions(stamps, n):
    """positions whose stamps start at the given origins: ceil(x0 + n / 2 - n / 2) = x0 exactly"""
    return np.array([k for k, _, _ in stamps]), np.array([[x0 + n / 2, y0 + n / 2] for _, x0, y0 in stamps], np.float64)


@pytest.fixture(scope='module')
def cuts(frameset):
    """One cut per size with both switches off, shared by the tests below and left unchanged."""
    out = {}
    for n in SIZES:
        stamps = _origins(n)
        index, pos = _positions(stamps, n)
        out[n] = (stamps, index, pos, frameset.cut_stamps(index, pos, n, exptimes=EXPTIMES, background_rms=RMS))
    return out


@pytest.mark.parametrize('n', SIZES)
def test_every_overlap_class_is_present(n):
    classes = _classes(_origins(n), n)
    need = SMALL if n <= min(H, W) else ALWAYS | {'larger'}
    assert need <= classes, sorted(need - classes)


@pytest.mark.parametrize('n', SIZES)
def test_cut_and_n_inside_have_the_bits_of_the_restatement(frames, cuts, n):
    stamps, index, pos, got = cuts[n]
    want = R.cut_stamps(frames, index, pos, n, EXPTIMES, RMS)
    assert [tuple(o) for o in got['origin']] == [(x0, y0) for _, x0, y0 in stamps]
    assert got['data'].dtype == np.float32 and R.same_bits(np.isnan(got['data']), np.isnan(want['data']))
    assert R.same_bits(got['data'], want['data'])
    assert np.array_equal(got['n_inside'], want['n_inside'])
    assert np.array_equal(got['n_inside'], (~np.isnan(R.cut(np.zeros_like(frames), index, got['origin'][:, 0],
                                                            got['origin'][:, 1], n)[0])).sum(axis=(1, 2)))
    assert np.array_equal(got['origin'], want['origin']) and np.array_equal(got['center_original'], want['center_original'])
    assert got['mask'].dtype == bool and not got['mask'].any()          # both switches off


@pytest.mark.parametrize('n', SIZES)
def test_noise_map(ctx, cuts, n):
    from lightcurver_amd.processes.preprocessing import prepare_stamps
    stamps, index, pos, got = cuts[n]
    dev = prepare_stamps(got['data'], rms=RMS[index], exptime=EXPTIMES[index], ctx=ctx, want=('noisemap',))['noisemap']
    # prepare_stamps cleans the pixels that are NaN in both planes (noise 1.0); the cut keeps them NaN
    both_nan = np.isnan(got['data'])
    assert np.array_equal(np.isnan(got['noisemap']), both_nan) and (dev[both_nan] == 1.0).all()
    assert R.same_bits(got['noisemap'][~both_nan], dev[~both_nan])
    assert R.same_bits(got['noisemap'], R.noisemap(got['data'], RMS[index], EXPTIMES[index]))
    R.close(got['noisemap'], op.noisemap_from_rms(got['data'], RMS[index], EXPTIMES[index]), 2e-6)
    clamp = (got['data'] == 0.0) & (index == 2)[:, None, None]          # the all-zero region of the frame with rms 0
    if n <= min(H, W):
        assert clamp.any()
    assert (got['noisemap'][clamp] == np.float32(1e-7) / EXPTIMES[2]).all()


@pytest.mark.parametrize('n', SIZES)
def test_masks_are_those_of_mask_cutout_batch(ctx, frameset, cuts, n):
    from lightcurver_amd.processes.cutout_making import mask_cutout_batch
    stamps, index, pos, plain = cuts[n]
    params = dict(sigclip=4.0, objlim=4.0)
    seen = {}
    for columns, cosmics in ((True, False), (False, True), (True, True)):
        got = frameset.cut_stamps(index, pos, n, exptimes=EXPTIMES, background_rms=RMS, do_mask_bad_columns=columns,
                                  do_mask_cosmics=cosmics, cosmics_masking_params=params)
        assert R.same_bits(got['data'], plain['data']) and R.same_bits(got['noisemap'], plain['noisemap'])
        want = mask_cutout_batch(got['data'], got['noisemap'], columns, cosmics, params, ctx=ctx)
        assert got['mask'].dtype == bool and np.array_equal(got['mask'], want)
        seen[columns, cosmics] = got['mask']
    assert np.array_equal(seen[True, True], seen[True, False] | seen[False, True])
    assert seen[True, False].any() and seen[False, True].any()
    assert not np.array_equal(seen[True, False], seen[False, True])


def _scenes():
    return np.stack([E.fast_scene(333, 257, 40, 60 + k)[0] + np.float32(100.0 + 20 * k) for k in range(3)])


def _same_import(a, b, keys):
    for key in keys:
        assert R.same_bits(a[key], b[key]), key
    assert a['box'] == b['box'] and len(a['objects']) == len(b['objects'])
    for x, y in zip(a['objects'], b['objects']):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


IMPORT_KEYS = ('sub', 'mesh_back', 'mesh_rms', 'globalback', 'globalrms', 'status', 'nobj', 'ex_status')


@pytest.mark.parametrize('mask_sources_first', [False, True])
def test_import_on_the_resident_planes(ctx, mask_sources_first):
    from lightcurver_amd import _lib
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.frame_importation import import_frames
    stack = _scenes()
    t = np.array([30.0, 12.5, 60.0], np.float32)
    want = import_frames(stack, t, 10, mask_sources_first, 3, 10, ctx=ctx)
    assert (want['nobj'] > 10).all() and (want['ex_status'] == 0).all()
    with FrameSet(stack, ctx) as fs:
        assert not fs.imported and R.same_bits(fs.planes(), stack) and R.same_bits(fs.planes(1, 1), stack[1:2])
        download = mask_sources_first                      # one case with sub downloaded, one without
        got = fs.import_frames(t, 10, mask_sources_first, 3, 10, download_sub=download)
        assert ('sub' in got) == download
        _same_import(got, want, IMPORT_KEYS if download else IMPORT_KEYS[1:])
        assert fs.imported and R.same_bits(fs.planes(), want['sub']) and R.same_bits(fs.planes(2), want['sub'][2:])
        index = np.array([2, 0, 1, 0])
        pos = np.array([[10.2, 300.0], [128.0, 166.5], [255.0, 2.0], [60.0, 60.0]])
        recorded = fs.cut_stamps(index, pos, 24, do_mask_cosmics=True)
        explicit = fs.cut_stamps(index, pos, 24, exptimes=t, background_rms=want['globalrms'], do_mask_cosmics=True)
        for key in ('data', 'noisemap', 'mask', 'n_inside'):
            assert R.same_bits(recorded[key], explicit[key]), key
        assert R.same_bits(recorded['data'], R.cut_stamps(want['sub'], index, pos, 24, t, want['globalrms'])['data'])
        assert R.same_bits(recorded['noisemap'], R.cut_stamps(want['sub'], index, pos, 24, t, want['globalrms'])['noisemap'])
        with pytest.raises(_lib.LcError):
            fs.import_frames(t, 10, mask_sources_first, 3, 10)
        assert R.same_bits(fs.planes(), want['sub'])


def test_import_runs_again_on_a_full_object_table(ctx):
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.frame_importation import import_frames
    stack = _scenes()
    t = np.array([30.0, 12.5, 60.0], np.float32)
    want = import_frames(stack, t, max_objects=5, ctx=ctx)
    assert (want['nobj'] > 5).all() and (want['ex_status'] == 0).all()
    with FrameSet(stack, ctx) as fs:
        got = fs.import_frames(t, max_objects=5, download_sub=True)
        _same_import(got, want, IMPORT_KEYS)
        assert fs.imported and R.same_bits(fs.planes(), want['sub'])


def test_refusals_happen_on_the_host(ctx, frames):
    from lightcurver_amd import _lib
    from lightcurver_amd.frames import FrameSet
    lib = _lib.lib()
    i32 = lambda *v: np.array(v, np.int32)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    with FrameSet(frames, ctx) as fs:
        with pytest.raises(ValueError):
            fs.cut_stamps([0], [[70.0, 20.0]], 8, exptimes=EXPTIMES, background_rms=RMS)            # no overlap
        with pytest.raises(ValueError):
            fs.cut_stamps([3], [[20.0, 20.0]], 8, exptimes=EXPTIMES, background_rms=RMS)            # frame index
        with pytest.raises(ValueError):
            fs.cut_stamps([-1], [[20.0, 20.0]], 8, exptimes=EXPTIMES, background_rms=RMS)
        with pytest.raises(_lib.LcError):
            fs.cut_stamps([0], [[20.0, 20.0]], 4, exptimes=EXPTIMES, background_rms=RMS, do_mask_cosmics=True)
        with pytest.raises(_lib.LcError):
            fs.cut_stamps([0], [[20.0, 20.0]], 8, exptimes=EXPTIMES)                                 # no rms, not imported
        with pytest.raises(_lib.LcError):
            fs.cut_stamps([0], [[20.0, 20.0]], 8)
        with pytest.raises(ValueError):
            fs.cut_stamps([0], [[20.0, 20.0]], 8, exptimes=[30.0, 0.0, 1.0], background_rms=RMS)
        # the library's own checks, behind the ones of the Python layer
        data = np.full((1, 8, 8), 7.0, np.float32)
        noise = np.full((1, 8, 8), 7.0, np.float32)

        def raw(frame, y0, x0, n=8, t=EXPTIMES, rms=RMS, want_noise=True, out=data):
            return lib.lc_frames_cut_stamps(fs.h, 1, n, p32(i32(frame)), p32(i32(y0)), p32(i32(x0)), _lib.ptr(t), _lib.ptr(rms),
                                            0, 0, None, None, _lib.ptr(out), _lib.ptr(noise) if want_noise else None, None,
                                            None, None)

        bad_t = np.array([30.0, np.inf, 1.0], np.float32)
        for rc in (raw(0, 20, 56), raw(0, 20, -8), raw(0, 40, 20), raw(0, -8, 20), raw(3, 20, 20), raw(-1, 20, 20),
                   raw(0, 20, 20, rms=None), raw(0, 20, 20, t=None), raw(0, 20, 20, t=bad_t), raw(0, 20, 20, n=0),
                   raw(0, 20, 20, out=None)):
            assert rc == -1                                                                          # LC_ERR_INVALID
            assert lib.lc_last_error(ctx.h)
        assert (data == 7.0).all() and (noise == 7.0).all()                                          # nothing was written
        assert raw(0, 20, 20, t=None, rms=None, want_noise=False) == 0                               # data alone needs neither
        assert R.same_bits(data, R.cut(frames, [0], [20], [20], 8)[0])
        # the context and the set are as usable as before
        index, pos = _positions(_origins(17), 17)
        got = fs.cut_stamps(index, pos, 17, exptimes=EXPTIMES, background_rms=RMS)
        assert R.same_bits(got['data'], R.cut_stamps(frames, index, pos, 17, EXPTIMES, RMS)['data'])
    with pytest.raises(_lib.LcError):
        fs.planes()                                                                                  # closed


def test_chain_to_the_psf_stamps(ctx):
    """FrameSet -> extract_all_stamps_of_frames -> read_psf_batch -> prepare_psf_stamps_batched gives the arrays of the
    path that cuts on the host: sub downloaded, NumPy slices, prepare_stamps for the noise, mask_cutout_batch."""
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.io.regions import frames_for_psf_model, read_psf_batch
    from lightcurver_amd.processes.cutout_making import extract_all_stamps_of_frames, mask_cutout_batch
    from lightcurver_amd.processes.frame_importation import import_frames
    from lightcurver_amd.processes.preprocessing import prepare_stamps
    from lightcurver_amd.processes.psf_modelling import prepare_psf_stamps_batched
    stack = _scenes()
    K, h, w = stack.shape
    t = np.array([30.0, 12.5, 60.0], np.float32)
    rng = np.random.default_rng(3)
    roi = np.array([[128.3, 166.1], [128.9, 165.4], [127.6, 166.8]])
    stars = [np.column_stack([rng.uniform(-3, w + 3, 4), rng.uniform(-3, h + 3, 4)]) for _ in range(K)]
    stars[1] = stars[1][:3]
    names = [[f'star{i}' for i in range(len(p))] for p in stars]
    n_roi, n_star = 32, 24
    with FrameSet(stack, ctx) as fs:
        fs.import_frames(t)
        resident = extract_all_stamps_of_frames(fs, roi, stars, names, n_roi, n_star, True, True)
    imp = import_frames(stack, t, ctx=ctx)
    host = {}
    for k in range(K):
        g = host[str(k)] = dict(frame_shape=np.array([h, w]), data={}, noisemap={}, cosmicsmask={}, image_pixel_coordinates={})
        for name, position, n in [('ROI', roi[k], n_roi)] + [(s, p, n_star) for s, p in zip(names[k], stars[k])]:
            (x0, y0), centre = R.cutout_origin(position, n, (h, w))
            d = R.cut(imp['sub'], [k], [x0], [y0], n)[0]
            nm = prepare_stamps(d, rms=imp['globalrms'][k:k + 1], exptime=t[k:k + 1], ctx=ctx, want=('noisemap',))['noisemap']
            nm[np.isnan(d)] = np.nan           # prepare_stamps cleans what is NaN in both planes; the stamps on disk keep it
            g['data'][name], g['noisemap'][name] = d[0], nm[0]
            g['cosmicsmask'][name] = mask_cutout_batch(d, nm, True, True, ctx=ctx)[0]
            g['image_pixel_coordinates'][name] = np.array(centre)
    selection = [(str(k), names[k]) for k in range(K)]
    a, b = read_psf_batch(resident, selection), read_psf_batch(host, selection)
    for key in ('data', 'noisemap', 'cosmics', 'positions', 'frame_shape', 'n_stars'):
        assert R.same_bits(a[key], b[key]), key
    for name in ('ROI',):
        for k in range(K):
            for key in ('data', 'noisemap', 'cosmicsmask', 'image_pixel_coordinates'):
                assert R.same_bits(resident[str(k)][key][name], host[str(k)][key][name]), (k, key)
    pa = prepare_psf_stamps_batched(frames_for_psf_model(a))
    pb = prepare_psf_stamps_batched(frames_for_psf_model(b))
    for x, y in zip(pa, pb):
        for u, v in zip(x, y):
            assert R.same_bits(u, v)
