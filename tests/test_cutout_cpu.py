"""Host side of the stamp cutting (DESIGN.md section 5 "Stamp cutting"): where a stamp lies, against the SPEC's cases; the
restatement's noise against the float64 oracle; lc_cutout_supported; and the layout extract_all_stamps_of_frames returns,
with the device call replaced by the restatement (tests/_cutout.py).  No device is touched."""
import numpy as np
import pytest

from oracle import prep as op

from . import _cutout as R


def _origin(position, size, shape):
    from lightcurver_amd.processes.cutout_making import cutout_origin
    got = cutout_origin(position, size, shape)
    want = R.cutout_origin(position, size, shape)
    assert tuple(got[0]) == want[0] and tuple(got[1]) == want[1]
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    return want


def test_anchor_case_of_the_reference():
    """The reference's tests/test_processes/test_cutout_making.py: 100 x 100, CRPIX = 50 (pixel 49.0), size 10 gives
    columns and rows 44 .. 53."""
    (x0, y0), centre = _origin((49.0, 49.0), 10, (100, 100))
    assert (x0, y0) == (44, 44) and (x0 + 10 - 1, y0 + 10 - 1) == (53, 53)
    assert centre == (48.5, 48.5)


def test_half_integer_positions_and_odd_sizes():
    assert _origin((49.5, 49.5), 10, (100, 100))[0] == (45, 45)
    (x0, y0), centre = _origin((49.0, 49.0), 9, (100, 100))
    assert (x0, x0 + 9 - 1) == (45, 53) and (y0, y0 + 9 - 1) == (45, 53) and centre == (49.0, 49.0)
    assert _origin((49.4999, 49.5001), 9, (100, 100))[0] == (45, 46)
    assert _origin((12.25, 7.75), 1, (40, 56))[0] == (12, 8)


def test_negative_origins_and_partial_centres_on_every_edge():
    h, w, n = 40, 56, 10
    cases = {
        'left': ((1.0, 20.0), (-4, 15), (2.5, 19.5)),          # columns 0 .. 5
        'right': ((54.0, 20.0), (49, 15), (52.0, 19.5)),       # columns 49 .. 55
        'bottom': ((20.0, 0.0), (15, -5), (19.5, 2.0)),        # rows 0 .. 4
        'top': ((20.0, 39.0), (15, 34), (19.5, 36.5)),         # rows 34 .. 39
        'corner': ((-3.0, -2.5), (-8, -7), (0.5, 1.0)),        # columns 0 .. 1, rows 0 .. 2
        'one pixel': ((60.0, 44.0), (55, 39), (55.0, 39.0)),
        'one pixel, low': ((-5.0, -5.0), (-10, -10), None),
    }
    for name, (position, origin, centre) in cases.items():
        if centre is None:
            with pytest.raises(ValueError):
                _origin(position, n, (h, w))
            continue
        got = _origin(position, n, (h, w))
        assert got[0] == origin and got[1] == centre, name
    assert _origin((-4.0, -4.0), n, (h, w)) == ((-9, -9), (0.0, 0.0))


def test_stacked_positions_keep_their_shape():
    from lightcurver_amd.processes.cutout_making import cutout_origin
    pos = np.array([[49.0, 49.0], [49.5, 3.0], [-2.0, 97.25]])
    origin, centre = cutout_origin(pos, 10, (100, 100))
    assert origin.shape == (3, 2) and centre.shape == (3, 2)
    for p, o, c in zip(pos, origin, centre):
        want = R.cutout_origin(p, 10, (100, 100))
        assert tuple(o) == want[0] and tuple(c) == want[1]


@pytest.mark.parametrize('position', [(70.0, 20.0), (-6.0, 20.0), (20.0, 45.0), (20.0, -5.001), (1e30, 0.0)])
def test_no_overlap_raises(position):
    from lightcurver_amd.processes.cutout_making import cutout_origin
    with pytest.raises(ValueError):
        cutout_origin(position, 10, (40, 56))
    with pytest.raises(ValueError):
        R.cutout_origin(position, 10, (40, 56))


@pytest.mark.parametrize('position', [(np.nan, 3.0), (3.0, np.inf), (-np.inf, np.nan)])
def test_non_finite_positions_raise(position):
    from lightcurver_amd.processes.cutout_making import cutout_origin
    with pytest.raises(ValueError):
        cutout_origin(position, 10, (40, 56))
    with pytest.raises(ValueError):
        cutout_origin([(5.0, 5.0), position], 10, (40, 56))


def test_cutout_supported():
    from lightcurver_amd import _lib
    lib = _lib.lib()
    for n in (8, 9, 17, 32, 64, 127, 128):
        assert lib.lc_cutout_supported(n, 1) == 1 and lib.lc_cutout_supported(n, 0) == 1
    for n in (1, 4, 7, 129, 1000, 46340):
        assert lib.lc_cutout_supported(n, 1) == 0 and lib.lc_cutout_supported(n, 0) == 1
    for n in (0, -3, 46341, 2 ** 30):
        assert lib.lc_cutout_supported(n, 1) == 0 and lib.lc_cutout_supported(n, 0) == 0


def _frames():
    rng = np.random.default_rng(5)
    frames = rng.normal(0.0, 4.0, (3, 40, 56)).astype(np.float32)
    frames[0, 3, 4] = np.nan
    frames[2, 10:20, 10:20] = 0.0
    return frames, np.array([30.0, 12.5, 300.0], np.float32), np.array([3.0, 5.5, 0.0], np.float32)


def test_restated_noise_against_the_float64_formula():
    """The float32 steps against oracle.prep.noisemap_from_rms, at the bound tests/test_prep_gpu.py holds the device to."""
    frames, t, rms = _frames()
    index = np.array([0, 1, 2, 2, 0])
    data, inside = R.cut(frames, index, [0, 50, 8, -3, 2], [0, 30, 8, -3, 1], 12)
    assert inside.tolist() == [144, 60, 144, 81, 144]
    assert np.isnan(data[1, :, 6:]).all() and np.isnan(data[1, 10:]).all() and not np.isnan(data[1, :10, :6]).any()
    noise = R.noisemap(data, rms[index], t[index])
    R.close(noise, op.noisemap_from_rms(data, rms[index], t[index]), 2e-6)
    assert np.isnan(noise[0, 3, 4]) and (noise[2, 2:12, 2:12] == np.float32(1e-7) / np.float32(300.0)).all()


class _RestatedFrameSet:
    """FrameSet's shape and cut_stamps, from the restatement; counts the calls."""

    def __init__(self, frames, exptimes, rms):
        self.frames, self.exptimes, self.rms = frames, exptimes, rms
        self.shape = frames.shape
        self.calls = []

    def cut_stamps(self, frame_index, positions_xy, size, exptimes=None, background_rms=None, do_mask_bad_columns=False,
                   do_mask_cosmics=False, cosmics_masking_params=None):
        self.calls.append((len(np.asarray(positions_xy).reshape(-1, 2)), size, do_mask_bad_columns, do_mask_cosmics))
        return R.cut_stamps(self.frames, frame_index, positions_xy, size,
                            self.exptimes if exptimes is None else exptimes, self.rms if background_rms is None else background_rms)


def test_layout_of_extract_all_stamps_of_frames():
    from lightcurver_amd.io.regions import read_psf_batch, rescale_image_coordinates
    from lightcurver_amd.processes.cutout_making import extract_all_stamps_of_frames
    frames, t, rms = _frames()
    fs = _RestatedFrameSet(frames, t, rms)
    roi = np.array([[28.0, 20.0], [28.4, 19.7], [27.5, 20.5]])
    stars = [np.array([[10.0, 10.0], [50.2, 33.1]]), np.array([[11.0, 9.0]]), np.array([[9.5, 10.5], [54.0, 38.0], [1.0, 1.0]])]
    names = [['a', 'b'], ['a'], ['a', 'b', 'c']]
    rels = ['night1/f0.fits', 'night1/f1.fits', 'night2/f2.fits']
    out = extract_all_stamps_of_frames(fs, roi, stars, names, 16, 9, True, True, dict(sigclip=5.0), image_relpaths=rels)
    assert fs.calls == [(3, 16, True, True), (6, 9, True, True)]          # one call per stamp size
    assert sorted(out) == sorted(rels)
    for k, rel in enumerate(rels):
        g = out[rel]
        assert sorted(g) == ['cosmicsmask', 'data', 'frame_shape', 'image_pixel_coordinates', 'noisemap']   # no wcs
        assert tuple(g['frame_shape']) == (40, 56)
        for key in ('data', 'noisemap', 'cosmicsmask', 'image_pixel_coordinates'):
            assert sorted(g[key]) == sorted(names[k] + ['ROI'])
        for name, position, n in [('ROI', roi[k], 16)] + [(s, p, 9) for s, p in zip(names[k], stars[k])]:
            one = R.cut_stamps(frames, [k], [position], n, t, rms)
            assert R.same_bits(g['data'][name], one['data'][0]) and R.same_bits(g['noisemap'][name], one['noisemap'][0])
            assert g['cosmicsmask'][name].dtype == bool and g['cosmicsmask'][name].shape == (n, n)
            assert tuple(g['image_pixel_coordinates'][name]) == R.cutout_origin(position, n, (40, 56))[1]
    batch = read_psf_batch(out, [(rel, ids) for rel, ids in zip(rels, names)])
    assert batch['data'].shape == (3, 3, 9, 9) and batch['n_stars'].tolist() == [2, 1, 3]
    assert R.same_bits(batch['data'][2, 1], out[rels[2]]['data']['b'])
    assert np.isnan(batch['data'][2, 1][:, 6:]).all()                       # (54, 38): columns 50 .. 58 of 56
    want = rescale_image_coordinates(np.array(R.cutout_origin(stars[2][1], 9, (40, 56))[1]), (40, 56))
    assert np.array_equal(batch['positions'][2, 1], want)
    default = extract_all_stamps_of_frames(fs, roi, stars, names, 16, 9)
    assert sorted(default) == ['0', '1', '2']
    with pytest.raises(ValueError):
        extract_all_stamps_of_frames(fs, roi[:2], stars, names, 16, 9)
    with pytest.raises(ValueError):
        extract_all_stamps_of_frames(fs, roi, stars, [['a'], ['a'], ['a']], 16, 9)
