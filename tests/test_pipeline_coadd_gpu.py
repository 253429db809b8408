"""``light_curves_from_frames(star_catalogue_from='coadd')`` on the scene of tests/_frames_scene.py (DESIGN.md section 5
"Co-addition of frames"): the star catalogue comes from the co-add of the surviving frames instead of from the reference
frame's own sources.  The catalogue against the truth and against the reference frame's, the light curves against the chain
fed with the truth (the acceptance rule of tests/test_pipeline_gpu.py), and the co-add stage against its parts called by
hand."""
import numpy as np
import pytest

from . import _frames_scene as S
from .test_pipeline_gpu import KEPT, MJD, SIZES, log_rms, true_fluxes, truth_fed_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def run():
    from lightcurver_amd.pipeline import light_curves_from_frames
    sc = S.scene()
    out = light_curves_from_frames(sc['frames'], sc['exptimes'], S.ROI, S.POINT_SOURCES, mjd=MJD, star_catalogue_from='coadd',
                                   **SIZES)
    return sc, out


@pytest.fixture(scope='module')
def by_hand(ctx):
    """Stages 1 to 3 and the co-add stage, as a user would call them."""
    from lightcurver_amd import sep
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.coaddition import coadd_frames, relative_flux_scales
    from lightcurver_amd.processes.plate_solving import register_frames
    from lightcurver_amd.processes.star_extraction import extract_stars, sources_table_from_objects
    from lightcurver_amd.processes.star_selection import reference_star_catalogue
    from lightcurver_amd.utilities.footprint import frame_footprints, points_in_footprints
    sc = S.scene()
    with FrameSet(sc['frames'], ctx) as fs:
        imported = fs.import_frames(sc['exptimes'].astype(np.float32))
        tables = [sources_table_from_objects(sep.objects_view(o)) for o in imported['objects']]
        results = register_frames(tables, reference=0, ctx=ctx)
        roi_inside = points_in_footprints(S.ROI, frame_footprints(results, S.SHAPE), S.N_ROI / 2.0)[:, 0]
        frames = [k for k in range(S.K) if results[k]['success'] and roi_inside[k]]
        scales = relative_flux_scales(tables, results, 0)
        coadd = coadd_frames(fs, results, frames, flux_scale=scales, order=3, combine='median')
        mean = coadd_frames(fs, results, frames, flux_scale=scales, order=3, combine='mean')
    with np.errstate(divide='ignore'):
        table = extract_stars(coadd['image'], 1.0 / coadd['weight'], ctx=ctx)
    return dict(frames=frames, scales=scales, coadd=coadd, mean=mean, table=table, tables=tables, imported=imported,
                stars=reference_star_catalogue(table, S.ROI, S.N_ROI / 2.0),
                reference_stars=reference_star_catalogue(tables[0], S.ROI, S.N_ROI / 2.0))


def _nearest(xy, catalogue):
    got = np.stack([catalogue['x'], catalogue['y']], axis=1)
    return np.sqrt(((got[None] - np.asarray(xy)[:, None]) ** 2).sum(-1)).min(axis=1)


def test_catalogue_of_the_coadd_holds_the_stars_of_the_reference_catalogue(run, by_hand):
    _, out = run
    held = _nearest(S.STARS, by_hand['reference_stars']) < 0.5                 # the truth's stars the reference frame detected
    assert held.sum() == len(S.STARS)
    distance = _nearest(S.STARS, out['stars'])
    print('distance of the truth\'s stars to the co-add catalogue (px):', np.array2string(distance, precision=3))
    print('to the reference frame\'s catalogue:', np.array2string(_nearest(S.STARS, by_hand['reference_stars']), precision=3))
    assert np.all(distance[held] < 0.5)
    assert set(out['seconds']) == {'import', 'registration', 'coadd', 'footprints_and_stars', 'stamps', 'psf', 'star_stacks',
                                   'calibrated_light_curves'}
    assert out['eliminated'] == {S.BLANK: 'registration', S.SHIFTED: 'roi_not_in_footprint'} and out['kept'].tolist() == KEPT
    # below 11 frames the driver takes the median; every kept frame went in
    co = out['coadd']
    assert co['frames'].tolist() == KEPT and not co['n_rejected'].any() and co['count'].max() == len(KEPT)
    assert co['image'].shape == S.SHAPE and np.isnan(co['image']).any()
    # pixels no frame covers yield no source
    covered = co['count'] > 0
    assert not covered.all() and np.array_equal(covered, np.isfinite(co['image']))
    t = co['sources_table']
    assert len(t) >= len(S.STARS) and covered[np.rint(t['y']).astype(int), np.rint(t['x']).astype(int)].all()


def test_relative_flux_scales_follow_the_transparency(by_hand):
    """The frames' fluxes are the scene's times the transparency, so the scale that brings frame k onto the reference is
    T[0] / T[k], within the photometric noise of the matched stars' isophotal fluxes (a few per cent)."""
    scales = by_hand['scales']
    assert scales[0] == 1.0 and np.isnan(scales[S.BLANK])
    want = S.T[0] / S.T[KEPT]
    print('relative flux scale x transparency ratio:', np.array2string(scales[KEPT] / want, precision=4))
    assert np.all(np.abs(scales[KEPT] / want - 1.0) < 0.1)


def test_coadd_is_deeper_than_the_reference_frame(by_hand):
    """The rms of the source-free sky of the weighted-mean co-add against that of the imported reference frame: with the
    weights 1 / (s rms)^2 it is at most 1.1 / sqrt(sum w) (interpolation only lowers it), far below the frame's own."""
    mean = by_hand['mean']
    full = mean['count'] == len(KEPT)
    yy, xx = np.mgrid[0:S.SHAPE[0], 0:S.SHAPE[1]]
    away = np.ones(S.SHAPE, bool)
    for x, y in np.vstack([S.STARS, S.POINT_SOURCES]):
        away &= (xx - x) ** 2 + (yy - y) ** 2 > 14.0 ** 2
    sky = full & away
    assert sky.sum() >= 5000
    rms = float(np.sqrt(np.mean(mean['image'][sky].astype(np.float64) ** 2)))
    expected = float(np.median(1.0 / np.sqrt(mean['weight'][sky])))
    single = float(by_hand['imported']['globalrms'][0])
    print(f'sky rms of the co-add {rms:.4f}, 1 / sqrt(sum w) {expected:.4f}, of the reference frame {single:.4f}')
    assert rms <= 1.1 * expected and rms < 0.6 * single


def test_light_curves_follow_the_injected_ones(run, ctx):
    """The acceptance rule of tests/test_pipeline_gpu.py: the rms over the kept epochs of log(fitted / injected flux), per
    source, is at most twice what the chain gives when it is fed the truth, computed in the same run."""
    from lightcurver_amd.processes.calibration import calibrated_light_curves
    _, out = run
    inp = truth_fed_inputs(ctx)
    fed = calibrated_light_curves(inp['star_stacks'], inp['roi_stack'], S.SS, inp['xs'], inp['ys'],
                                  star_frame_index=inp['star_frame_index'], n_frames=len(KEPT), mjd=MJD[KEPT],
                                  angles_to_north=inp['angles'], ctx=ctx)
    driver, reference = log_rms(out['fluxes'], true_fluxes()), log_rms(fed['fluxes'], true_fluxes())
    print(f'rms of log(flux / truth) over the epochs, per source: driver with the co-add catalogue {driver}, fed with the '
          f'truth {reference}')
    assert np.all(driver <= 2.0 * reference)


def test_driver_equals_the_coadd_stage_called_by_hand(run, by_hand):
    _, out = run
    assert by_hand['frames'] == KEPT
    for key in ('image', 'weight', 'count', 'n_rejected'):
        assert np.array_equal(out['coadd'][key].view(np.uint32), by_hand['coadd'][key].view(np.uint32)), key
    assert out['coadd']['sources_table'].tobytes() == by_hand['table'].tobytes()
    assert out['stars'].dtype == by_hand['stars'].dtype and out['stars'].tobytes() == by_hand['stars'].tobytes()


def test_a_catalogue_from_the_caller_still_wins_and_bad_options_are_refused(by_hand, monkeypatch):
    from lightcurver_amd import frames as frames_module
    from lightcurver_amd.pipeline import light_curves_from_frames
    sc = S.scene()

    def no_device(*args, **kw):
        raise AssertionError('the driver reached the device')

    monkeypatch.setattr(frames_module.FrameSet, '__init__', no_device)
    call = lambda **kw: light_curves_from_frames(sc['frames'], sc['exptimes'], S.ROI, S.POINT_SOURCES, **{**SIZES, **kw})
    with pytest.raises(ValueError, match='star_catalogue_from'):
        call(star_catalogue_from='gaia')
    with pytest.raises(ValueError, match='coadd_order'):
        call(star_catalogue_from='coadd', coadd_order=2)
    with pytest.raises(ValueError, match='coadd_combine'):
        call(star_catalogue_from='coadd', coadd_combine='sum')
    monkeypatch.undo()
    monkeypatch.setattr(frames_module.FrameSet, 'coadd', no_device)
    quick = dict(psf_n_iter_analytic=20, psf_n_iter_pixels=50, star_deconv_n_iter=50, roi_deconv_translations_iters=10,
                 roi_deconv_all_iters=20)
    out = call(star_catalogue=by_hand['reference_stars'], star_catalogue_from='coadd', **quick)
    assert 'coadd' not in out and 'coadd' not in out['seconds']
    assert out['stars'].tobytes() == by_hand['reference_stars'].tobytes()
