"""From raw frames to light curves (DESIGN.md section 5 "From frames to light curves"): ``light_curves_from_frames`` on
synthetic frames with injected light curves (tests/_frames_scene.py), against the truth, against the chain fed with the
truth, and against its own stages called by hand."""
import numpy as np
import pytest

from . import _frames_scene as S

pytestmark = pytest.mark.gpu

KEPT = list(S.GOOD)
SIZES = dict(stamp_size_stars=S.N_STARS, stamp_size_ROI=S.N_ROI, subsampling_factor=S.SS)
QUICK = dict(psf_n_iter_analytic=20, psf_n_iter_pixels=50, star_deconv_n_iter=50, roi_deconv_translations_iters=10,
             roi_deconv_all_iters=20)          # for the tests that look at the bookkeeping, not at the fits
MJD = 60000.0 + np.arange(S.K)


def log_rms(fluxes, truth):
    """Per source: rms over the epochs of log(fitted / true flux) about its mean."""
    return np.std(np.log(np.asarray(fluxes) / truth), axis=1)


def true_fluxes():
    """(M, K_kept): the injected light curves, before the transparency."""
    return S.roi_fluxes()[KEPT].T


@pytest.fixture(scope='module')
def run():
    from lightcurver_amd.pipeline import light_curves_from_frames
    sc = S.scene()
    out = light_curves_from_frames(sc['frames'], sc['exptimes'], S.ROI, S.POINT_SOURCES, mjd=MJD, **SIZES)
    return sc, out


def star_order():
    """The scene's stars in the order of the catalogue: by distance to the ROI."""
    return np.argsort(np.sqrt(((S.STARS - S.ROI) ** 2).sum(axis=1)), kind='stable')


def test_elimination_and_shapes(run):
    _, out = run
    assert out['eliminated'] == {S.BLANK: 'registration', S.SHIFTED: 'roi_not_in_footprint'}
    assert out['kept'].tolist() == KEPT and out['frames_fitted'].tolist() == KEPT
    assert np.array_equal(out['mjd'], MJD[KEPT])
    K, M, n_stars = len(KEPT), 2, len(out['normalization_stars'])
    assert out['fluxes'].shape == (M, K) and out['d_fluxes'].shape == (M, K) and out['reduced_chi2'].shape == (K,)
    assert np.all(np.isfinite(out['fluxes'])) and np.all(out['d_fluxes'] > 0)
    for name in ('star_fluxes', 'star_d_fluxes', 'star_chi2'):
        assert out[name].shape == (n_stars, K), name
    assert len(out['star_results']) == n_stars == 10
    for name in ('coefficient', 'coefficient_uncertainty', 'n_stars_used'):
        assert out['normalization'][name].shape == (K,), name
    assert out['zeropoint'] is None and out['global_zeropoint'] is None
    assert out['prepared']['data'].shape == (K, S.N_ROI, S.N_ROI) and out['prepared']['kept'].tolist() == list(range(K))
    assert out['footprints'].shape == (S.K, 4, 2) and np.isnan(out['footprints'][S.BLANK]).all()
    assert out['common_footprint'].ndim == 2 and out['common_footprint'].shape[1] == 2
    assert out['stars_in_frames'].shape == (S.K, 10) and len(out['psf_results']) == S.K
    assert [r is not None for r in out['psf_results']] == [k in KEPT for k in range(S.K)]
    assert out['roi_origin'].shape == (S.K, 2) and out['point_sources_in_stamps'].shape == (S.K, 2, 2)
    assert set(out['seconds']) == {'import', 'registration', 'footprints_and_stars', 'stamps', 'psf', 'star_stacks',
                                   'calibrated_light_curves'}
    print('wall clock per stage:', {k: round(v, 3) for k, v in out['seconds'].items()})
    # the catalogue is the scene's ten stars, nearest to the ROI first
    want = S.STARS[star_order()]
    got = np.stack([out['stars']['x'], out['stars']['y']], axis=1)
    assert got.shape == want.shape and np.abs(got - want).max() < 0.5
    assert out['stars']['name'].tolist() == list('abcdefghij')


def test_stars_in_frames_equal_the_table_of_the_true_transforms(run):
    sc, out = run
    truth = sc['truth']['stars_in_frames'][:, star_order()]
    registered = [k for k in range(S.K) if k != S.BLANK]
    assert np.array_equal(out['stars_in_frames'][registered], truth[registered])
    assert not out['stars_in_frames'][S.BLANK].any()
    # ragged: the star near the edge is missing from some good frames, and used where it is present
    edge = int(np.flatnonzero(star_order() == S.EDGE_STAR)[0])
    column = out['stars_in_frames'][KEPT, edge]
    assert 0 < column.sum() < len(KEPT)
    assert out['star_frame_index'][out['normalization_stars'].index(out['stars']['name'][edge])].tolist() \
        == [k for k, there in zip(KEPT, column) if there]
    assert np.array_equal(np.isnan(out['star_fluxes']), ~out['stars_in_frames'][KEPT].T)


def test_angles_equal_the_injected_rotations(run):
    """Within 0.1 degree, sign included: 0.2 px over the 128-pixel frame, far above the registration noise at this signal and
    far below the smallest injected rotation.  Measured on MI355X: 0, -0.023, +0.0002, -0.009, +0.008, +0.007 degrees for the
    kept frames (+0.039 for the shifted frame, which registers on six stars)."""
    _, out = run
    registered = [k for k in range(S.K) if k != S.BLANK]
    deviation = out['angles'][registered] - S.ROTATIONS[registered]
    print('registered angle - injected rotation (degrees):', np.array2string(deviation, precision=4))
    print('scale - 1:', np.array2string(out['scales'][registered] - 1.0, precision=5))
    assert np.all(np.abs(deviation[:len(KEPT)]) <= 0.1)
    assert np.isnan(out['angles'][S.BLANK])


def test_chi2_of_the_psf_fits_and_of_the_stars(run):
    _, out = run
    psf_chi2 = out['psf_chi2'][KEPT]
    star_chi2 = np.array([r['chi2'] for r in out['star_results']])
    print('PSF chi2 per frame:', np.array2string(psf_chi2, precision=3))
    print('star chi2 per star:', np.array2string(star_chi2, precision=3))
    print('seeing estimate per frame:', np.array2string(out['seeing_pixels'], precision=2))
    assert np.all(psf_chi2 < 2.0)
    assert np.all(star_chi2 < 2.0)


def test_coefficients_follow_the_transparency(run):
    _, out = run
    norm = out['normalization']
    ratio = norm['coefficient'] / S.T[KEPT]
    relative = norm['coefficient_uncertainty'] / norm['coefficient']
    deviation = np.abs(ratio / np.mean(ratio) - 1.0)
    print('coefficient / t:', np.array2string(ratio, precision=5))
    print('deviation from the mean ratio:', np.array2string(deviation, precision=5))
    print('relative uncertainty         :', np.array2string(relative, precision=5))
    assert np.all(deviation <= 3.0 * relative)


# ---- the chain of the parent commit, fed with the truth ----------------------------------------------------------------
def truth_fed_inputs(ctx):
    """Stamps cut at the TRUE positions from the imported frames, the generator's narrow PSFs, the true angles."""
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.star_photometry import prepare_star_epochs
    sc = S.scene()
    truth = sc['truth']
    table = truth['stars_in_frames']
    with FrameSet(sc['frames'], ctx) as fs:
        fs.import_frames(sc['exptimes'].astype(np.float32))
        roi_positions = np.array([truth['transforms'][k][:2, :2] @ S.ROI + truth['transforms'][k][:2, 2] for k in KEPT])
        roi = fs.cut_stamps(KEPT, roi_positions, S.N_ROI, do_mask_bad_columns=True, do_mask_cosmics=True)
        where = [(j, g) for j, k in enumerate(KEPT) for g in range(len(S.STARS)) if table[k, g]]
        cut = fs.cut_stamps([KEPT[j] for j, _ in where], np.array([truth['stars_xy'][KEPT[j], g] for j, g in where]), S.N_STARS,
                            do_mask_bad_columns=True, do_mask_cosmics=True)
    star_stacks, star_frame_index = [], []
    for g in range(len(S.STARS)):
        rows = [i for i, (_, gg) in enumerate(where) if gg == g]
        epochs = np.array([where[i][0] for i in rows])
        data, noisemap = prepare_star_epochs(cut['data'][rows], cut['noisemap'][rows], cut['mask'][rows])
        star_stacks.append((data, noisemap, truth['narrow_psf'][np.array(KEPT)[epochs]]))
        star_frame_index.append(epochs)
    roi_stack = (roi['data'], roi['noisemap'], roi['mask'], truth['narrow_psf'][KEPT])
    in_stamp = truth['roi_xy'][KEPT[0]] - roi['origin'][0]
    return dict(star_stacks=star_stacks, star_frame_index=star_frame_index, roi_stack=roi_stack, xs=in_stamp[:, 0],
                ys=in_stamp[:, 1], angles=S.ROTATIONS[KEPT], in_stamps=truth['roi_xy'][KEPT] - roi['origin'][:, None, :])


@pytest.fixture(scope='module')
def truth_fed(ctx):
    from lightcurver_amd.processes.calibration import calibrated_light_curves
    inp = truth_fed_inputs(ctx)
    out = calibrated_light_curves(inp['star_stacks'], inp['roi_stack'], S.SS, inp['xs'], inp['ys'],
                                  star_frame_index=inp['star_frame_index'], n_frames=len(KEPT), mjd=MJD[KEPT],
                                  angles_to_north=inp['angles'], ctx=ctx)
    return inp, out


def test_light_curves_follow_the_injected_ones(run, truth_fed):
    """The rms over the kept epochs of log(fitted flux / injected flux) about its mean, per source (A varies by +-25 %, B is
    constant; the transparency's log has an rms of 0.27 over the six frames): (a) at most a fifth of that of log t, the
    condition that calibration works; (b) at most twice what the chain gives when it is fed the truth - stamps cut at the
    true positions, the generator's narrow PSFs, the true angles - which the test computes as its comparison run.  The
    factor of two is the room given to PSFs fitted from 6 - 10 stars and to registered positions.  Measured on MI355X:
    driver 0.0034 (A) and 0.0092 (B), fed with the truth 0.0030 and 0.0094; a fifth of the rms of log t is 0.054.  With the
    angles handed over with the wrong sign the driver gives 0.094 and 0.31, with no angles 0.0056 and 0.023 (a script run
    once, not part of the suite): either fails (b)."""
    _, out = run
    _, fed = truth_fed
    driver, reference = log_rms(out['fluxes'], true_fluxes()), log_rms(fed['fluxes'], true_fluxes())
    spread = np.std(np.log(S.T[KEPT]))
    print(f'rms of log(flux / truth) over the epochs, per source: driver {driver}, fed with the truth {reference}; '
          f'rms of log t {spread:.4f}')
    print('driver flux / truth:', np.array2string(out['fluxes'] / true_fluxes(), precision=4))
    print('truth-fed flux / truth:', np.array2string(fed['fluxes'] / true_fluxes(), precision=4))
    print('driver reduced chi2 of the ROI per frame:', np.array2string(out['reduced_chi2'], precision=3))
    assert np.all(driver <= spread / 5.0)
    assert np.all(driver <= 2.0 * reference)


# ---- the driver against its stages called by hand -----------------------------------------------------------------------
def test_driver_equals_its_stages_called_by_hand(run, ctx):
    """README.md's stage-by-stage example, executable."""
    from lightcurver_amd import sep
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.calibration import calibrated_light_curves
    from lightcurver_amd.processes.frame_characterization import estimate_seeing
    from lightcurver_amd.processes.plate_solving import positions_in_frames, register_frames
    from lightcurver_amd.processes.psf_modelling import model_psfs_of_frames
    from lightcurver_amd.processes.star_extraction import sources_table_from_objects
    from lightcurver_amd.processes.star_photometry import prepare_star_epochs
    from lightcurver_amd.processes.star_selection import reference_star_catalogue, select_stars
    from lightcurver_amd.utilities.footprint import frame_angles, frame_footprints, points_in_footprints
    sc, out = run
    n, masks = S.N_STARS, dict(do_mask_bad_columns=True, do_mask_cosmics=True)
    with FrameSet(sc['frames'], ctx) as fs:
        # 1 import, 2 registration
        imported = fs.import_frames(sc['exptimes'].astype(np.float32))
        tables = [sources_table_from_objects(sep.objects_view(o)) for o in imported['objects']]
        seeing = [float(estimate_seeing(t)) for t in tables]
        results = register_frames(tables, reference=0, ctx=ctx)
        # 3 elimination: failed frames, then the ROI with a margin of half its stamp
        footprints = frame_footprints(results, S.SHAPE)
        roi_inside = points_in_footprints(S.ROI, footprints, S.N_ROI / 2.0)[:, 0]
        frames = [k for k in range(S.K) if results[k]['success'] and roi_inside[k]]
        assert frames == KEPT
        # 4 stars: the reference frame's sources but the ROI, by distance; which star is in which frame
        stars = reference_star_catalogue(tables[0], S.ROI, S.N_ROI / 2.0)
        stars_xy = np.stack([stars['x'], stars['y']], axis=1)
        table = points_in_footprints(stars_xy, footprints, n / 2.0)
        # 5 stamps: positions (x, y) in every frame from the transforms; one cut for the ROI, one for the stars
        roi_k = positions_in_frames(results, S.ROI[None])
        stars_k = positions_in_frames(results, stars_xy)
        sources_k = positions_in_frames(results, S.POINT_SOURCES)
        roi = fs.cut_stamps(frames, np.stack([roi_k[k][0] for k in frames]), S.N_ROI, **masks)
        where = [(k, g) for k in frames for g in np.flatnonzero(table[k])]
        cut = fs.cut_stamps([k for k, _ in where], np.stack([stars_k[k][g] for k, g in where]), n, **masks)
    stamp = {kg: i for i, kg in enumerate(where)}
    # 6 PSFs: per frame the (at most 16) nearest of its stars
    psf_frames = []
    for k in frames:
        rows = [stamp[k, g] for g in select_stars(stars, None, None, available=table[k])[:16]]
        psf_frames.append(dict(datas=cut['data'][rows], noisemaps=cut['noisemap'][rows], cosmics_masks=cut['mask'][rows],
                               seeing_pixels=seeing[k]))
    psfs = [res for _, res in model_psfs_of_frames(psf_frames, S.SS, 100, 3000, mask_neighbours=True)]
    assert all(res is not None for res in psfs)
    for k, res in zip(frames, psfs):
        assert np.array_equal(res['narrow_psf'], out['psf_results'][k]['narrow_psf']), k
        assert res['chi2'] == out['psf_chi2'][k]
    # 7 star stacks: per star its frames, cleaned, each epoch with its frame's narrow PSF
    star_stacks, star_frame_index = [], []
    for g in select_stars(stars, None, None):
        epochs = [j for j, k in enumerate(frames) if table[k, g]]
        rows = [stamp[frames[j], g] for j in epochs]
        data, noisemap = prepare_star_epochs(cut['data'][rows], cut['noisemap'][rows], cut['mask'][rows])
        star_stacks.append((data, noisemap, np.stack([psfs[j]['narrow_psf'] for j in epochs])))
        star_frame_index.append(np.array(epochs))
    # 8 the chain; the sources where they are in the first frame's ROI stamp: position in the frame minus the stamp's origin
    in_stamp = sources_k[frames[0]] - roi['origin'][0]
    roi_stack = (roi['data'], roi['noisemap'], roi['mask'], np.stack([res['narrow_psf'] for res in psfs]))
    by_hand = calibrated_light_curves(star_stacks, roi_stack, S.SS, in_stamp[:, 0], in_stamp[:, 1],
                                      star_frame_index=star_frame_index, n_frames=len(frames), mjd=MJD[frames],
                                      psf_chi2=np.array([res['chi2'] for res in psfs]),
                                      angles_to_north=frame_angles(results)[frames], ctx=ctx)
    assert np.array_equal(np.array(frames)[by_hand['kept']], out['kept'])
    assert np.array_equal(by_hand['fluxes'], out['fluxes']) and np.array_equal(by_hand['d_fluxes'], out['d_fluxes'])
    for key in ('coefficient', 'coefficient_uncertainty'):
        assert np.array_equal(by_hand['normalization'][key], out['normalization'][key]), key
    assert np.array_equal(roi['origin'], out['roi_origin'][frames])


# ---- the two forms of the positions in calibrated_light_curves ------------------------------------------------------------
def test_calibrated_light_curves_takes_positions_per_frame(truth_fed, ctx):
    from lightcurver_amd.processes.calibration import calibrated_light_curves
    inp, _ = truth_fed
    quick = dict(star_n_iter=50, roi_deconv_translations_iters=10, roi_deconv_all_iters=20)
    n_frames = len(KEPT)

    def chain(xs, ys, **kw):
        return calibrated_light_curves(inp['star_stacks'], inp['roi_stack'], S.SS, xs, ys, star_frame_index=inp['star_frame_index'],
                                       n_frames=n_frames, angles_to_north=inp['angles'], ctx=ctx, **quick, **kw)

    def same(a, b):
        return all(np.array_equal(a[key], b[key]) for key in ('fluxes', 'd_fluxes', 'reduced_chi2', 'kept'))

    plain = chain(inp['xs'], inp['ys'])
    assert same(chain(np.tile(inp['xs'], (n_frames, 1)), np.tile(inp['ys'], (n_frames, 1))), plain)
    # rows that differ: the sources in every frame's own stamp; row kept[0] is the one used
    per_frame = inp['in_stamps']                                              # (n_frames, M, 2)
    assert np.abs(per_frame[1] - per_frame[0]).max() > 0.05
    assert same(chain(per_frame[:, :, 0], per_frame[:, :, 1]), plain)
    drop_first = dict(frame_columns={'frame': np.arange(n_frames)}, frame_constraints={'frame': (1, n_frames)})
    without_first = chain(per_frame[:, :, 0], per_frame[:, :, 1], **drop_first)
    assert without_first['kept'].tolist() == list(range(1, n_frames))
    assert same(without_first, chain(per_frame[1, :, 0], per_frame[1, :, 1], **drop_first))
    assert not same(without_first, chain(per_frame[0, :, 0], per_frame[0, :, 1], **drop_first))
    with pytest.raises(ValueError, match='n_frames'):
        chain(per_frame[1:, :, 0], per_frame[1:, :, 1])
    with pytest.raises(ValueError, match='n_frames'):
        chain(per_frame[:, :, 0], per_frame[0, :, 1])


def test_common_footprint_stars_leaves_out_the_star_near_the_edge(run):
    from lightcurver_amd.pipeline import light_curves_from_frames
    sc, full = run
    out = light_curves_from_frames(sc['frames'], sc['exptimes'], S.ROI, S.POINT_SOURCES,
                                   star_selection_strategy='common_footprint_stars', **SIZES, **QUICK)
    everywhere = full['stars_in_frames'][KEPT].all(axis=0)
    assert not everywhere.all() and not everywhere[int(np.flatnonzero(star_order() == S.EDGE_STAR)[0])]
    assert out['stars']['name'].tolist() == full['stars']['name'][everywhere].tolist()
    assert out['stars_in_frames'].shape == (S.K, everywhere.sum()) and out['stars_in_frames'][KEPT].all()
    assert out['normalization_stars'] == out['stars']['name'].tolist()
    assert all(names == out['normalization_stars'] for names in out['psf_stars'].values())
    assert not np.isnan(out['star_fluxes']).any() and out['kept'].tolist() == KEPT


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(monkeypatch, ctx):
    from lightcurver_amd import frames as frames_module
    from lightcurver_amd.pipeline import light_curves_from_frames
    sc = S.scene()
    imported_set = frames_module.FrameSet(sc['frames'][:3], ctx)
    try:
        imported_set.import_frames(sc['exptimes'][:3].astype(np.float32))

        def no_device(*args, **kw):
            raise AssertionError('the driver reached the device')

        monkeypatch.setattr(frames_module.FrameSet, '__init__', no_device)
        monkeypatch.setattr(frames_module.FrameSet, 'import_frames', no_device)
        monkeypatch.setattr(frames_module.FrameSet, 'cut_stamps', no_device)
        call = lambda frames=sc['frames'], exptimes=sc['exptimes'], roi=S.ROI, **kw: \
            light_curves_from_frames(frames, exptimes, roi, S.POINT_SOURCES, **{**SIZES, **kw})
        with pytest.raises(ValueError, match='stamp_size_stars'):
            call(stamp_size_stars=7)
        with pytest.raises(ValueError, match='stamp_size_ROI'):
            call(stamp_size_ROI=7)
        with pytest.raises(ValueError, match='outside the reference frame'):
            call(roi=(S.SHAPE[1] + 3.0, 40.0))
        with pytest.raises(ValueError, match='outside the reference frame'):
            call(roi=(130.0, 84.6))                             # x beyond w = 128, though inside h = 160: not (row, column)
        with pytest.raises(ValueError, match='exptimes'):
            call(exptimes=sc['exptimes'][:5])
        with pytest.raises(ValueError, match='imported already'):
            call(frames=imported_set, exptimes=sc['exptimes'][:3])
        with pytest.raises(ValueError, match='at least 3'):
            call(frames=sc['frames'][:2], exptimes=sc['exptimes'][:2])
        with pytest.raises(ValueError, match='star_selection_strategy'):
            call(star_selection_strategy='ROI_disk')
        with pytest.raises(ValueError, match='catalog_mags'):
            call(catalog_mags=np.zeros(10))
    finally:
        monkeypatch.undo()
        imported_set.close()


def test_two_good_frames_are_refused_before_any_stamp_is_cut(monkeypatch):
    from lightcurver_amd import frames as frames_module
    from lightcurver_amd.pipeline import light_curves_from_frames
    frames, exptimes = S.two_good_frames()

    def no_stamp(*args, **kw):
        raise AssertionError('a stamp was cut')

    monkeypatch.setattr(frames_module.FrameSet, 'cut_stamps', no_stamp)
    with pytest.raises(ValueError, match='2 of 3 frames survive'):
        light_curves_from_frames(frames, exptimes, S.ROI, S.POINT_SOURCES, **SIZES)
