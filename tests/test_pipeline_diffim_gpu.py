"""Difference imaging at the end of the whole-frame chain, on the scene of tests/_frames_scene.py (DESIGN.md section 5
"Difference imaging"): import, register, ``coadd_frames``, ``difference_frames`` with r = 3, the ROI masked from the fit
as a user who knows the target varies would mask it.  The differences against the restatement of tests/_diffim.py on the
same resampled frames, the photometric scale against the injected transparency, and the difference light curve of the
ROI blend against the injected variation of source A."""
import numpy as np
import pytest

from . import _diffim as DI
from . import _frames_scene as S

pytestmark = pytest.mark.gpu

KEPT = list(S.GOOD)
APERTURE = 8.0          # holds both point sources (3.5 px apart) at every seeing of the scene
MASK_RADIUS = 12.0
SETTINGS = dict(r=3, bg_degree=1, regions=(1, 1), clip_iters=2, n_sigma=4.0)


def _roi_mask():
    yy, xx = np.mgrid[0:S.SHAPE[0], 0:S.SHAPE[1]]
    return ((xx - S.ROI[0]) ** 2 + (yy - S.ROI[1]) ** 2 <= MASK_RADIUS ** 2).astype(np.uint8)


@pytest.fixture(scope='module')
def chain(ctx):
    from lightcurver_amd import sep
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.coaddition import coadd_frames, relative_flux_scales
    from lightcurver_amd.processes.difference_imaging import difference_frames
    from lightcurver_amd.processes.plate_solving import register_frames
    from lightcurver_amd.processes.star_extraction import sources_table_from_objects
    sc = S.scene()
    with FrameSet(sc['frames'], ctx) as fs:
        imported = fs.import_frames(sc['exptimes'].astype(np.float32))
        tables = [sources_table_from_objects(sep.objects_view(o)) for o in imported['objects']]
        results = register_frames(tables, reference=0, ctx=ctx)
        scales = relative_flux_scales(tables, results, 0)
        deep = coadd_frames(fs, results, KEPT, flux_scale=scales, order=3, combine='median')
        diff = difference_frames(fs, results, deep['image'], KEPT + [S.BLANK], mask=_roi_mask(), **SETTINGS)
        by_set = difference_frames(fs, results, deep['image'], mask=np.broadcast_to(_roi_mask(), (S.K,) + S.SHAPE),
                                   sigma=np.where(np.isfinite(imported['globalrms']), imported['globalrms'], 1.0),
                                   download=('n_used',), **SETTINGS)
        warped = np.stack([fs.coadd([k], [results[k]['transform']], order=3, combine='mean', weights=[1.0])['image']
                           for k in KEPT])
        m = [np.asarray(results[k]['transform'].params, np.float64) for k in KEPT]
        sigma = np.array([np.float64(imported['globalrms'][k]) * abs(a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0])
                          for k, a in zip(KEPT, m)], np.float32)
    return dict(deep=deep, diff=diff, warped=warped, sigma=sigma, scales=scales, by_set=by_set)


@pytest.fixture(scope='module')
def restated(chain):
    return [DI.subtract(chain['warped'][i], chain['deep']['image'], mask=_roi_mask(), sigma=chain['sigma'][i], **SETTINGS)
            for i in range(len(KEPT))]


def test_differences_equal_the_restatement_on_the_same_frames(chain, restated):
    diff = chain['diff']
    assert diff['frames'].tolist() == KEPT                                  # the blank frame failed its registration
    assert (diff['status'] == 0).all()
    # sigma and mask per frame of the set: the frames that failed fall out with their entries
    assert chain['by_set']['frames'].tolist() == [k for k in range(S.K) if k != S.BLANK]
    assert chain['by_set']['n_used'].shape == (S.K - 1, 1) and (chain['by_set']['n_used'][:len(KEPT)] > 0).all()
    for i, ref in enumerate(restated):
        assert diff['n_used'][i, 0] == ref['n_used'][0]
        assert np.array_equal(np.isnan(diff['diff'][i]), np.isnan(ref['diff64']))
        ok = np.isfinite(ref['diff64'])
        ratio = np.abs(diff['diff'][i][ok] - ref['diff64'][ok]) / DI.diff_bound(ref['magnitude'][ok])
        print(f'frame {KEPT[i]}: n_used {ref["n_used"][0]}, chi2 {diff["chi2"][i, 0]:.3f}, worst error {ratio.max():.3f} of the bound')
        assert ratio.max() <= 1.0


def test_scale_follows_the_transparency(chain, restated):
    """The deep image is on frame 0's flux scale (``relative_flux_scales``), so the photometric scale of frame k against
    it is T[k] / T[0].  Held to twice the deviation the float64 restatement shows on the same inputs."""
    want = S.T[KEPT] / S.T[0]
    got = chain['diff']['scale'][:, 0] / want - 1.0
    ref = np.array([r['scale'][0] for r in restated]) / want - 1.0
    print('scale / (T[k] / T[0]) - 1 on the device:', np.array2string(got, precision=5), 'restated:',
          np.array2string(ref, precision=5), 'against 1 / relative_flux_scales:',
          np.array2string(chain['diff']['scale'][:, 0] * chain['scales'][KEPT] - 1.0, precision=5))
    assert np.all(np.abs(got) <= 2.0 * np.abs(ref))
    assert np.all(np.abs(ref) < 0.03)


def test_the_blend_varies_and_the_stars_do_not(chain, ctx):
    """The difference light curve of the ROI blend, in an aperture that holds both sources, against the injected
    variation of A (B is constant): with the scene's true transforms and tests/_coadd.py the restatement gives a
    correlation of 0.999 and a slope of 0.99 for the blend, and slopes of at most 0.0094 in size for the ten stars (the
    correlation coefficient of six noisy points is no measure there: it ranges from -0.92 to 0.56).  Asked here: correlation >
    0.98, slope within 0.1 of 1, and five times the restatement's worst slope for the stars."""
    from lightcurver_amd.processes.difference_imaging import difference_light_curves
    diff = chain['diff']
    positions = np.vstack([S.ROI[None], S.STARS])
    lc = difference_light_curves(diff['diff'], diff['scale'], positions, APERTURE, sigma=chain['sigma'], ctx=ctx)
    a = S.roi_fluxes()[KEPT, 0] * S.T[0]
    slopes, corr = np.full(len(positions), np.nan), np.full(len(positions), np.nan)
    for j in range(len(positions)):
        f = lc['flux'][:, j]
        ok = np.isfinite(f)
        if ok.sum() >= 4:
            slopes[j] = np.polyfit(a[ok], f[ok], 1)[0]
            corr[j] = np.corrcoef(a[ok], f[ok])[0, 1]
    print('slope against the variation of A: blend', round(slopes[0], 4), 'stars', np.array2string(slopes[1:], precision=4),
          'correlation: blend', round(corr[0], 4), 'stars', np.array2string(corr[1:], precision=3))
    assert np.isfinite(slopes).all()
    assert corr[0] > 0.98 and abs(slopes[0] - 1.0) < 0.1
    assert np.all(np.abs(slopes[1:]) < 0.05)
