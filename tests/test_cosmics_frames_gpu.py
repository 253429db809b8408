"""The frame form of the cosmic-ray kernels on the device (lc_detect_cosmics_frames, lc_frames_detect_cosmics) against the
float32 restatement of the SPEC on the whole frame (tests/_lacosmic.py): bit for bit on crmask, clean and iters, no
tolerance and no excluded pixel.  The inputs are those tests/test_cosmics_frames_cpu.py holds to their properties."""
import ctypes as C

import numpy as np
import pytest

from tests import _cosmics_frames as CF
from tests import _lacosmic as LA

pytestmark = pytest.mark.gpu

_ip = C.POINTER(C.c_int32)
_u8 = C.POINTER(C.c_uint8)


def _check(got, want, label):
    print(label, 'iters', got['iters'], 'flagged', got['n_flagged'], 'kernel_ms', round(got['kernel_ms'], 3))
    assert not CF.same(got, want), label
    assert np.array_equal(got['n_flagged'], want['crmask'].reshape(len(got['iters']), -1).sum(axis=1)), label


# ---- 1. bit equality with the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_invar', (False, True))
@pytest.mark.parametrize('shape', CF.SHAPES)
def test_equals_the_restatement(ctx, shape, with_invar):
    from lightcurver_amd.astroscrappy import lacosmic_frames
    d, (y, x) = CF.plain_input(shape)
    kw = dict(invar=CF.model_invar(d)) if with_invar else {}
    got = lacosmic_frames(d, ctx=ctx, **kw)
    _check(got, CF.wanted(d, **kw), (shape, with_invar))
    assert got['crmask'][0, y, x]


@pytest.mark.parametrize('shape', ((40, 56), (65, 127)))
def test_global_fallback(ctx, shape):
    from lightcurver_amd.astroscrappy import lacosmic_frames
    d, inmask, (cy, cx) = CF.fallback_input(shape)
    got = lacosmic_frames(d, inmask=inmask, ctx=ctx)
    _check(got, CF.wanted(d, inmask=inmask), shape)
    # everything but the hit is masked: no good pixel in the frame, the value is 0
    alone = CF.all_but(d.shape, cy, cx)
    got = lacosmic_frames(d, inmask=alone, ctx=ctx)
    _check(got, CF.wanted(d, inmask=alone), (shape, 'no good pixel'))
    assert got['crmask'][0, cy, cx] and got['clean'][0, cy, cx] == 0.0


@pytest.mark.parametrize('with_invar', (False, True))
def test_frames_of_one_call_stop_at_different_iterations(ctx, with_invar):
    from lightcurver_amd.astroscrappy import lacosmic_frames
    d = CF.early_exit_input()
    kw = dict(invar=CF.model_invar(d)) if with_invar else {}
    got = lacosmic_frames(d, ctx=ctx, **kw)
    _check(got, CF.wanted(d, **kw), with_invar)
    assert list(got['iters']) == [1, 2, 4]
    got = lacosmic_frames(d, niter=12, ctx=ctx, **kw)
    _check(got, CF.wanted(d, niter=12, **kw), (with_invar, 'niter 12'))
    assert list(got['iters']) == [1, 2, 12]
    got = lacosmic_frames(d, niter=0, ctx=ctx, **kw)
    _check(got, CF.wanted(d, niter=0, **kw), (with_invar, 'niter 0'))


def test_hits_across_every_tile_line_and_chunking(ctx):
    from lightcurver_amd.astroscrappy import lacosmic_frames
    d, hit = CF.straddle_input()
    got = lacosmic_frames(d, ctx=ctx)
    _check(got, CF.wanted(d), 'straddle')
    assert got['crmask'][hit].all() and list(got['n_flagged']) == [240, 0]
    one = lacosmic_frames(d, scratch_frames=1, ctx=ctx)
    assert not CF.same(one, got) and np.array_equal(one['n_flagged'], got['n_flagged'])
    # a frame's result does not depend on what else is in the call
    alone = lacosmic_frames(d[:1], ctx=ctx)
    assert np.array_equal(alone['crmask'][0], got['crmask'][0]) and np.array_equal(CF.bits(alone['clean'][0]), CF.bits(got['clean'][0]))


def test_saturated_core_and_nan_columns(ctx):
    from lightcurver_amd.astroscrappy import lacosmic_frames
    d = CF.saturated_input()
    got = lacosmic_frames(d, ctx=ctx)
    _check(got, CF.wanted(d), 'saturated')
    assert not got['crmask'].any()
    d = CF.nan_columns_input()
    got = lacosmic_frames(d, ctx=ctx)
    _check(got, CF.wanted(d), 'nan columns')
    assert np.isfinite(got['clean']).all()


def test_settings_other_than_the_defaults(ctx):
    from lightcurver_amd.astroscrappy import lacosmic_frames
    for label, d, case, base in CF.settings_cases():
        want = CF.wanted(d, **case)
        assert CF.same(want, CF.wanted(d, **base)), label
        _check(lacosmic_frames(d, ctx=ctx, **case), want, label)


# ---- 2. agreement with the stamp kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (24, 64, 65, 128))
def test_square_frames_equal_the_stamp_kernel(ctx, n):
    from lightcurver_amd import astroscrappy
    d, nm, inmask, satlevel = LA.star_stamps(3, n, seed=10 * n + (5 if n == 128 else 6), electrons=False)
    kw = dict(inmask=inmask, invar=nm ** 2, satlevel=satlevel)
    stamp = astroscrappy.lacosmic(d, ctx=ctx, **kw)
    frame = astroscrappy.lacosmic_frames(d, ctx=ctx, **kw)
    print(n, stamp['iters'], frame['n_flagged'])
    assert not CF.same(frame, stamp) and frame['n_flagged'].sum() >= 4
    frame = astroscrappy.lacosmic_frames(d, inmask=inmask, satlevel=satlevel, gain=1.5, ctx=ctx)
    assert not CF.same(frame, astroscrappy.lacosmic(d, inmask=inmask, satlevel=satlevel, gain=1.5, ctx=ctx))
    # detect_cosmics keeps the stamp kernel for the inputs it has always taken, and sends the others to the frame kernel
    cr, clean = astroscrappy.detect_cosmics(d, ctx=ctx, **kw)
    assert np.array_equal(cr, stamp['crmask']) and np.array_equal(CF.bits(clean), CF.bits(stamp['clean']))


def test_detect_cosmics_takes_whole_images(ctx):
    from lightcurver_amd.astroscrappy import detect_cosmics
    d, inmask, _ = CF.fallback_input((40, 56))
    want = CF.wanted(d, inmask=inmask)
    cr, clean = detect_cosmics(d[0], inmask=inmask[0], ctx=ctx)
    assert cr.shape == (40, 56) and np.array_equal(cr, want['crmask'][0]) and np.array_equal(CF.bits(clean), CF.bits(want['clean'][0]))
    d, _ = CF.plain_input((130, 67))
    cr, clean = detect_cosmics(d, ctx=ctx)
    assert np.array_equal(cr, CF.wanted(d)['crmask']) and np.array_equal(CF.bits(clean), CF.bits(CF.wanted(d)['clean']))


# ---- 3. FrameSet ---------------------------------------------------------------------------------------------------------------------
def _frame_noisemaps(fs, index, **kw):
    """The noise map cut_stamps forms, for the whole frames ``index``: one stamp per frame that covers it."""
    K, h, w = fs.shape
    n = max(h, w)
    cut = fs.cut_stamps(index, np.tile([(n - 1) / 2.0, (n - 1) / 2.0], (len(index), 1)), n, **kw)
    assert (cut['origin'] == 0).all()
    return cut['noisemap'][:, :h, :w]


def _with_hits(frames, amplitude, seed):
    d = np.array(frames, np.float32)
    rng = np.random.default_rng(seed)
    K, h, w = d.shape
    for k in range(K):
        for _ in range(6):
            y, x = int(rng.integers(3, h - 4)), int(rng.integers(3, w - 4))
            d[k, y, x:x + 1 + k % 2] += amplitude
    return d


def test_frameset_on_a_raw_set(ctx):
    from lightcurver_amd.frames import FrameSet
    d = _with_hits(CF.sky((3, 70, 101), 31), 3000.0, 32)
    with FrameSet(d, ctx) as fs:
        # noise = 'model' is the default of a raw set; apply = None leaves the planes as they are
        got = fs.detect_cosmics(download=('crmask', 'clean'))
        _check(got, CF.wanted(d), 'raw model')
        assert got['n_flagged'].min() >= 6 and np.array_equal(CF.bits(fs.planes()), CF.bits(d))
        # a list in another order, a frame twice, no download
        twice = fs.detect_cosmics([2, 0, 2], download=())
        assert twice['crmask'] is None and twice['clean'] is None
        assert np.array_equal(twice['n_flagged'], got['n_flagged'][[2, 0, 2]]) and np.array_equal(twice['iters'], got['iters'][[2, 0, 2]])
        # noise = 'rms' with explicit exposure times and rms: the variance is the square of cut_stamps' noise map
        t, rms = np.array([60.0, 45.0, 90.0], np.float32), np.array([0.3, 0.4, 0.25], np.float32)
        nm = _frame_noisemaps(fs, np.arange(3), exptimes=t, background_rms=rms)
        rmsgot = fs.detect_cosmics(exptimes=t, background_rms=rms, noise='rms', download=('crmask', 'clean'))
        _check(rmsgot, CF.wanted(d, invar=nm * nm), 'raw rms')
        inmask = np.random.default_rng(5).uniform(size=(2, 70, 101)) < 0.02
        masked = fs.detect_cosmics([1, 2], inmask=inmask, download=('crmask', 'clean'), scratch_frames=1,
                                   cosmics_masking_params=dict(sigclip=4.0, gain=1.3))
        _check(masked, CF.wanted(d[1:], inmask=inmask, sigclip=4.0, gain=1.3), 'raw masked')
        with pytest.raises(Exception, match='rms|imported'):
            fs.detect_cosmics(noise='rms')
        with pytest.raises(ValueError, match='twice'):
            fs.detect_cosmics([0, 1, 0], apply='nan')
        with pytest.raises(NotImplementedError):
            fs.detect_cosmics(cosmics_masking_params=dict(sepmed=False))
        assert np.array_equal(CF.bits(fs.planes()), CF.bits(d))
        # apply = 'clean': the flagged pixels of the listed frames take the cleaned values
        fs.detect_cosmics([1], apply='clean', download=())
        planes = fs.planes()
        assert np.array_equal(CF.bits(planes[1]), CF.bits(got['clean'][1])) and got['crmask'][1].any()
        assert np.array_equal(CF.bits(planes[[0, 2]]), CF.bits(d[[0, 2]]))
        # apply = 'nan': NaN exactly on crmask
        out = fs.detect_cosmics([0, 2], apply='nan')
        planes = fs.planes()
        assert np.array_equal(out['crmask'], got['crmask'][[0, 2]])
        assert np.array_equal(np.isnan(planes[[0, 2]]), got['crmask'][[0, 2]])
        keep = ~got['crmask'][[0, 2]]
        assert np.array_equal(CF.bits(planes[[0, 2]][keep]), CF.bits(d[[0, 2]][keep]))


def test_frameset_on_an_imported_set(ctx):
    from lightcurver_amd.frames import FrameSet
    from tests import _frames_scene as S
    sc = S.scene()
    d = _with_hits(sc['frames'][:3], 400.0, 33)
    with FrameSet(d, ctx) as fs:
        fs.import_frames(sc['exptimes'][:3].astype(np.float32))
        assert fs.imported
        planes = fs.planes()
        nm = _frame_noisemaps(fs, np.arange(3))
        got = fs.detect_cosmics(download=('crmask', 'clean'))                  # noise = 'rms' from the recorded values
        want = CF.wanted(planes, invar=nm * nm)
        _check(got, want, 'imported rms')
        assert got['n_flagged'].min() >= 6
        model = fs.detect_cosmics(noise='model', download=('crmask', 'clean'))
        _check(model, CF.wanted(planes), 'imported model')
        assert np.array_equal(CF.bits(fs.planes()), CF.bits(planes))


def test_refusals_leave_the_outputs_untouched(ctx):
    from lightcurver_amd import _lib
    from lightcurver_amd.frames import FrameSet
    lib = _lib.lib()
    K, h, w = 2, 9, 12
    d = CF.sky((K, h, w), 41)
    good = _lib.CosmicsCfg(4.5, 0.3, 5.0, 1.0, 6.5, 65536.0, 4, 1, 0, 0)

    def cfg(**kw):
        c = _lib.CosmicsCfg(4.5, 0.3, 5.0, 1.0, 6.5, 65536.0, 4, 1, 0, 0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def outputs():
        return (np.full((K, h, w), 7, np.uint8), np.full((K, h, w), -7.0, np.float32), np.full(K, -7, np.int32),
                np.full(K, -7, np.int32))

    def untouched(out):
        return (out[0] == 7).all() and (out[1] == -7.0).all() and (out[2] == -7).all() and (out[3] == -7).all()

    p = lambda a, t: None if a is None else a.ctypes.data_as(t)

    def host(K=K, h=h, w=w, data=d, c=good, scratch=0, crmask=True):
        out = outputs()
        rc = lib.lc_detect_cosmics_frames(ctx.h, K, h, w, p(data, _lib.fp), None, None, None if c is None else C.byref(c),
                                          scratch, p(out[0], _u8) if crmask else None, p(out[1], _lib.fp), p(out[2], _ip),
                                          p(out[3], _ip), None)
        return rc, out

    bad_settings = dict(gain_zero=cfg(gain=0.0), gain_nan=cfg(gain=float('nan')), sigclip_inf=cfg(sigclip=float('inf')),
                        niter_negative=cfg(niter=-1), satlevel_nan=cfg(satlevel=float('nan')))
    invalid = dict(K_zero=dict(K=0), K_negative=dict(K=-2), no_data=dict(data=None), no_cfg=dict(c=None),
                   no_crmask=dict(crmask=False), scratch_negative=dict(scratch=-1),
                   **{k: dict(c=v) for k, v in bad_settings.items()})
    unsupported = dict(h_small=dict(h=7, w=15), w_small=dict(h=27, w=4), sepmed_0=dict(c=cfg(sepmed=0)),
                       cleantype=dict(c=cfg(cleantype=1)), fsmode=dict(c=cfg(fsmode=1)))
    for name, kw in invalid.items():
        rc, out = host(**kw)
        assert rc == -1 and untouched(out), name
        assert lib.lc_last_error(ctx.h), name
    for name, kw in unsupported.items():
        rc, out = host(**kw)
        assert rc == -3 and untouched(out), name
    rc, out = host()
    assert rc == 0 and not CF.same(dict(crmask=out[0].astype(bool), clean=out[1], iters=out[2]), CF.wanted(d))

    with FrameSet(d, ctx) as fs:
        def frames(n=K, frame=np.arange(K, dtype=np.int32), t=None, rms=None, from_rms=0, c=good, apply=0, scratch=0, outs=True):
            out = outputs()
            rc = lib.lc_frames_detect_cosmics(fs.h, n, p(frame, _ip), p(t, _lib.fp), p(rms, _lib.fp), from_rms, None,
                                              None if c is None else C.byref(c), apply, scratch,
                                              p(out[0], _u8) if outs else None, p(out[1], _lib.fp) if outs else None,
                                              p(out[2], _ip) if outs else None, p(out[3], _ip) if outs else None, None)
            return rc, out

        ones = np.ones(K, np.float32)
        invalid = dict(n_zero=dict(n=0), n_negative=dict(n=-1), no_frame=dict(frame=None), no_cfg=dict(c=None),
                       frame_low=dict(frame=np.array([0, -1], np.int32)), frame_high=dict(frame=np.array([K, 0], np.int32)),
                       no_output_no_apply=dict(outs=False), apply_3=dict(apply=3), apply_negative=dict(apply=-1),
                       twice_nan=dict(frame=np.array([1, 1], np.int32), apply=1),
                       twice_clean=dict(frame=np.array([0, 0], np.int32), apply=2), scratch_negative=dict(scratch=-1),
                       rms_of_a_raw_set=dict(from_rms=1), rms_without_exptime=dict(from_rms=1, rms=ones),
                       exptime_zero=dict(from_rms=1, rms=ones, t=np.array([1.0, 0.0], np.float32)),
                       **{k: dict(c=v) for k, v in bad_settings.items()})
        for name, kw in invalid.items():
            rc, out = frames(**kw)
            assert rc == -1 and untouched(out), name
            assert lib.lc_last_error(ctx.h), name
        rc, out = frames(c=cfg(sepmed=0))
        assert rc == -3 and untouched(out)
        assert np.array_equal(CF.bits(fs.planes()), CF.bits(d))                 # no refused call applied anything
        rc, out = frames(frame=np.array([1, 1], np.int32))                      # a frame twice is fine without apply
        assert rc == 0 and np.array_equal(out[0][0], out[0][1])
        rc, out = frames(apply=1, outs=False)                                   # apply alone is a result
        assert rc == 0 and untouched(out)


# ---- 4. co-add -------------------------------------------------------------------------------------------------------------------------
def test_coadd_frames_rejects_the_cosmics(ctx):
    """Four registered frames (identity and small shifts), hits in frame 2, combine = 'mean', order = 1.  With
    reject_cosmics = {} the flagged pixels are NaN in the planes, so every output pixel with a flagged pixel among its four
    bilinear taps loses exactly that sample; the result is the co-add of a set whose flagged pixels (the restatement's) were
    set to NaN on the host, bit for bit."""
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.coaddition import coadd_frames
    h, w = 60, 75
    d = CF.sky((4, h, w), 51)
    for y, x in ((10, 12), (30, 47), (31, 48), (50, 70)):
        d[2, y, x] += 3000.0
    shifts = [(0.0, 0.0), (1.0, -2.0), (0.37, 1.62), (-1.25, 0.5)]
    results = [dict(success=True, transform=np.array([[1.0, 0.0, sx], [0.0, 1.0, sy], [0.0, 0.0, 1.0]])) for sx, sy in shifts]
    want = CF.wanted(d)
    cr = want['crmask']
    assert cr[2, 10, 12] and cr[2, 30, 47] and cr[2, 50, 70] and not cr[[0, 1, 3]].any()
    kw = dict(combine='mean', order=1)
    with FrameSet(d, ctx) as fs:
        plain = coadd_frames(fs, results, **kw)
        none = coadd_frames(fs, results, reject_cosmics=None, **kw)
        for key in ('image', 'weight', 'count', 'n_rejected'):
            assert np.array_equal(CF.bits(plain[key]), CF.bits(none[key])), key
        assert np.array_equal(CF.bits(fs.planes()), CF.bits(d))
        clean = coadd_frames(fs, results, reject_cosmics={}, **kw)
        assert np.array_equal(np.isnan(fs.planes()), cr)                        # the planes keep the NaNs
    holes = d.copy()
    holes[cr] = np.nan
    with FrameSet(holes, ctx) as fs:
        ref = coadd_frames(fs, results, **kw)
    for key in ('image', 'weight', 'count', 'n_rejected'):
        assert np.array_equal(CF.bits(clean[key]), CF.bits(ref[key])), key
    # the footprint: output pixel (i, j) reads frame 2 at the taps floor(j + sx) + {0, 1}, floor(i + sy) + {0, 1}
    sx, sy = shifts[2]
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    fx, fy = np.floor(jj + sx).astype(int), np.floor(ii + sy).astype(int)
    inside = (fx >= 0) & (fx <= w - 2) & (fy >= 0) & (fy <= h - 2)
    fxc, fyc = np.clip(fx, 0, w - 2), np.clip(fy, 0, h - 2)
    taps = cr[2][fyc, fxc] | cr[2][fyc, fxc + 1] | cr[2][fyc + 1, fxc] | cr[2][fyc + 1, fxc + 1]
    footprint = inside & taps
    assert footprint.sum() >= 12
    assert np.array_equal(plain['count'] - clean['count'], footprint.astype(np.int32))
    # without the rejection the stack carries the hits: 3000 / 4 above the sky at the pixel that reads (30, 47)
    i, j = np.argwhere(footprint & (fyc == 30) & (fxc == 47))[0]
    assert plain['image'][i, j] - clean['image'][i, j] > 100.0
    assert abs(clean['image'][i, j] - 200.0) < 40.0
