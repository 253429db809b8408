"""lc_detect_cosmics on the device against the float32 NumPy restatement of the SPEC (tests/_lacosmic.py, DESIGN.md §5
"Cosmic-ray detection"): crmask, clean and iters bit for bit, both median modes, every stamp-size class (LDS planes up
to 64, global planes above, odd sizes), with and without invar, with inmask, NaN borders and saturated cores; then the
single-stamp form against the batched one, the chain mask_cosmics_batch -> lc_prepare_stamps -> build_psf_batch, and every
setting away from its default (LA.SETTINGS), also as cosmics_masking_params through mask_cutout_batch."""
import numpy as np
import pytest

from tests import _lacosmic as LA

pytestmark = pytest.mark.gpu

SIZES_K = [(8, 800), (16, 300), (24, 1), (25, 120), (32, 200), (33, 80), (64, 40), (65, 24), (128, 6)]


_stamps = LA.star_stamps        # the inputs, shared with the settings lists of tests/_lacosmic.py


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('sepmed', [True, False])
@pytest.mark.parametrize('with_invar', [True, False])
@pytest.mark.parametrize('n,K', SIZES_K)
def test_bit_equal_to_the_float32_restatement(ctx, n, K, with_invar, sepmed):
    from lightcurver_amd.astroscrappy import lacosmic
    d, nm, inmask, satlevel = _stamps(K, n, seed=10 * n + K, electrons=not with_invar)
    invar = nm ** 2 if with_invar else None
    gain = 1.0 if with_invar else 1.5
    kw = dict(invar=invar, inmask=inmask, satlevel=satlevel, gain=gain, sepmed=sepmed)
    want = LA.lacosmic(d, **kw)
    got = lacosmic(d, ctx=ctx, **kw)
    print(f'n={n} K={K} invar={with_invar} sepmed={sepmed}: flagged {want["crmask"].sum()} / device '
          f'{got["crmask"].sum()}, saturated-mask pixels {(want["mask"] & ~inmask & np.isfinite(d)).sum()}, '
          f'iters {np.bincount(want["iters"]).tolist()}, kernel {got["kernel_ms"]:.3f} ms')
    assert want['crmask'].any() or K < 8
    assert np.array_equal(got['crmask'], want['crmask'])
    assert _same(got['clean'], want['clean'].astype(np.float32))
    assert np.array_equal(got['iters'], want['iters'])


def test_bit_equal_at_8000_stamps_of_24(ctx):
    from lightcurver_amd.astroscrappy import lacosmic
    d, nm, inmask, satlevel = _stamps(8000, 24, seed=24, electrons=False)
    kw = dict(invar=nm ** 2, inmask=inmask, satlevel=satlevel)
    want = LA.lacosmic(d, **kw)
    got = lacosmic(d, ctx=ctx, **kw)
    print(f'8000 x 24^2: flagged {want["crmask"].sum()}, kernel {got["kernel_ms"]:.3f} ms')
    assert np.array_equal(got['crmask'], want['crmask'])
    assert _same(got['clean'], want['clean'].astype(np.float32))
    assert np.array_equal(got['iters'], want['iters'])


def test_stamp_without_good_neighbour_takes_the_stamp_median(ctx):
    """The meanmask fall-back (no good pixel in the 5 x 5 window) on the device."""
    from lightcurver_amd.astroscrappy import lacosmic
    rng = np.random.default_rng(3)
    d = (100.0 + 10.0 * rng.standard_normal((4, 32, 32))).astype(np.float32)
    inmask = np.zeros(d.shape, bool)
    for k in range(4):
        d[k, 16, 16] += 800.0
        inmask[k, 14:19, 14:19] = True
        inmask[k, 16, 16] = False
    want = LA.lacosmic(d, inmask=inmask)
    got = lacosmic(d, inmask=inmask, ctx=ctx)
    assert want['crmask'][:, 16, 16].all()
    assert np.array_equal(got['crmask'], want['crmask'])
    assert _same(got['clean'], want['clean'])
    assert np.array_equal(got['iters'], want['iters'])


def test_single_stamp_calls_equal_the_batched_call(ctx):
    from lightcurver_amd.astroscrappy import detect_cosmics
    d, nm, inmask, satlevel = _stamps(12, 33, seed=5, electrons=False)
    cr, clean = detect_cosmics(d, inmask=inmask, invar=nm ** 2, satlevel=satlevel, ctx=ctx)
    assert cr.shape == d.shape and cr.dtype == bool and clean.dtype == np.float32 and cr.any()
    for k in range(len(d)):
        c1, k1 = detect_cosmics(d[k], inmask=inmask[k], invar=nm[k] ** 2, satlevel=satlevel, ctx=ctx)
        assert c1.shape == (33, 33)
        assert np.array_equal(c1, cr[k]) and _same(k1, clean[k])


def test_mask_cosmics_batch_feeds_prepare_stamps_and_build_psf(ctx):
    """mask_cosmics_batch -> lc_prepare_stamps(bad=...) -> build_psf_batch gives the masks, weights and masked counts of
    the direct calls (one detect_cosmics per stamp, as the reference calls it), bit for bit; every injected cosmic
    pixel has zero weight."""
    from lightcurver_amd.astroscrappy import detect_cosmics
    from lightcurver_amd.processes.cutout_making import mask_cosmics_batch
    from lightcurver_amd.processes.preprocessing import prepare_stamps
    from lightcurver_amd.starred.procedures.psf_routines import build_psf_batch
    from lightcurver_amd.synthetic import make_psf_dataset
    F, S, n = 3, 4, 32
    ds = make_psf_dataset(F=F, S=S, n=n, seed=11)
    d = ds['data'].reshape(-1, n, n)
    nm = ds['noisemap'].reshape(-1, n, n)
    d, hit = LA.inject_cosmics(d, nm, np.random.default_rng(12), max_per_stamp=2, amp=(30.0, 50.0))
    # the inputs: bright tracks away from the stars' cores, so that every injected pixel is a detection
    params = dict(sigclip=4.5, sigfrac=0.3, objlim=5.0)
    assert hit.any() and np.all(LA.lacosmic(d, invar=nm ** 2, **params)['crmask'][hit])

    mask = mask_cosmics_batch(d, nm, params, ctx=ctx)
    direct = np.stack([detect_cosmics(d[k], invar=nm[k] ** 2, ctx=ctx, **params)[0] for k in range(len(d))])
    assert mask.dtype == bool and np.array_equal(mask, direct)
    listed = mask_cosmics_batch(list(d), list(nm), params, ctx=ctx)
    assert all(np.array_equal(a, b) for a, b in zip(listed, direct))

    out = prepare_stamps(d, noisemap=nm, bad=mask, ctx=ctx)
    ref = prepare_stamps(d, noisemap=nm, bad=direct, ctx=ctx)
    for key in ('data', 'noisemap', 'weight', 'masked_count'):
        assert _same(out[key], ref[key]), key
    assert np.all(out['weight'][hit] == 0)
    assert np.array_equal(out['masked_count'], mask.sum(axis=(1, 2)))

    def fit(prep):
        w = prep['weight'].reshape(F, S, n, n)
        return build_psf_batch(list(prep['data'].reshape(F, S, n, n)), list(prep['noisemap'].reshape(F, S, n, n)), 2,
                               masks=list(w > 0), n_iter_analytic=5, n_iter_adabelief=5, ctx=ctx)
    got, want = fit(out), fit(ref)
    for g, w in zip(got, want):
        assert np.all(np.isfinite(g['narrow_psf']))
        assert np.array_equal(g['narrow_psf'], w['narrow_psf']) and np.array_equal(g['full_psf'], w['full_psf'])


@pytest.mark.parametrize('n,K,with_invar,sepmed', LA.SETTINGS_INPUTS)
def test_settings_other_than_the_defaults(ctx, n, K, with_invar, sepmed):
    """Every case of LA.SETTINGS that applies to this input (LA.settings_cases), bit for bit.  Each changes the
    restatement's result against its base (tests/test_cosmics_cpu.py asserts that), so a kernel that ignored or mixed
    up a setting fails here.  With invar, readnoise is told apart through the invalid pixels alone, at sigclip 1; values
    far above the noise of every pixel (30 against 6.5 on the scaled stamps) are not told apart by any input we found,
    so 30 runs on the stamps in electrons there."""
    from lightcurver_amd.astroscrappy import lacosmic
    wrong = []
    for label, d, kw, want, base in LA.settings_wanted(n, K, with_invar, sepmed):
        got = lacosmic(d, ctx=ctx, **kw)
        same = (np.array_equal(got['crmask'], want['crmask']), _same(got['clean'], want['clean'].astype(np.float32)),
                np.array_equal(got['iters'], want['iters']))
        print(f'n={n} K={K} invar={with_invar} sepmed={sepmed} {label}: flagged {want["crmask"].sum()} / device '
              f'{got["crmask"].sum()} (base {base["crmask"].sum()}), iters {np.bincount(want["iters"]).tolist()} / device '
              f'{np.bincount(got["iters"]).tolist()}, crmask, clean, iters equal: {same}')
        if not all(same):
            wrong.append((label, same))
    assert not wrong, wrong


def test_configuration_path_takes_the_users_settings(ctx):
    """cosmics_masking_params as a user writes them in the configuration (a raised objlim, fewer iterations, the keys
    of fsmode='convolve' that have no effect) through mask_cutout_batch and mask_cosmics_batch: the restatement with
    those values, ORed with the row / column half where that is on."""
    from tests import _ccdmask as CM
    from lightcurver_amd.processes.cutout_making import mask_cosmics_batch, mask_cutout_batch
    user = dict(objlim=8, sigclip=3, niter=2)
    params = dict(user, verbose=False, psffwhm=2.5)
    sets = {}
    for n, K in ((24, 16), (65, 4)):
        d, nm = CM.star_stamps(n, F=(K + 7) // 8, seed=n + 40)
        d, nm = d[:K], nm[:K]
        d, _, _ = CM.inject_lines(d, nm, np.random.default_rng(n + 41))
        d, _ = LA.inject_cosmics(d, nm, np.random.default_rng(n + 42))
        cosmics = LA.lacosmic(d, invar=nm ** 2, **user)['crmask']
        lines = CM.ccdmask(d)['rowcol']
        assert not np.array_equal(cosmics, LA.lacosmic(d, invar=nm ** 2)['crmask'])       # the settings matter here
        assert cosmics.any() and lines.any() and (cosmics & ~lines).any()
        assert np.array_equal(mask_cutout_batch(d, nm, False, True, params, ctx=ctx), cosmics)
        assert np.array_equal(mask_cutout_batch(d, nm, True, True, params, ctx=ctx), cosmics | lines)
        assert np.array_equal(mask_cutout_batch(d, nm, True, False, params, ctx=ctx), lines)
        assert np.array_equal(mask_cosmics_batch(d, nm, params, ctx=ctx), cosmics)
        sets[n] = d, nm, cosmics | lines
    mixed = mask_cutout_batch([sets[24][0][0], sets[65][0][1], sets[24][0][2]],
                              [sets[24][1][0], sets[65][1][1], sets[24][1][2]], True, True, params, ctx=ctx)
    assert all(np.array_equal(m, w) for m, w in zip(mixed, (sets[24][2][0], sets[65][2][1], sets[24][2][2])))
    d, nm, _ = sets[24]
    assert params == dict(user, verbose=False, psffwhm=2.5)                               # the caller's dict is left alone
    for bad, err in ((dict(user, cleantype='median'), NotImplementedError), (dict(user, sigclipp=3.0), TypeError)):
        with pytest.raises(err):
            mask_cutout_batch(d, nm, True, True, bad, ctx=ctx)
        with pytest.raises(err):
            mask_cosmics_batch(d, nm, bad, ctx=ctx)


def test_library_refuses_what_is_not_built(ctx):
    import ctypes as C
    from lightcurver_amd import _lib
    lib = _lib.lib()
    d = np.zeros((1, 16, 16), np.float32)
    cr = np.zeros(d.shape, np.uint8)
    u8 = C.POINTER(C.c_uint8)
    for field, value, n in (('cleantype', 1, 16), ('fsmode', 1, 16), (None, 0, 7), (None, 0, 129)):
        cfg = _lib.CosmicsCfg(4.5, 0.3, 5.0, 1.0, 6.5, 65536.0, 4, 1, 0, 0)
        if field:
            setattr(cfg, field, value)
        dd = np.zeros((1, n, n), np.float32)
        cc = np.zeros(dd.shape, np.uint8)
        rc = lib.lc_detect_cosmics(ctx.h, 1, n, _lib.ptr(dd), None, None, C.byref(cfg), cc.ctypes.data_as(u8), None,
                                   None, None)
        assert rc == -3, (field, n, rc)
