"""lc_ccdmask_stamps and lc_mask_cutouts on the device against the float32 NumPy restatement of the SPEC
(tests/_ccdmask.py, DESIGN.md §5 "Bad rows and columns"): mask, rowcol, bad_cols and bad_rows exactly and sigma
numerically at every stamp-size class (even and odd, 36 KiB to 144 KiB of LDS planes, K = 1), the hand cases of the
column fill, lsigma, hsigma and ngood away from 9 / 9 / 5 (CM.settings_cases), the ccdproc-shaped shim, and
mask_cutout_batch against the two separate calls and through the chain mask_cutout_batch -> lc_prepare_stamps ->
build_psf_batch."""
import numpy as np
import pytest

from tests import _ccdmask as CM
from tests import _lacosmic as LA

pytestmark = pytest.mark.gpu

SIZES_K = [(8, 64), (16, 64), (24, 1), (25, 40), (32, 64), (33, 24), (64, 16), (65, 8), (128, 4)]
_wanted = {}


def _case(n, K):
    """Inputs and the restatement's outputs of one (n, K), computed once."""
    if (n, K) not in _wanted:
        d = CM.device_batch(n, K, seed=10 * n + K)
        _wanted[n, K] = d, CM.ccdmask(d)
    return _wanted[n, K]


@pytest.mark.parametrize('n,K', SIZES_K)
def test_equal_to_the_float32_restatement(ctx, n, K):
    from lightcurver_amd.ccdproc import ccdmask_stamps
    d, want = _case(n, K)
    filled = want['mask'] & ~want['mask4']
    lines = want['bad_cols'].sum() + want['bad_rows'].sum()
    got = ccdmask_stamps(d, ctx=ctx)
    print(f'n={n} K={K}: flagged {want["mask4"].sum()} / filled {filled.sum()} / lines {lines}, stamps with sigma NaN '
          f'{np.isnan(want["sigma"]).sum()} and 0 {(want["sigma"] == 0).sum()}, device mask {got["mask"].sum()}, kernel '
          f'{got["kernel_ms"]:.3f} ms')
    assert want['mask4'].any() and lines >= 1 and (filled.any() or n < 16)     # an all-False result cannot pass
    for key in ('mask', 'rowcol', 'bad_cols', 'bad_rows'):
        assert got[key].dtype == bool and np.array_equal(got[key], want[key]), key
    assert got['sigma'].dtype == np.float32
    assert np.array_equal(np.isnan(got['sigma']), np.isnan(want['sigma']))
    ok = ~np.isnan(want['sigma'])
    assert np.array_equal(got['sigma'][ok], want['sigma'][ok])


@pytest.mark.parametrize('n', [8, 16])
def test_short_gaps_by_hand_on_the_device(ctx, n):
    """The hand cases of tests/test_ccdmask_cpu.py::test_short_gaps_by_hand: NaN pixels are the flagged ones."""
    from lightcurver_amd.ccdproc import ccdmask, ccdmask_stamps
    M = np.zeros((n, n), bool)
    for c, lines in enumerate(((0, 2), (1, 7), (0, 7), (n - 8, n - 6, n - 1), (n - 6, n - 1), (n - 7, n - 1),
                               (n - 6, n - 2))):
        M[list(lines), c] = True
    want = np.zeros((n, n), bool)
    for c, lines in enumerate(((0, 1, 2), range(1, 8), (0, 7), range(n - 8, n), (n - 6, n - 1), range(n - 7, n),
                               (n - 6, n - 2))):
        want[list(lines), c] = True
    d = np.zeros((n, n), np.float32)
    d[M] = np.nan
    assert np.array_equal(CM.ccdmask(d)['mask'], want)
    got = ccdmask_stamps(d[None], ctx=ctx)
    assert np.array_equal(got['mask'][0], want) and np.isnan(got['sigma'][0])
    assert np.array_equal(got['bad_cols'][0], want[0] & want[-1]) and not got['bad_rows'].any()
    assert np.array_equal(ccdmask(d, findbadcolumns=True, ctx=ctx), want)
    assert np.array_equal(ccdmask(d, ctx=ctx), M)


def test_without_findbadcolumns_the_mask_is_that_of_the_threshold(ctx):
    from lightcurver_amd.ccdproc import ccdmask
    d, want = _case(32, 64)
    assert (want['mask'] & ~want['mask4']).any()
    got = ccdmask(d, ctx=ctx)
    assert got.dtype == bool and got.shape == d.shape and np.array_equal(got, want['mask4'])
    assert np.array_equal(ccdmask(d, findbadcolumns=True, ctx=ctx), want['mask'])


@pytest.mark.parametrize('n,K', CM.SETTINGS_SIZES)
def test_settings_other_than_the_defaults(ctx, n, K):
    """Every case of CM.settings_cases, all five outputs exactly, then through the ccdproc-shaped call with
    findbadcolumns both ways.  Each case changes the restatement's mask against the defaults
    (tests/test_ccdmask_cpu.py asserts that), so a kernel that ignored a threshold, swapped the two or ran the fill
    loop one line short or long fails here."""
    from lightcurver_amd.ccdproc import ccdmask, ccdmask_stamps
    d, base, cases = CM.settings_wanted(n, K)
    wrong = []
    for kw, want in cases:
        got = ccdmask_stamps(d, ctx=ctx, **kw)
        same = {key: bool(got[key].dtype == bool and np.array_equal(got[key], want[key]))
                for key in ('mask', 'rowcol', 'bad_cols', 'bad_rows')}
        same['sigma'] = bool(got['sigma'].dtype == np.float32 and np.array_equal(got['sigma'], want['sigma'], equal_nan=True))
        same['ccdmask(findbadcolumns=True)'] = np.array_equal(ccdmask(d, findbadcolumns=True, ctx=ctx, **kw), want['mask'])
        same['ccdmask()'] = np.array_equal(ccdmask(d, ctx=ctx, **kw), want['mask4'])
        print(f'n={n} K={K} {kw}: mask {want["mask"].sum()} / device {got["mask"].sum()} (defaults {base["mask"].sum()}), '
              f'filled {(want["mask"] & ~want["mask4"]).sum()}, lines {want["bad_cols"].sum() + want["bad_rows"].sum()} / '
              f'device {got["bad_cols"].sum() + got["bad_rows"].sum()}')
        if not all(same.values()):
            wrong.append((kw, [key for key, ok in same.items() if not ok]))
    assert not wrong, wrong


def test_single_stamp_calls_equal_the_batched_call(ctx):
    from lightcurver_amd.ccdproc import ccdmask
    d, want = _case(33, 24)
    for k in range(len(d)):
        m = ccdmask(d[k], findbadcolumns=True, ctx=ctx)
        assert m.shape == (33, 33) and np.array_equal(m, want['mask'][k])


def _cutouts(K, n, seed):
    """Star stamps with injected lines and injected cosmics, and their noise maps."""
    d, nm = CM.star_stamps(n, F=(K + 7) // 8, seed=seed)
    d, nm = d[:K], nm[:K]
    d, _, _ = CM.inject_lines(d, nm, np.random.default_rng(seed + 1))
    d, _ = LA.inject_cosmics(d, nm, np.random.default_rng(seed + 2), amp=(30.0, 50.0))
    return d, nm


def test_mask_cutout_batch_is_the_or_of_the_two_calls(ctx):
    from lightcurver_amd.ccdproc import ccdmask_stamps
    from lightcurver_amd.processes.cutout_making import mask_cosmics_batch, mask_cutout_batch
    params = dict(sigclip=4.5, sigfrac=0.3, objlim=5.0)
    for n, K in ((24, 40), (65, 6)):
        d, nm = _cutouts(K, n, seed=n)
        lines = ccdmask_stamps(d, ctx=ctx)['rowcol']
        cosmics = mask_cosmics_batch(d, nm, params, ctx=ctx)
        assert lines.any() and cosmics.any() and (cosmics & ~lines).any()
        assert np.array_equal(lines, CM.ccdmask(d)['rowcol'])
        both = mask_cutout_batch(d, nm, True, True, params, ctx=ctx)
        assert both.dtype == bool and np.array_equal(both, lines | cosmics)
        assert np.array_equal(mask_cutout_batch(d, nm, False, True, params, ctx=ctx), cosmics)
        assert np.array_equal(mask_cutout_batch(d, nm, True, False, params, ctx=ctx), lines)
        assert not mask_cutout_batch(d, nm, False, False, params, ctx=ctx).any()


def test_mask_cutout_batch_takes_mixed_sizes(ctx):
    from lightcurver_amd.processes.cutout_making import mask_cutout_batch
    params = dict(sigclip=4.5, sigfrac=0.3, objlim=5.0)
    d24, nm24 = _cutouts(5, 24, seed=3)
    d32, nm32 = _cutouts(3, 32, seed=4)
    want24 = mask_cutout_batch(d24, nm24, True, True, params, ctx=ctx)
    want32 = mask_cutout_batch(d32, nm32, True, True, params, ctx=ctx)
    order = [('a', 0), ('b', 0), ('a', 1), ('a', 2), ('b', 1), ('a', 3), ('b', 2), ('a', 4)]
    pick = lambda a, b: [(a if w == 'a' else b)[i] for w, i in order]
    got = mask_cutout_batch(pick(d24, d32), pick(nm24, nm32), True, True, params, ctx=ctx)
    assert all(np.array_equal(g, w) for g, w in zip(got, pick(want24, want32)))
    assert any(g.any() for g in got)


def test_mask_cutout_batch_feeds_prepare_stamps_and_build_psf(ctx):
    """mask_cutout_batch -> lc_prepare_stamps(bad=...) -> build_psf_batch gives the weights, masked counts and PSFs of
    the direct calls (ccdmask and detect_cosmics per stamp, as the reference calls them), bit for bit."""
    from lightcurver_amd.astroscrappy import detect_cosmics
    from lightcurver_amd.ccdproc import ccdmask
    from lightcurver_amd.processes.cutout_making import mask_cutout_batch
    from lightcurver_amd.processes.preprocessing import prepare_stamps
    from lightcurver_amd.starred.procedures.psf_routines import build_psf_batch
    F, S, n = 2, 4, 24
    d, nm = _cutouts(F * S, n, seed=11)
    params = dict(sigclip=4.5, sigfrac=0.3, objlim=5.0)
    mask = mask_cutout_batch(d, nm, True, True, params, ctx=ctx)
    direct = []
    for k in range(len(d)):
        m = ccdmask(d[k], findbadcolumns=True, ctx=ctx)
        lines = np.zeros((n, n), bool)
        lines[:, m[0] & m[-1]] = True
        lines[m[:, 0] & m[:, -1], :] = True
        direct.append(lines | detect_cosmics(d[k], invar=nm[k] ** 2, ctx=ctx, **params)[0])
    direct = np.stack(direct)
    assert np.array_equal(mask, direct) and mask.any() and mask.all(axis=1).any()     # at least one whole column

    out = prepare_stamps(d, noisemap=nm, bad=mask, ctx=ctx)
    ref = prepare_stamps(d, noisemap=nm, bad=direct, ctx=ctx)
    for key in ('data', 'noisemap', 'weight', 'masked_count'):
        assert np.array_equal(out[key].view(np.uint8), ref[key].view(np.uint8)), key
    assert np.all(out['weight'][mask] == 0)
    assert np.array_equal(out['masked_count'], mask.sum(axis=(1, 2)))

    def fit(prep):
        w = prep['weight'].reshape(F, S, n, n)
        return build_psf_batch(list(prep['data'].reshape(F, S, n, n)), list(prep['noisemap'].reshape(F, S, n, n)), 2,
                               masks=list(w > 0), n_iter_analytic=5, n_iter_adabelief=5, ctx=ctx)
    got, want = fit(out), fit(ref)
    for g, w in zip(got, want):
        assert np.all(np.isfinite(g['narrow_psf']))
        assert np.array_equal(g['narrow_psf'], w['narrow_psf']) and np.array_equal(g['full_psf'], w['full_psf'])


def test_library_refuses_what_is_not_built(ctx):
    import ctypes as C
    from lightcurver_amd import _lib
    lib = _lib.lib()
    u8 = C.POINTER(C.c_uint8)
    for field, value, n, rc_want in (('byblocks', 1, 16, -3), ('ncmed', 5, 16, -3), ('nlmed', 9, 16, -3), (None, 0, 7, -3),
                                     (None, 0, 129, -3), ('ngood', -1, 16, -1), ('lsigma', float('nan'), 16, -1)):
        cfg = _lib.CcdmaskCfg(7, 7, 9.0, 9.0, 5, 0, 1)
        if field:
            setattr(cfg, field, value)
        dd = np.zeros((1, n, n), np.float32)
        mm = np.zeros(dd.shape, np.uint8)
        rc = lib.lc_ccdmask_stamps(ctx.h, 1, n, _lib.ptr(dd), C.byref(cfg), mm.ctypes.data_as(u8), None, None, None,
                                   None, None)
        assert rc == rc_want, (field, n, rc)
        ccfg = _lib.CosmicsCfg(4.5, 0.3, 5.0, 1.0, 6.5, 65536.0, 4, 1, 0, 0)
        rc = lib.lc_mask_cutouts(ctx.h, 1, n, _lib.ptr(dd), _lib.ptr(dd), 1, 1, C.byref(ccfg), C.byref(cfg),
                                 mm.ctypes.data_as(u8), None)
        assert rc == rc_want, (field, n, rc)
    cfg = _lib.CcdmaskCfg(7, 7, 9.0, 9.0, 5, 0, 1)
    dd = np.zeros((1, 16, 16), np.float32)
    assert lib.lc_ccdmask_stamps(ctx.h, 1, 16, _lib.ptr(dd), C.byref(cfg), None, None, None, None, None, None) == -1
