"""lc_segment_stamps on the device against the NumPy restatement of the SPEC (tests/_segment.py, DESIGN.md §5 "Source
masking"): mask, segmap, nobj, status and the float32 barycentres bit for bit at every stamp-size class; every
setting away from its default (SG.SETTINGS); the full table; single against batched calls; mixed sizes; the host route
for large stamps; the chain into the PSF fit."""
import ctypes as C

import numpy as np
import pytest

from tests import _segment as SG

pytestmark = pytest.mark.gpu

SIZES_K = [(8, 64), (16, 200), (24, 300), (25, 60), (32, 200), (33, 40), (63, 24), (64, 60)]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check(got, want):
    assert np.array_equal(got['status'], want['status'])
    assert np.array_equal(got['nobj'], want['nobj'])
    assert got['segmap'].dtype == np.int32 and np.array_equal(got['segmap'], want['segmap'])
    assert got['mask'].dtype == bool and np.array_equal(got['mask'], want['mask'])
    assert _same(got['xy'], want['xy'])


@pytest.mark.parametrize('n,K', SIZES_K)
def test_bit_equal_to_the_restatement(ctx, n, K):
    from lightcurver_amd.processes.source_masking import segment_batch
    d, s, kinds = SG.make_scenes(K, n, seed=100 * n + K)
    want = SG.segment(d, s)
    got = segment_batch(d, s, ctx=ctx)
    P = want['paths']
    took = dict(split=sum(p['split'] for p in P), deeper=sum(p['depth'] >= 2 for p in P),
                merged=sum(p['merged'] > 0 for p in P), zero=sum(p['zero'] for p in P),
                masked=int((~want['mask']).any(axis=(1, 2)).sum()))
    print(f'n={n} K={K}: objects {np.bincount(want["nobj"]).tolist()}, paths {took}, device status '
          f'{np.bincount(got["status"]).tolist()}, kernel {got["kernel_ms"]:.3f} ms')
    assert np.all(want['status'] == 0) and took['zero'] > 0
    if n >= 16:    # (an 8 x 8 stamp holds one object: nothing to split there)
        assert took['split'] > 0 and took['deeper'] > 0 and took['masked'] > 0
    if n in (24, 32):
        assert took['merged'] > 0
    _check(got, want)


@pytest.mark.parametrize('n,K', SG.SETTINGS_SIZES)
def test_settings_other_than_the_defaults(ctx, n, K):
    """Every case of SG.SETTINGS at this size, bit for bit.  Each changes the restatement's segmap against its base and
    against the defaults (tests/test_segment_cpu.py asserts that), so a kernel that ignored a setting fails here."""
    from lightcurver_amd.processes.source_masking import segment_batch
    wrong = []
    for kw, d, s, want, base, plain in SG.settings_wanted(n, K):
        args = {('clean_detections' if key == 'clean' else key): v for key, v in kw.items()}
        got = segment_batch(d, s, ctx=ctx, **args)
        same = dict(status=np.array_equal(got['status'], want['status']), nobj=np.array_equal(got['nobj'], want['nobj']),
                    segmap=got['segmap'].dtype == np.int32 and np.array_equal(got['segmap'], want['segmap']),
                    mask=got['mask'].dtype == bool and np.array_equal(got['mask'], want['mask']),
                    xy=_same(got['xy'], want['xy']))
        print(f'n={n} K={K} {kw}: objects {np.bincount(want["nobj"]).tolist()} / device {np.bincount(got["nobj"]).tolist()} '
              f'(base {np.bincount(base["nobj"]).tolist()}), device status {np.bincount(got["status"]).tolist()}')
        if not all(same.values()):
            wrong.append((kw, [key for key, ok in same.items() if not ok]))
    assert not wrong, wrong


def test_full_table_is_reported_and_leaves_the_batch_untouched(ctx):
    """49 separate objects in one 64 x 64 stamp: more than the 32 the table holds.  status 1, an all-good mask, and the
    stamps around it in the batch as if it were not there."""
    from lightcurver_amd.processes.source_masking import segment_batch
    d, s, _ = SG.make_scenes(4, 64, seed=77)
    cd, cs = SG.crowded_stamp(64)
    full_d, full_s = np.concatenate([d[:2], cd[None], d[2:]]), np.concatenate([s[:2], cs[None], s[2:]])
    want = SG.segment(full_d, full_s)
    assert want['status'].tolist() == [0, 0, 1, 0, 0]
    got = segment_batch(full_d, full_s, ctx=ctx)
    _check(got, want)
    assert got['mask'][2].all() and got['nobj'][2] == 0 and not got['segmap'][2].any()
    alone = segment_batch(d, s, ctx=ctx)
    for key in ('mask', 'segmap', 'nobj', 'xy', 'status'):
        assert np.array_equal(np.delete(got[key], 2, axis=0), alone[key]), key


def test_single_stamp_calls_equal_the_batched_call(ctx):
    from lightcurver_amd.processes.source_masking import extract_batch, segment_batch
    d, s, _ = SG.make_scenes(16, 33, seed=5)
    got = segment_batch(d, s, ctx=ctx)
    pairs = extract_batch(d, s, ctx=ctx)
    assert (got['nobj'] >= 2).any()
    for k in range(len(d)):
        one = segment_batch(d[k:k + 1], s[k:k + 1], ctx=ctx)
        for key in ('mask', 'segmap', 'nobj', 'xy', 'status'):
            assert np.array_equal(one[key][0], got[key][k]), (k, key)
        objects, seg = pairs[k]
        assert len(objects) == got['nobj'][k] and np.array_equal(seg, got['segmap'][k])
        assert np.array_equal(objects['npix'], np.bincount(seg.ravel(), minlength=len(objects) + 1)[1:])
        assert np.array_equal(objects['x'].astype(np.float32), got['xy'][k, :len(objects), 0])


def test_mixed_sizes_equal_the_per_size_calls_and_66_goes_through_the_host(ctx):
    from lightcurver_amd.processes.psf_modelling import mask_surrounding_stars, mask_surrounding_stars_batch
    sets = {n: SG.make_scenes(8, n, seed=n) for n in (24, 32, 66)}
    ds = [sets[n][0][k] for k in range(8) for n in (32, 66, 24)]
    ns = [sets[n][1][k] for k in range(8) for n in (32, 66, 24)]
    masks, n_host = mask_surrounding_stars_batch(ds, ns, ctx=ctx)
    assert isinstance(masks, list) and n_host == 8
    per = {n: mask_surrounding_stars_batch(sets[n][0], sets[n][1], ctx=ctx) for n in (24, 32)}
    assert per[24][1] == 0 and per[32][1] == 0 and per[24][0].shape == (8, 24, 24) and per[24][0].dtype == bool
    assert any((~m).any() for m in masks)
    for i, m in enumerate(masks):
        k, n = i // 3, (32, 66, 24)[i % 3]
        want = per[n][0][k] if n != 66 else mask_surrounding_stars(sets[66][0][k], sets[66][1][k])
        assert m.dtype == bool and np.array_equal(m, want), (k, n)
    alone, cnt = mask_surrounding_stars_batch(sets[66][0][:2], sets[66][1][:2], ctx=ctx)
    assert cnt == 2 and alone.shape == (2, 66, 66)


def _frames_with_neighbours(seed):
    """3 frames x 4 stars x 32^2 of make_psf_dataset, a bright neighbour injected into every stamp."""
    from lightcurver_amd.synthetic import make_psf_dataset
    F, S, n = 3, 4, 32
    ds = make_psf_dataset(F=F, S=S, n=n, seed=seed)
    d, nm = ds['data'].astype(np.float32).copy(), ds['noisemap'].astype(np.float32).copy()
    rng = np.random.default_rng(seed + 1)
    cores = np.zeros(d.shape, bool)
    for f in range(F):
        for j in range(S):
            x0, y0 = (25, 9) if (f + j) % 2 else (6, 24)
            amp = 150.0 * float(np.median(nm[f, j]))
            star = SG._star(n, x0 + rng.uniform(-0.3, 0.3), y0 + rng.uniform(-0.3, 0.3), amp, 1.6)
            d[f, j] += star.astype(np.float32)
            nm[f, j] = np.sqrt(nm[f, j] ** 2 + np.float32(0.01) * star.astype(np.float32) * np.median(nm[f, j]))
            cores[f, j, y0 - 1:y0 + 2, x0 - 1:x0 + 2] = True
    return d, nm, cores


def test_chain_from_the_masks_into_the_psf_fit(ctx):
    """mask_cosmics_batch -> mask_surrounding_stars_batch -> prepare_psf_stamps_batched(automatic_masks=...) ->
    build_psf_batch: the PSF bits of the same chain fed the restatement's masks; the neighbours' cores carry no weight."""
    from lightcurver_amd.processes.cutout_making import mask_cosmics_batch
    from lightcurver_amd.processes.psf_modelling import mask_surrounding_stars_batch, prepare_psf_stamps_batched
    from lightcurver_amd.starred.procedures.psf_routines import build_psf_batch
    d, nm, cores = _frames_with_neighbours(21)
    F, S, n = d.shape[:3]
    cm = mask_cosmics_batch(d.reshape(-1, n, n), nm.reshape(-1, n, n), dict(sigclip=4.5, sigfrac=0.3, objlim=5.0), ctx=ctx)
    am, n_host = mask_surrounding_stars_batch(d.reshape(-1, n, n), nm.reshape(-1, n, n), ctx=ctx)
    want = SG.segment(d.reshape(-1, n, n), nm.reshape(-1, n, n))
    assert n_host == 0 and np.all(want['status'] == 0)
    assert np.array_equal(am, want['mask']) and not am.reshape(d.shape)[cores].any()

    def run(auto):
        frames = [dict(datas=d[f], noisemaps=nm[f], cosmics_masks=cm.reshape(d.shape)[f],
                       automatic_masks=auto.reshape(d.shape)[f]) for f in range(F)]
        prep = prepare_psf_stamps_batched(frames)
        for f, (_, _, good, keep) in enumerate(prep):
            assert keep.all() and not good[cores[f]].any()
        return build_psf_batch([p[0] for p in prep], [p[1] for p in prep], 2, masks=[p[2] for p in prep],
                               n_iter_analytic=5, n_iter_adabelief=5, ctx=ctx)
    got, ref = run(am), run(want['mask'])
    for g, w in zip(got, ref):
        assert np.all(np.isfinite(g['narrow_psf']))
        assert np.array_equal(g['narrow_psf'], w['narrow_psf']) and np.array_equal(g['full_psf'], w['full_psf'])


def test_model_psfs_of_frames_masks_the_neighbours_on_request(ctx):
    from lightcurver_amd.processes.psf_modelling import mask_surrounding_stars_batch, model_psfs_of_frames
    d, nm, cores = _frames_with_neighbours(31)
    F, S, n = d.shape[:3]
    none = np.zeros((S, n, n), bool)
    frames = [dict(datas=d[f], noisemaps=nm[f], cosmics_masks=none) for f in range(F)]
    am, _ = mask_surrounding_stars_batch(d.reshape(-1, n, n), nm.reshape(-1, n, n), ctx=ctx)
    assert not am.reshape(d.shape)[cores].any()
    masked = [dict(fr, automatic_masks=am.reshape(d.shape)[f]) for f, fr in enumerate(frames)]
    kw = dict(psf_n_iter_analytic=5, psf_n_iter_pixels=5)
    on = model_psfs_of_frames(frames, mask_neighbours=True, **kw)
    given = model_psfs_of_frames(masked, **kw)
    off = model_psfs_of_frames(frames, mask_neighbours=False, **kw)
    today = model_psfs_of_frames(frames, **kw)
    differs = False
    for (fa, a), (_, b), (_, c), (_, e), fr in zip(on, given, off, today, frames):
        assert fa is fr
        for key in ('narrow_psf', 'full_psf'):
            assert np.array_equal(a[key], b[key]) and np.array_equal(c[key], e[key])
        differs |= not np.array_equal(a['full_psf'], c['full_psf'])
    assert differs
    # a frame that brings its masks keeps them
    mixed = [masked[0]] + frames[1:]
    again = model_psfs_of_frames(mixed, mask_neighbours=True, **kw)
    assert all(np.array_equal(x[1]['full_psf'], y[1]['full_psf']) for x, y in zip(again, on))


def test_library_refuses_what_is_not_built(ctx):
    from lightcurver_amd import _lib
    lib = _lib.lib()
    u8 = C.POINTER(C.c_uint8)
    cases = [(None, 0, 7), (None, 0, 65), ('clean_param', 2.0, 16), ('deblend_nthresh', 12, 16),
             ('deblend_nthresh', 64, 16), ('minarea', 0, 16)]
    for field, value, n in cases:
        cfg = _lib.SegmentCfg(3.0, 15, 32, 0.001, 1.0, 1)
        if field:
            setattr(cfg, field, value)
        dd = np.zeros((1, n, n), np.float32)
        mm = np.zeros(dd.shape, np.uint8)
        rc = lib.lc_segment_stamps(ctx.h, 1, n, _lib.ptr(dd), _lib.ptr(dd + 1), C.byref(cfg), mm.ctypes.data_as(u8), None,
                                   None, None, None, None)
        assert rc == -3, (field, value, n, rc)
