"""Optional outputs of the stamp-level entry points (csrc/device_call.h: a null host pointer gives a null device pointer,
no buffer and no copy).  lc_prepare_stamps, lc_detect_cosmics, lc_ccdmask_stamps and lc_segment_stamps are called through
ctypes once with every output requested and once per output with only that output (and, for cosmics and segment, the
mandatory mask): each output of a partial call is byte-equal to the one of the full call, with kernel_ms null and
non-null.  K = 3 stamps of 8 and 16 pixels, for cosmics also 72 (the planes in global scratch, above 64)."""
import ctypes as C

import numpy as np
import pytest

from tests import _ccdmask as CM
from tests import _lacosmic as LA

pytestmark = pytest.mark.gpu

K = 3
_inputs = {}


def _stamps(n):
    """K star stamps of make_psf_dataset with an injected column each (and a row on the odd one) and injected cosmics,
    their noise maps, and the pixels the cosmics hit; computed once per size."""
    if n not in _inputs:
        d, nm = CM.star_stamps(n, F=1, S=8, seed=n)
        d, nm = d[:K], np.ascontiguousarray(nm[:K])
        d, _, _ = CM.inject_lines(d, nm, np.random.default_rng(n + 1), depth=1000.0)   # found even in 8 x 8 stamps
        d, hit = LA.inject_cosmics(d, nm, np.random.default_rng(n + 2), amp=(30.0, 50.0))
        for a in (d, nm, hit):
            a.setflags(write=False)
        _inputs[n] = np.ascontiguousarray(d), nm, hit
    return _inputs[n]


def _p(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


_CTYPE = {np.dtype(np.float32): C.c_float, np.dtype(np.uint8): C.c_uint8, np.dtype(np.int32): C.c_int32}


def _run(ctx, name, call, spec, want, timed, fill):
    """One call with the outputs named in `want`; the others are passed as null.  call(pointers, kernel_ms) -> rc."""
    outs = {k: np.full(shape, fill, dtype) if k in want else None for k, (shape, dtype) in spec.items()}
    ms = C.c_float(-1.0)
    ctx.check(call({k: _p(a, _CTYPE[np.dtype(spec[k][1])]) for k, a in outs.items()}, C.byref(ms) if timed else None), name)
    assert (ms.value >= 0.0) if timed else (ms.value == -1.0)
    return outs


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _each_output_alone(ctx, name, call, spec, mandatory=()):
    """-> the outputs of the full call, after comparing every partial call with it.  The full call's buffers start from
    another fill value than the partial calls', so equal bytes are bytes both calls wrote."""
    full = _run(ctx, name, call, spec, set(spec), True, 0x55)
    untimed = _run(ctx, name, call, spec, set(spec), False, 0x33)
    for k in spec:
        assert np.array_equal(_bytes(untimed[k]), _bytes(full[k])), (name, k, 'kernel_ms null')
    for i, k in enumerate(spec):
        one = _run(ctx, name, call, spec, {k, *mandatory}, i % 2 == 0, 0xAA)
        for got in {k, *mandatory}:
            assert np.array_equal(_bytes(one[got]), _bytes(full[got])), (name, 'only', k, 'compared', got)
    return full


@pytest.mark.parametrize('mode', ['noisemap', 'rms_exptime'])
@pytest.mark.parametrize('n', [8, 16])
def test_prepare_stamps(ctx, n, mode):
    from lightcurver_amd import _lib
    lib = _lib.lib()
    d, nm, hit = _stamps(n)
    bad = hit.astype(np.uint8)
    rms = np.median(nm.reshape(K, -1), axis=1).astype(np.float32)
    exptime = np.array([60.0, 90.0, 120.0], np.float32)
    coef = np.array([1.0, 0.97, 1.04], np.float32)
    given = (_lib.ptr(nm), None, None) if mode == 'noisemap' else (None, _lib.ptr(rms), _lib.ptr(exptime))
    spec = dict(data=((K, n, n), np.float32), noisemap=((K, n, n), np.float32), weight=((K, n, n), np.float32),
                masked_count=((K,), np.int32))

    def call(o, ms):
        return lib.lc_prepare_stamps(ctx.h, K, n * n, _lib.ptr(d), *given, _lib.ptr(coef), _p(bad, C.c_uint8), 1.0e7,
                                     1000.0, 0, o['data'], o['noisemap'], o['weight'], o['masked_count'], ms)
    full = _each_output_alone(ctx, 'lc_prepare_stamps', call, spec)
    assert bad.any() and np.array_equal(full['masked_count'], bad.sum(axis=(1, 2)))
    assert np.all(full['weight'][hit] == 0) and (full['weight'] > 0).any()


@pytest.mark.parametrize('n', [8, 16, 72])
def test_detect_cosmics(ctx, n):
    from lightcurver_amd import _lib
    lib = _lib.lib()
    d, nm, hit = _stamps(n)
    invar = np.ascontiguousarray(nm ** 2)
    cfg = _lib.CosmicsCfg(4.5, 0.3, 5.0, 1.0, 6.5, 65536.0, 4, 1, 0, 0)
    spec = dict(crmask=((K, n, n), np.uint8), clean=((K, n, n), np.float32), iters=((K,), np.int32))

    def call(o, ms):
        return lib.lc_detect_cosmics(ctx.h, K, n, _lib.ptr(d), _lib.ptr(invar), None, C.byref(cfg), o['crmask'], o['clean'],
                                     o['iters'], ms)
    full = _each_output_alone(ctx, 'lc_detect_cosmics', call, spec, mandatory=('crmask',))
    assert full['crmask'].any() and set(np.unique(full['crmask'])) <= {0, 1}
    assert np.array_equal(full['crmask'].astype(bool), LA.lacosmic(d, invar=invar)['crmask'])


@pytest.mark.parametrize('n', [8, 16])
def test_ccdmask_stamps(ctx, n):
    from lightcurver_amd import _lib
    lib = _lib.lib()
    d, _, _ = _stamps(n)
    cfg = _lib.CcdmaskCfg(7, 7, 9.0, 9.0, 5, 0, 1)
    spec = dict(mask=((K, n, n), np.uint8), rowcol=((K, n, n), np.uint8), bad_cols=((K, n), np.uint8),
                bad_rows=((K, n), np.uint8), sigma=((K,), np.float32))

    def call(o, ms):
        return lib.lc_ccdmask_stamps(ctx.h, K, n, _lib.ptr(d), C.byref(cfg), o['mask'], o['rowcol'], o['bad_cols'],
                                     o['bad_rows'], o['sigma'], ms)
    full = _each_output_alone(ctx, 'lc_ccdmask_stamps', call, spec)
    want = CM.ccdmask(d)
    for k in ('mask', 'rowcol', 'bad_cols', 'bad_rows'):
        assert full[k].any() and np.array_equal(full[k].astype(bool), want[k]), k


@pytest.mark.parametrize('n', [8, 16])
def test_segment_stamps(ctx, n):
    from lightcurver_amd import _lib
    lib = _lib.lib()
    d, nm, _ = _stamps(n)
    cfg = _lib.SegmentCfg(3.0, 5, 32, 0.001, 1.0, 1)
    spec = dict(mask=((K, n, n), np.uint8), segmap=((K, n, n), np.int32), nobj=((K,), np.int32),
                xy=((K, _lib.SEGMENT_MAX_OBJECTS, 2), np.float32), status=((K,), np.int32))

    def call(o, ms):
        return lib.lc_segment_stamps(ctx.h, K, n, _lib.ptr(d), _lib.ptr(nm), C.byref(cfg), o['mask'], o['segmap'], o['nobj'],
                                     o['xy'], o['status'], ms)
    full = _each_output_alone(ctx, 'lc_segment_stamps', call, spec, mandatory=('mask',))
    assert full['mask'].any() and not full['mask'].all() and full['segmap'].any() and full['nobj'].any() and not full['status'].any()
