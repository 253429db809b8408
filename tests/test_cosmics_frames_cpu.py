"""The frame form of the cosmic-ray kernels without a device: every input of tests/_cosmics_frames.py is held to the
property it is built to exercise, on the restatement (tests/_lacosmic.py) that is the device tests' yardstick, so that a
kernel cannot pass tests/test_cosmics_frames_gpu.py by luck; and the ABI and the Python signatures."""
import ctypes as C
import inspect

import numpy as np
import pytest

from tests import _cosmics_frames as CF
from tests import _lacosmic as LA


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ((40, 56), (65, 127)))
def test_fallback_input_takes_the_global_fallback(shape):
    d, inmask, (cy, cx) = CF.fallback_input(shape)
    r = CF.wanted(d, inmask=inmask)
    assert r['crmask'][0, cy, cx] and list(r['iters']) == [2]
    good = ~r['mask'][0] & ~r['crmask'][0]
    assert not good[cy - 2:cy + 3, cx - 2:cx + 3].any()                       # no good pixel in the 5 x 5 window
    want = LA.lower_median(np.float32(1.0) * d[0][good])
    print(shape, float(want))
    assert r['clean'][0, cy, cx] == want and 190.0 < want < 210.0
    # with every other pixel masked there is no good pixel at all: the value is 0
    r = CF.wanted(d, inmask=CF.all_but(d.shape, cy, cx))
    assert r['crmask'][0, cy, cx] and r['crmask'].sum() == 1 and r['clean'][0, cy, cx] == 0.0


def test_early_exit_input_stops_at_three_different_iterations():
    d = CF.early_exit_input()
    for kw in ({}, dict(invar=CF.model_invar(d))):
        r = CF.wanted(d, **kw)
        flagged = r['crmask'].reshape(3, -1).sum(axis=1)
        print(sorted(kw), r['iters'], flagged)
        assert list(r['iters']) == [1, 2, 4]
        assert flagged[0] == 0 and flagged[1] >= 1 and flagged[2] >= 49
        assert list(CF.wanted(d, niter=12, **kw)['iters']) == [1, 2, 12]
    assert CF.wanted(d, invar=CF.model_invar(d))['crmask'][2].sum() == 72


def test_straddling_input_crosses_every_tile_line():
    d, hit = CF.straddle_input()
    hits = CF.straddle_hits()
    assert len(hits) == 55 and hit.sum() == 220 and not hit[1].any()
    for step in (16, 32, 48, 64):                                               # a hit across every multiple, both ways
        for size, axis in ((200, 0), (261, 1)):
            lines = range(step, size - 16, step)
            assert all(any(p[axis] == line for p in hits) for line in lines), (step, axis)
    r = CF.wanted(d)
    assert r['crmask'][hit].all() and r['crmask'].sum() == 240
    assert list(r['iters']) == [2, 1] and not r['crmask'][1].any()


def test_saturated_and_nan_inputs():
    r = CF.wanted(CF.saturated_input())
    assert r['mask'].sum() == 80 and not r['crmask'].any()
    r = CF.wanted(CF.nan_columns_input())
    assert np.isfinite(r['clean']).all() and r['crmask'][0, 20, 50] and r['mask'][0, :, :5].all()


def test_settings_cases_differ_from_the_defaults_exactly_where_they_run():
    ran = set()
    for label, d, case, base in CF.settings_cases():
        ran.add(label)
        assert CF.same(CF.wanted(d, **case), CF.wanted(d, **base)), label
    assert len(ran) == 11
    # what is not run changes nothing on the straddling input
    d = CF.straddle_input()[0]
    inv = dict(invar=CF.model_invar(d))
    assert not CF.same(CF.wanted(d, objlim=1.0), CF.wanted(d))
    assert not CF.same(CF.wanted(d, objlim=1.0, **inv), CF.wanted(d, **inv))
    assert not CF.same(CF.wanted(d, readnoise=0.0, **inv), CF.wanted(d, **inv))


def test_plain_inputs_flag_their_hit():
    for shape in CF.SHAPES:
        d, (y, x) = CF.plain_input(shape)
        for kw in ({}, dict(invar=CF.model_invar(d))):
            r = CF.wanted(d, **kw)
            assert r['crmask'][0, y, x] and list(r['iters']) == [2, 1] and not r['crmask'][1].any(), shape


# ---- ABI and façade --------------------------------------------------------------------------------------------------------------
def test_supported_answers_without_a_device():
    from lightcurver_amd import _lib
    lib = _lib.lib()
    assert lib.lc_cosmics_frames_supported(8, 8) == 1 and lib.lc_cosmics_frames_supported(8, 9) == 1
    assert lib.lc_cosmics_frames_supported(7, 9) == 0 and lib.lc_cosmics_frames_supported(9, 7) == 0
    assert lib.lc_cosmics_frames_supported(46341, 46341) == 0 and lib.lc_cosmics_frames_supported(32768, 65535) == 1
    assert lib.lc_cosmics_frames_supported(32768, 65536) == 0
    assert lib.lc_cosmics_frames_supported(2048, 2048) == 1 and lib.lc_cosmics_frames_supported(4, 2048) == 0


def test_null_handles_are_refused():
    from lightcurver_amd import _lib
    lib = _lib.lib()
    d = np.zeros((1, 8, 8), np.float32)
    cr = np.zeros((1, 8, 8), np.uint8)
    cfg = _lib.CosmicsCfg(4.5, 0.3, 5.0, 1.0, 6.5, 65536.0, 4, 1, 0, 0)
    u8 = C.POINTER(C.c_uint8)
    assert lib.lc_detect_cosmics_frames(None, 1, 8, 8, _lib.ptr(d), None, None, C.byref(cfg), 0, cr.ctypes.data_as(u8),
                                        None, None, None, None) == -1
    frame = np.zeros(1, np.int32)
    assert lib.lc_frames_detect_cosmics(None, 1, frame.ctypes.data_as(C.POINTER(C.c_int32)), None, None, 0, None,
                                        C.byref(cfg), 0, 0, cr.ctypes.data_as(u8), None, None, None, None) == -1
    assert not cr.any()


def test_python_signatures():
    from lightcurver_amd.frames import FrameSet
    from lightcurver_amd.processes.coaddition import coadd_frames
    from lightcurver_amd import astroscrappy
    p = inspect.signature(FrameSet.detect_cosmics).parameters
    assert list(p) == ['self', 'frame_index', 'exptimes', 'background_rms', 'noise', 'inmask', 'apply',
                       'cosmics_masking_params', 'download', 'scratch_frames']
    want = dict(frame_index=None, exptimes=None, background_rms=None, noise=None, inmask=None, apply=None,
                cosmics_masking_params=None, download=('crmask',), scratch_frames=0)
    assert {k: p[k].default for k in want} == want
    q = inspect.signature(coadd_frames).parameters
    assert q['reject_cosmics'].default is None and 'NaN' in coadd_frames.__doc__
    r = inspect.signature(astroscrappy.lacosmic_frames).parameters
    assert [k for k in r][:3] == ['stack', 'inmask', 'invar'] and r['sepmed'].default is True and r['ctx'].default is None


def test_full_medians_are_refused_on_frames_before_any_device_call():
    from lightcurver_amd.astroscrappy import detect_cosmics, lacosmic_frames
    d = CF.sky((40, 56), 1)
    with pytest.raises(NotImplementedError, match='sepmed'):
        detect_cosmics(d, sepmed=False)
    with pytest.raises(NotImplementedError, match='sepmed'):
        lacosmic_frames(d[None], sepmed=False)
