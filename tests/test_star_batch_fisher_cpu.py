"""The batched star photometry's Fisher information with the shifts free (lc_joint_groups_fisher_shifts,
StarPhotometryBatch.fisher_shifts_per_star, do_many_stars_forward_modelling(marginalize_shifts=...)): what can be checked
without a device - the entry point is declared, exported and bound, the Python switches exist with their defaults, and the
refusals of the one-object calls on a batch stay as they were."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'lc_joint_groups_fisher_shifts'


def test_entry_point_is_declared_exported_and_bound():
    from lightcurver_amd import _lib
    with open(os.path.join(ROOT, 'include', 'lcmi.h')) as f:
        header = f.read()
    assert re.search(r'int\s+' + NAME + r'\s*\(\s*lc_joint\s*\*\s*j\s*,\s*int\s+flags\s*,\s*const\s+lc_fisher_shifts_out\s*\*\s*'
                     r'out\s*,\s*int32_t\s*\*\s*star_ok\s*\)\s*;', header)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    ret, args = _lib.SIGNATURES[NAME]
    assert ret is ctypes.c_int and len(args) == 4
    assert args[2] is _lib.SIGNATURES['lc_joint_fisher_shifts'][1][2]       # the same output structure
    assert args[3] is ctypes.POINTER(ctypes.c_int32)
    assert getattr(_lib.lib(), NAME).argtypes == list(args)


def test_step_function_has_the_switch_and_it_is_off():
    from lightcurver_amd.processes import star_photometry as S
    p = inspect.signature(S.do_many_stars_forward_modelling).parameters
    assert p['marginalize_shifts'].default is False
    assert list(p)[-1] == 'marginalize_shifts'                              # behind the existing arguments
    assert 'fluxes_uncertainties_marginal' in S.do_many_stars_forward_modelling.__doc__
    assert 'L-BFGS-B' in S.do_many_stars_forward_modelling.__doc__         # the one difference from the one-star function
    assert S.do_many_stars_forward_modelling([], 2, marginalize_shifts=True) == []


def test_batch_has_its_own_method_and_the_one_object_calls_still_refuse():
    from lightcurver_amd.joint import JointFit, StarPhotometryBatch
    p = inspect.signature(StarPhotometryBatch.fisher_shifts_per_star).parameters
    assert list(p) == ['self', 'mean'] and p['mean'].default is False
    assert not hasattr(JointFit, 'fisher_shifts_per_star')
    b = object.__new__(StarPhotometryBatch)                                 # no device: the refusals need none
    b.h = None
    with pytest.raises(NotImplementedError):
        b.fisher_shifts()
    with pytest.raises(NotImplementedError):
        b.fisher_positions()
