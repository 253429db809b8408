"""The kernel tables at subsampling 1 (host-side look-ups: no GPU): which stamp sizes have a PSF-fit / joint-fit kernel of
their own, which size every other even stamp is embedded in, and that the tables at subsampling 2 and the set of sizes with
a per-star-background batch are what they were."""
import pytest

from lightcurver_amd import _lib
from lightcurver_amd.joint import background_batch_supported, joint_fit_size
from lightcurver_amd.starred.procedures.psf_routines import _fit_size

PSF_NATIVE_SS1 = [16, 32, 64]
JOINT_NATIVE_SS1 = [16, 24, 32, 40, 48, 56, 64, 128]


def test_psf_sizes_at_subsampling_1():
    l = _lib.lib()
    for n in (16, 32, 64):
        assert l.lc_psf_supported(n, 1) == 1, n
    native = [n for n in range(2, 130, 2) if l.lc_psf_supported(n, 1)]
    assert native == PSF_NATIVE_SS1
    for n in range(8, 66, 2):
        m = _fit_size(n, 1)
        assert m in native and m >= n and (m - n) % 2 == 0 and (m == n) == (n in native)
        assert all(k < n for k in native if k < m)          # the smallest one that holds the stamp
    for n in (66, 15, 21, 33):
        with pytest.raises(_lib.LcError):
            _fit_size(n, 1)
    with pytest.raises(_lib.LcError):
        _fit_size(20, 3)


def test_joint_sizes_at_subsampling_1():
    l = _lib.lib()
    for n in (16, 24, 32, 64, 128):
        assert l.lc_joint_supported(n, 1) == 1, n
    native = [n for n in range(2, 130, 2) if l.lc_joint_supported(n, 1)]
    assert native == JOINT_NATIVE_SS1
    for n in range(10, 130, 2):
        m = joint_fit_size(n, 1)
        assert m in native and m >= n and (m - n) % 2 == 0 and (m == n) == (n in native)
        assert all(k < n for k in native if k < m)
    for n in (130, 21, 33, 127):
        with pytest.raises(_lib.LcError):
            joint_fit_size(n, 1)
    with pytest.raises(_lib.LcError):
        joint_fit_size(20, 3)


def test_tables_at_subsampling_2_are_unchanged():
    l = _lib.lib()
    assert [n for n in range(2, 130, 2) if l.lc_psf_supported(n, 2)] == [16, 24, 32, 64]
    assert [n for n in range(2, 130, 2) if l.lc_joint_supported(n, 2)] == [16, 24, 32, 40, 48, 56, 64, 128]
    assert not any(l.lc_psf_supported(n, ss) or l.lc_joint_supported(n, ss) for ss in (0, 3, 4) for n in range(2, 130))
    assert not any(l.lc_psf_supported(n, ss) or l.lc_joint_supported(n, ss) for ss in (1, 2) for n in range(1, 130, 2))


def test_background_batch_sizes_are_unchanged():
    l = _lib.lib()
    got = {(n, ss) for ss in (1, 2) for n in range(2, 130, 2) if l.lc_joint_groups_background_supported(n, ss)}
    assert got == {(16, 2), (24, 2), (32, 2), (16, 1)}
    assert all(background_batch_supported(n, ss) == ((n, ss) in got) for ss in (1, 2) for n in range(2, 130, 2))
