"""PSF stamps of a side other than the joint fit's grid, without a device: the NumPy form of the placement rule
(joint.place_psf) against the tests' own tap-by-tap statement of it (tests/_psf_place.py), the rule pinned to
fftconvolve(., ., 'same') through the float64 oracle, read_roi_file with the ROI file of the reference's default
configuration (48 x 48 PSFs beside 32 x 32 data), and the library's index function (csrc/joint_psf_place.h) in a
stand-alone host program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from lightcurver_amd.synthetic import make_narrow_psf, make_roi_dataset
from tests import _psf_place as PP
from tests.test_device_call_cpu import HOST, ROOT, _compiler

# (n, P, ss): the stamps of tests/test_joint_psf_size_gpu.py's model test that fit into the grid
IDENTITY_CASES = [(16, 8, 2), (16, 30, 2), (16, 31, 2), (16, 24, 2), (16, 9, 1), (64, 96, 2)]


@pytest.mark.parametrize('N,P', [(32, 1), (32, 8), (32, 31), (32, 32), (32, 33), (32, 48), (32, 200), (16, 9), (16, 24)])
def test_place_psf_is_the_rule(N, P):
    from lightcurver_amd.joint import place_psf, psf_flux_outside
    rng = np.random.default_rng(1000 * N + P)
    psf = rng.uniform(0.1, 1.0, size=(3, P, P)).astype(np.float32)
    got, want = place_psf(psf, N), PP.place(psf, N)
    assert got.shape == (3, N, N) and got.dtype == psf.dtype
    assert np.array_equal(got, want)
    cP, cN = (P - 1) // 2, (N - 1) // 2
    assert np.array_equal(got[:, cN, cN], psf[:, cP, cP])          # zero lag on zero lag
    assert np.count_nonzero(got[0]) == min(P, N) ** 2              # (the stamps have no zero tap)
    if P == N:
        assert np.array_equal(got, psf)
    lost = psf_flux_outside(psf, N)
    if P <= N:
        assert lost == 0.0
    else:
        assert abs(lost - PP.flux_outside(psf, N)) <= 1e-12 * lost and 0.0 < lost < 1.0


@pytest.mark.parametrize('n,P,ss', IDENTITY_CASES)
def test_placed_stamp_is_the_same_operator(n, P, ss):
    """deconv_model with the P x P stamps (the oracle's conv_same takes any kernel size) against deconv_model with the
    stamps placed on the N x N grid: for P <= N the same linear operator, to rounding of the float64 FFTs."""
    from oracle import model as om
    E, M = 2, 2
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=5 + P)
    rng = np.random.default_rng(P)
    stamps = np.stack([make_narrow_psf(rng, P, ss)[0] for _ in range(E)])
    p = {k: om.T(np.array(v, dtype=np.float64)) for k, v in ds['truth'].items()}
    direct = om.deconv_model(p, om.T(stamps), ss, n).numpy()
    placed = om.deconv_model(p, om.T(PP.place(stamps, n * ss)), ss, n).numpy()
    assert np.abs(direct - placed).max() <= 1e-12 * np.abs(direct).max()


def _roi_node(E, n, ss, psf_shape):
    rng = np.random.default_rng(1)
    return dict(frame_id=np.arange(E), data=rng.normal(size=(E, n, n)), noisemap=np.ones((E, n, n)), psf=np.ones(psf_shape),
                seeing=np.ones(E), mjd=np.arange(E) + 6e4, subsampling_factor=np.full(E, ss))


def test_read_roi_file_takes_psf_stamps_of_their_own_side():
    from lightcurver_amd.io import regions as R
    E, n, ss = 5, 32, 2
    out = R.read_roi_file(_roi_node(E, n, ss, (E, 48, 48)))        # stamp_size_stars = 24, stamp_size_ROI = 32
    assert out['psf_side'] == 48 and out['psf'].shape == (E, 48, 48) and out['data'].shape == (E, n, n)
    assert R.read_roi_file(_roi_node(E, n, ss, (E, 64, 64)))['psf_side'] == 64
    with pytest.raises(ValueError):
        R.read_roi_file(_roi_node(E, n, ss, (E, 48, 50)))          # not square
    with pytest.raises(ValueError):
        R.read_roi_file(_roi_node(E, n, ss, (E + 1, 48, 48)))      # another number of epochs
    with pytest.raises(ValueError):
        R.read_roi_file(dict(_roi_node(E, n, ss, (E, 48, 48)), noisemap=np.ones((E, n, n + 1))))


def test_host_index_rule_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler found (CXX, c++, g++, clang++): the host program cannot be built')
    exe = str(tmp_path / 'psf_place_main')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=undefined', '-I', HOST,
                            '-I', os.path.join(ROOT, 'lightcurver_amd', 'csrc'),
                            os.path.join(HOST, 'psf_place_main.cpp'), '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'all checks passed' in run.stdout
