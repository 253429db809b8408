"""Requesting the operands of the transposed row pass a star ahead and keeping the starlet's transpose addresses live
(csrc/psf_kernels.h, csrc/starlet_device.h) change no operand, no order and no rounding: every case below gives, bit for
bit, what the library of the commit before that change gave on an MI355X.  tools/record_psf_budget_bits.py defines the cases
and recorded tests/golden/psf_budget_parent_bits.npz from that library; the comparison is np.array_equal on the uint32
views of the star parameters, the pixel grid and the loss history.

Cases at (n, ss) = (32, 2): S = 1, 3, 8 and 12 stars (12: two groups of stars, so the look-ahead meets the end of a group) at
-8, 0 and +8 data pixels in x and y (the quarter-stamp limit: the window is clamped at both ends), 40 iterations as one
launch and as 7 + 33, in the two-workgroup form and with LCMI_PSF_SINGLE_WG=1.  (16, 2): 4 pixels per lane; (24, 2): the
starlet through LDS; (64, 2), both forms: the kernel with its pixel state in global memory; and one evaluate() at (32, 2)
with every output requested.  Cases that differ only in how the run is cut into launches or in the form of the loop gave the
same bits in that library, so the file holds them once (record_psf_budget_bits.stored_as) and each is compared with that."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('record_psf_budget_bits',
                                               os.path.join(HERE, '..', 'tools', 'record_psf_budget_bits.py'))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'psf_budget_parent_bits.npz'))


def test_fixture_holds_every_case(golden):
    have = {k.split('/')[0] for k in golden.files}
    assert have == {rec.stored_as(name) for name in rec.case_names()}


@pytest.mark.parametrize('name', rec.case_names())
def test_bits_are_those_of_the_parent_commit(ctx, golden, name):
    out = rec.run_case(ctx, name)
    keys = [k for k in golden.files if k.startswith(rec.stored_as(name) + '/')]
    assert sorted(k.split('/')[1] for k in keys) == sorted(out)
    for k in keys:
        want = golden[k]
        got = np.ascontiguousarray(out[k.split('/')[1]], dtype=np.float32)
        assert got.shape == want.shape, (k, got.shape, want.shape)
        differ = got.view(np.uint32) != want.view(np.uint32)
        print(k, want.shape, 'elements that differ:', int(differ.sum()),
              'largest difference:', float(np.abs(got.astype(np.float64) - want)[differ].max()) if differ.any() else 0.0)
        assert np.isfinite(want).all(), k
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
