"""Fusing the DPP lane moves into their multiply-adds, products and sums (csrc/starlet_device.h: dpp_taps, dpp_gated,
line_sum, wave_sum4) changes no operand, no order and no rounding: every case below gives, bit for bit, what the library of
the commit before that change gave on an MI355X.  tools/record_psf_bits.py defines the cases and recorded
tests/golden/psf_dpp_parent_bits.npz from that library; the comparison is np.array_equal on the uint32 views.

Cases: the starlet alone (zero-weight stamp, evaluate()) where lanes sit at line ends and two or four lines share a DPP row -
(n, ss) = (16, 1): four lanes per line; (16, 2), (32, 2): eight lanes per line with 4 and 8 pixels per lane; (24, 2), (64, 2):
the LDS form, where only the sums change -, a short fit at n = 32 with stars at -7.5, 0 and +7.5 data pixels (window of
the transposed row pass clamped at both ends) in both forms of the iteration loop, the same at n = 64, one small joint fit
and one point-source fit (the wave sums are theirs too)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('record_psf_bits', os.path.join(HERE, '..', 'tools', 'record_psf_bits.py'))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'psf_dpp_parent_bits.npz'))


def test_fixture_holds_every_case(golden):
    have = {k.split('/')[0] for k in golden.files}
    assert have == set(rec.case_names())


@pytest.mark.parametrize('name', rec.case_names())
def test_bits_are_those_of_the_parent_commit(ctx, golden, name):
    out = rec.run_case(ctx, name, stored=golden)
    keys = [k for k in golden.files if k.startswith(name + '/') and not k.startswith(name + '/in_')]
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
