"""Wall-clock expectation of the batched star photometry with a background per star, apart from the correctness test that
measures it (tests/test_star_batch_background_gpu.py; tests/helpers.PERF).  Sorts after tests/test_zz_perf_gpu.py."""
import pytest

from tests import helpers as H

pytestmark = [pytest.mark.gpu, pytest.mark.perf]


def test_batched_background_photometry_beats_the_loop_over_stars():
    ratio = H.PERF.get('star_bg_batch_over_loop')
    if ratio is None:
        pytest.skip('tests/test_star_batch_background_gpu.py::test_thirty_stars_with_backgrounds_against_the_loop did not run in this session')
    print(f'batched star photometry with backgrounds: {ratio:.1f} x the loop')
    assert ratio >= 3.0
