"""bench.py --dump-outputs (bench.dump_outputs): every array written whole as <name>.npy while the outputs fit the cap,
past it the same fixed sample of frames for every array, reproducible from run to run, the files within the cap."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs(F):
    rng = np.random.default_rng(1)
    return {'chi2': rng.standard_normal(F).astype(np.float32),
            'grid': rng.standard_normal((F, 16, 16)).astype(np.float32),
            'loss_history': rng.standard_normal((F, 31)).astype(np.float32)}


def test_outputs_under_the_cap_are_written_whole(tmp_path):
    out = _outputs(10)
    bench.dump_outputs(str(tmp_path), dict(out))
    assert sorted(os.listdir(tmp_path)) == sorted(k + '.npy' for k in out)
    for k, a in out.items():
        b = np.load(tmp_path / (k + '.npy'))
        assert b.dtype == a.dtype and np.array_equal(a, b)


def test_outputs_past_the_cap_are_one_fixed_sample_of_frames(tmp_path, monkeypatch):
    limit = 1 << 16
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', limit)
    F = 200
    out = _outputs(F)
    assert sum(a.nbytes for a in out.values()) > limit
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), dict(out))
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= limit
    frames = np.load(tmp_path / 'a' / 'frames.npy')
    assert frames.dtype == np.float64 and 0 < frames.size < F
    idx = frames.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < F
    for k, a in out.items():
        sa, sb = np.load(tmp_path / 'a' / (k + '.npy')), np.load(tmp_path / 'b' / (k + '.npy'))
        assert np.array_equal(sa, a[idx]) and np.array_equal(sa, sb)
