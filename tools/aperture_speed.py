"""Speed of the exact circular-aperture sums on the device (DESIGN.md section 5 "Aperture sums") beside the float64 NumPy
restatement of the same SPEC (tests/_aperture.py) on this host's CPU.  The restatement is OUR NumPy, not photutils, which
is absent here: its time is indicative only.  It is given the aperture's bounding box cut from the image, as a host
implementation would do it, and is timed on --cpu-apertures apertures of each case.

    python tools/aperture_speed.py [--reps 5] [--cpu-apertures 200]

Two cases: 8 frames of 2048 x 2048 with 2000 apertures of r = 6 each, through photutils.aperture_sums_batch (the frames
are uploaded with the call) and through FrameSet.aperture_photometry (the frames are resident; with and without the
error), and one 64 x 64 stack with 4 apertures of r = 3 (the ROI's starting fluxes).  Wall time of the whole call (copies
included) and kernel_ms (HIP events around the kernel): median, and min .. max, of --reps calls."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib, photutils  # noqa: E402
from lightcurver_amd.frames import FrameSet  # noqa: E402
from tests import _aperture as A  # noqa: E402


def timed(call, reps):
    call()                                                          # warm-up
    wall, kms = [], []
    for _ in range(reps):
        t = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t) * 1e3)
        kms.append(r['kernel_ms'])
    spread = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    return dict(wall_ms=spread(wall), kernel_ms=spread(kms)), r


def host(images, index, xy, r, n):
    """ms per aperture of the restatement on the first n apertures, and its sums."""
    n = min(n, len(xy))
    h, w = images.shape[1:]
    t = time.perf_counter()
    sums = []
    for p in range(n):
        rows, cols = A.box(h, w, xy[p, 0], xy[p, 1], r)
        sums.append(A.aperture_sums(images[index[p]][rows, cols], xy[p, 0] - cols.start, xy[p, 1] - rows.start, r)[0])
    return (time.perf_counter() - t) * 1e3 / max(n, 1), np.array(sums)


def show(name, row):
    w, k = row['wall_ms'], row['kernel_ms']
    print(f'{name}: wall {w["median"]:.3f} ms ({w["min"]:.3f} .. {w["max"]:.3f}), kernel {k["median"]:.4f} ms '
          f'({k["min"]:.4f} .. {k["max"]:.4f})', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-apertures', type=int, default=200, help='apertures the restatement is timed on (0: none)')
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--apertures', type=int, default=2000, help='per frame')
    a = ap.parse_args()
    ctx = _lib.Context(0)
    rng = np.random.default_rng(1)
    out = dict(device=ctx.device_info()['name'], reps=a.reps)

    K, n, P = a.frames, a.size, a.apertures
    frames = rng.normal(100.0, 5.0, (K, n, n)).astype(np.float32)
    xy = rng.uniform(0.0, n - 1.0, (K * P, 2))
    index = np.repeat(np.arange(K), P).astype(np.int32)
    t, rms = np.full(K, 30.0, np.float32), np.full(K, 5.0, np.float32)
    case = dict(frames=K, size=n, apertures=K * P, r=6.0)
    case['batch'], r0 = timed(lambda: photutils.aperture_sums_batch(frames, index, xy, 6.0, ctx=ctx), a.reps)
    show(f'{K} frames of {n}^2, {K * P} apertures of r = 6, aperture_sums_batch (frames uploaded)', case['batch'])
    with FrameSet(frames, ctx) as fs:
        case['resident'], r1 = timed(lambda: fs.aperture_photometry(index, xy, 6.0), a.reps)
        show('  FrameSet.aperture_photometry (frames resident)', case['resident'])
        case['resident_with_error'], _ = timed(
            lambda: fs.aperture_photometry(index, xy, 6.0, with_error=True, exptimes=t, background_rms=rms), a.reps)
        show('  FrameSet.aperture_photometry with the error', case['resident_with_error'])
    assert r0['sum'].tobytes() == r1['sum'].tobytes()
    if a.cpu_apertures:
        ms, sums = host(frames, index, xy, 6.0, a.cpu_apertures)
        case['restatement_ms_per_aperture'] = ms
        case['restatement_max_rel_diff'] = float(np.max(np.abs(sums - r0['sum'][:len(sums)]) / np.abs(sums)))
        print(f'  the NumPy restatement {ms:.3f} ms per aperture on {len(sums)} of them ({ms * K * P:.0f} ms for all; largest '
              f'relative difference {case["restatement_max_rel_diff"]:.1e}): indicative only, it is not photutils', flush=True)
    out['frames'] = case

    stack = rng.normal(1.0, 0.1, (1, 64, 64)).astype(np.float32)
    xy = np.array([[30.2, 31.7], [35.9, 28.4], [20.5, 40.1], [44.3, 22.8]])
    case = dict(size=64, apertures=4, r=3.0)
    case['batch'], r0 = timed(lambda: photutils.aperture_sums_batch(stack, 0, xy, 3.0, ctx=ctx), a.reps)
    show('one 64^2 stack, 4 apertures of r = 3, aperture_sums_batch', case['batch'])
    if a.cpu_apertures:
        ms, sums = host(stack, np.zeros(4, int), xy, 3.0, 4)
        case['restatement_ms_per_aperture'] = ms
        print(f'  the NumPy restatement {ms * 4:.3f} ms for the four: indicative only, it is not photutils', flush=True)
    out['roi'] = case
    print(json.dumps(out))


if __name__ == '__main__':
    main()
