"""Speed of the co-addition of whole frames on the device (FrameSet.coadd, lc_frames_coadd; DESIGN.md §5 "Co-addition of
frames"): n frames of h x w, each with its own small rotation, scale and shift, resampled onto the frame's grid and
combined, both orders, for 'median' and 'sigma_clip' (and 'mean' with --mean).

    python tools/coadd_speed.py [--frames 200] [--shape 1024 960] [--reps 5] [--rows 0 ...] [--mean]

kernel_ms (HIP events around all kernels of the call) and the wall time of the whole call (uploads of the per-frame lists,
the four outputs copied back), medians of --reps calls after one warm-up call; beside them the HBM floor: the bytes every
form has to move, (n h w + 4 H W) 4, at the copy bandwidth measured in the same process (lc_copy_bandwidth).  --rows: strip
heights to time (0: the library's choice from its scratch budget)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib  # noqa: E402
from lightcurver_amd.frames import FrameSet  # noqa: E402


def geometry(n, h, w, seed):
    """(n, 2, 3): rotations within +-1.5 degrees about the centre, scales within 0.5 %, shifts within +-6 pixels."""
    rng = np.random.default_rng(seed)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    out = np.empty((n, 2, 3))
    for k in range(n):
        rad, s = np.deg2rad(rng.uniform(-1.5, 1.5)), rng.uniform(0.995, 1.005)
        a, b = s * np.cos(rad), s * np.sin(rad)
        sx, sy = rng.uniform(-6.0, 6.0, 2)
        out[k] = [[a, -b, cx - (a * cx - b * cy) + sx], [b, a, cy - (b * cx + a * cy) + sy]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--shape', type=int, nargs=2, default=(1024, 960))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rows', type=int, nargs='+', default=[0])
    ap.add_argument('--mean', action='store_true')
    a = ap.parse_args()
    n, (h, w) = a.frames, a.shape
    ctx = _lib.Context(0)
    gbps = C.c_float()
    ctx.check(_lib.lib().lc_copy_bandwidth(ctx.h, 1 << 30, 5, C.byref(gbps)), 'lc_copy_bandwidth')
    floor_bytes = (n * h * w + 4 * h * w) * 4
    floor_ms = floor_bytes / (gbps.value * 1e9) * 1e3
    print(f'{n} frames of {h} x {w}: copy bandwidth {gbps.value:.0f} GB/s, HBM floor {floor_bytes / 1e6:.0f} MB = '
          f'{floor_ms:.3f} ms', flush=True)
    rng = np.random.default_rng(3)
    data = rng.normal(100.0, 5.0, (n, h, w)).astype(np.float32)
    affines = geometry(n, h, w, 4)
    weights = rng.uniform(0.5, 2.0, n).astype(np.float32)
    rows_out = []
    with FrameSet(data, ctx) as fs:
        fs.coadd(np.arange(2), affines[:2], order=3, combine='median')                  # warm-up
        for order in (1, 3):
            for combine in ('median', 'sigma_clip') + (('mean',) if a.mean else ()):
                for rows in a.rows:
                    kms, wall = [], []
                    for rep in range(a.reps + 1):
                        t = time.perf_counter()
                        out = fs.coadd(np.arange(n), affines, weights=weights, order=order, combine=combine, scratch_rows=rows)
                        if rep:
                            wall.append((time.perf_counter() - t) * 1e3)
                            kms.append(out['kernel_ms'])
                    row = dict(n=n, h=h, w=w, order=order, combine=combine, scratch_rows=rows, reps=a.reps,
                               kernel_ms=float(np.median(kms)), kernel_ms_min=float(np.min(kms)), kernel_ms_max=float(np.max(kms)),
                               wall_ms=float(np.median(wall)), floor_ms=floor_ms,
                               fraction_of_floor=floor_ms / float(np.median(kms)), covered=float(np.isfinite(out['image']).mean()),
                               rejected_per_pixel=float(out['n_rejected'].mean()))
                    print(f'order {order} {combine:10s} rows {rows:4d}: kernels {row["kernel_ms"]:.2f} ms (min {row["kernel_ms_min"]:.2f}, '
                          f'max {row["kernel_ms_max"]:.2f}; {a.reps} calls), call {row["wall_ms"]:.1f} ms; the floor is '
                          f'{100 * row["fraction_of_floor"]:.1f} % of the kernels; covered {100 * row["covered"]:.1f} %, rejected per '
                          f'pixel {row["rejected_per_pixel"]:.2f}', flush=True)
                    rows_out.append(row)
    print(json.dumps(dict(device=ctx.device_info()['name'], copy_gbps=gbps.value, rows=rows_out)))


if __name__ == '__main__':
    main()
