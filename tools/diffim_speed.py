"""Speed of difference imaging on the device (FrameSet.subtract_reference, lc_frames_subtract_reference; DESIGN.md §5
"Difference imaging"): n resident frames of h x w, each with its own small rotation and shift, resampled onto the
reference's grid, matched and subtracted, with bg_degree = 1, for r = 3 and r = 5 and regions (1, 1) and (4, 4).

    python tools/diffim_speed.py [--frames 200] [--shape 1024 960] [--reps 5] [--r 3 5] [--clip-iters 2]

kernel_ms (HIP events around every launch of the call; the host solves in between are not in it) as the median of --reps
calls after one warm-up call, with the spread; the split of a call between the Gram sums, the host solves and the
subtraction (split_ms); the float64 multiply-adds of the Gram sums (fit-set pixels x (P + 1)(P + 2) / 2 per round: the
lower triangle with the right-hand side) against the vendor's fp64 vector peak (78.6 TFLOP/s = 39.3 T multiply-adds
per second on the MI355X); and the HBM floor (per frame two planes for the resample and three per round: T read by both
kernels, D written) at the copy bandwidth measured in the same process (lc_copy_bandwidth)."""
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

FP64_VECTOR_FMA_PER_S = 78.6e12 / 2


def field(h, w, seed, n_stars=400):
    """A reference image: n_stars Gaussian stars on white noise of rms 1."""
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((h, w))
    yy, xx = np.mgrid[-8:9, -8:9]
    for _ in range(n_stars):
        cx, cy, s = rng.uniform(10, w - 11), rng.uniform(10, h - 11), rng.uniform(1.2, 2.2)
        ix, iy = int(cx), int(cy)
        img[iy - 8:iy + 9, ix - 8:ix + 9] += rng.uniform(50, 5000) * np.exp(-0.5 * ((xx + ix - cx) ** 2 + (yy + iy - cy) ** 2) / s ** 2)
    return img.astype(np.float32)


def geometry(n, h, w, seed):
    """(n, 2, 3): rotations within +-0.5 degrees about the centre and shifts within +-3 pixels."""
    rng = np.random.default_rng(seed)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    out = np.empty((n, 2, 3))
    for k in range(n):
        rad = np.deg2rad(rng.uniform(-0.5, 0.5))
        a, b = np.cos(rad), np.sin(rad)
        sx, sy = rng.uniform(-3.0, 3.0, 2)
        out[k] = [[a, -b, cx - (a * cx - b * cy) + sx], [b, a, cy - (b * cx + a * cy) + sy]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--shape', type=int, nargs=2, default=(1024, 960))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--r', type=int, nargs='+', default=[3, 5])
    ap.add_argument('--clip-iters', type=int, default=2)
    a = ap.parse_args()
    n, (h, w) = a.frames, a.shape
    ctx = _lib.Context(0)
    gbps = C.c_float()
    ctx.check(_lib.lib().lc_copy_bandwidth(ctx.h, 1 << 30, 5, C.byref(gbps)), 'lc_copy_bandwidth')
    rounds = a.clip_iters + 1
    floor_bytes = n * h * w * 4 * (2 + 3 * rounds)
    floor_ms = floor_bytes / (gbps.value * 1e9) * 1e3
    print(f'{n} frames of {h} x {w}, {rounds} rounds: copy bandwidth {gbps.value:.0f} GB/s, HBM floor {floor_bytes / 1e9:.2f} GB = '
          f'{floor_ms:.2f} ms', flush=True)
    ref = field(h, w, 3)
    rng = np.random.default_rng(4)
    data = np.empty((n, h, w), np.float32)
    for k in range(n):                     # the frames are the reference scaled, offset and with noise of rms 2
        data[k] = rng.uniform(0.6, 1.2) * ref + rng.uniform(-5, 5) + 2.0 * rng.standard_normal((h, w)).astype(np.float32)
    affines = geometry(n, h, w, 5)
    sigma = np.full(n, 2.5, np.float32)
    rows_out = []
    with FrameSet(data, ctx) as fs:
        fs.subtract_reference([0, 1], affines[:2], ref, sigma=sigma[:2], r=1, download=('status',))        # warm-up
        for r in a.r:
            for regions in ((1, 1), (4, 4)):
                kms, wall, splits = [], [], []
                for rep in range(a.reps + 1):
                    t = time.perf_counter()
                    out = fs.subtract_reference(np.arange(n), affines, ref, sigma=sigma, r=r, bg_degree=1, regions=regions,
                                                clip_iters=a.clip_iters, download=('scale', 'status', 'n_used'))
                    if rep:
                        wall.append((time.perf_counter() - t) * 1e3)
                        kms.append(out['kernel_ms'])
                        splits.append(out['split_ms'].copy())
                P = (2 * r + 1) ** 2 + 3
                gram_ms, solve_ms, sub_ms = np.median(np.array(splits), axis=0)
                fma = float(out['n_used'].sum()) * (P + 1) * (P + 2) / 2 * rounds       # (the last round's fit set, every round)
                row = dict(n=n, h=h, w=w, r=r, regions=list(regions), P=P, rounds=rounds, reps=a.reps,
                           kernel_ms=float(np.median(kms)), kernel_ms_min=float(np.min(kms)), kernel_ms_max=float(np.max(kms)),
                           wall_ms=float(np.median(wall)), gram_ms=float(gram_ms), solve_ms=float(solve_ms),
                           subtract_ms=float(sub_ms), gram_fma=fma,
                           fraction_of_fp64_peak=fma / (gram_ms * 1e-3) / FP64_VECTOR_FMA_PER_S, floor_ms=floor_ms,
                           fraction_of_floor=floor_ms / float(np.median(kms)), ok=float((out['status'] == 0).mean()),
                           scale_median=float(np.nanmedian(out['scale'])))
                print(f'r {r} regions {regions}: kernels {row["kernel_ms"]:.1f} ms (min {row["kernel_ms_min"]:.1f}, max '
                      f'{row["kernel_ms_max"]:.1f}; {a.reps} calls), call {row["wall_ms"]:.0f} ms; Gram {gram_ms:.1f} ms, host '
                      f'solves {solve_ms:.1f} ms, subtraction {sub_ms:.1f} ms; {fma:.3g} multiply-adds = '
                      f'{100 * row["fraction_of_fp64_peak"]:.1f} % of the fp64 vector peak; the HBM floor is '
                      f'{100 * row["fraction_of_floor"]:.1f} % of the kernels; status 0 in {100 * row["ok"]:.0f} %', flush=True)
                rows_out.append(row)
    print(json.dumps(dict(device=ctx.device_info()['name'], copy_gbps=gbps.value, rows=rows_out), default=float))


if __name__ == '__main__':
    main()
