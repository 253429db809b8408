"""Speed of the cosmic-ray detection on whole frames: the device call (lc_detect_cosmics_frames: time of all launches from
HIP events and wall time of the whole call, copies included) beside (a) the float32 NumPy restatement of the SPEC
(tests/_lacosmic.py) on the same host and the same inputs, results bit-equal, and (b) the traffic floor: the bytes the
launches must read and write, divided by the measured copy bandwidth (lc_copy_bandwidth).

    python tools/cosmics_frames_speed.py [--reps 5] [--frames 8] [--side 2048] [--cpu-frames 8]

K frames of side x side pixels: Poisson sky of 200 counts plus read noise and about 200 injected cosmics per frame (1 - 3
pixel tracks), timed without a variance (the SPEC's noise model) and with invar.  --cpu-frames: the restatement runs on
the first so many frames (a frame's result does not depend on the others) and its time is scaled to K; 0 skips it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib  # noqa: E402
from lightcurver_amd.astroscrappy import lacosmic_frames  # noqa: E402
from tests import _lacosmic as LA  # noqa: E402


def frames(K, side, seed, hits=200):
    rng = np.random.default_rng(seed)
    d = (rng.poisson(200.0, (K, side, side)) + rng.normal(0.0, 6.5, (K, side, side))).astype(np.float32)
    steps = [(0, 1), (1, 0), (1, 1), (1, -1)]
    for k in range(K):
        for _ in range(hits):
            y, x = (int(v) for v in rng.integers(3, side - 3, 2))
            sy, sx = steps[int(rng.integers(0, 4))]
            for t in range(int(rng.integers(1, 4))):
                d[k, y + t * sy, x + t * sx] += np.float32(rng.uniform(300.0, 5000.0))
    return d


def floor_bytes(shape, iters, with_invar):
    """What the launches must move at the least: prep reads the inputs and writes the planes (C, N with a variance, M,
    CR); every iteration of a frame reads C, M and N; a cleaning reads CR; finish reads C and CR and writes crmask and
    clean."""
    K, h, w = shape
    var = 4 if with_invar else 0
    per_pixel = K * (4 + var + 4 + var + 2) + int(iters.sum()) * (5 + var) + int((iters > 1).sum()) + K * (5 + 5)
    return per_pixel * h * w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--side', type=int, default=2048)
    ap.add_argument('--cpu-frames', type=int, default=8)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    gbs = C.c_float()
    ctx.check(_lib.lib().lc_copy_bandwidth(ctx.h, 1 << 30, 5, C.byref(gbs)), 'lc_copy_bandwidth')
    bw = float(gbs.value)
    d = frames(a.frames, a.side, seed=a.frames + a.side)
    lacosmic_frames(d[:1], ctx=ctx)                                        # warm-up (code object load)
    rows = []
    for with_invar in (False, True):
        iv = (np.maximum(d, 0) + np.float32(6.5) ** 2).astype(np.float32) if with_invar else None
        kms, wall = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            got = lacosmic_frames(d, invar=iv, ctx=ctx)
            wall.append((time.perf_counter() - t) * 1e3)
            kms.append(got['kernel_ms'])
        m = min(a.cpu_frames, a.frames)
        cpu, same = float('nan'), None                                      # --cpu-frames 0: the device call alone
        if m > 0:
            t = time.perf_counter()
            want = LA.lacosmic(d[:m], invar=None if iv is None else iv[:m])
            cpu = (time.perf_counter() - t) * 1e3 * a.frames / m
            same = bool(np.array_equal(got['crmask'][:m], want['crmask']) and np.array_equal(got['iters'][:m], want['iters'])
                        and np.array_equal(got['clean'][:m].view(np.uint32), want['clean'].view(np.uint32)))
        floor_ms = floor_bytes(d.shape, got['iters'], with_invar) / (bw * 1e9) * 1e3
        row = dict(K=a.frames, h=a.side, w=a.side, with_invar=with_invar, kernel_ms=float(np.median(kms)),
                   call_wall_ms=float(np.median(wall)), cpu_restatement_ms=cpu, cpu_frames_timed=m, bit_equal=same,
                   iters=got['iters'].tolist(), flagged=int(got['n_flagged'].sum()), traffic_floor_ms=floor_ms,
                   copy_bandwidth_gb_s=bw)
        print(f'{a.frames} x {a.side}^2 {"invar" if with_invar else "model"}: launches {row["kernel_ms"]:.2f} ms, call '
              f'{row["call_wall_ms"]:.0f} ms | CPU restatement {cpu:.0f} ms ({m} frames timed), bit-equal {same} | traffic '
              f'floor {floor_ms:.2f} ms at {bw:.0f} GB/s | iters {row["iters"]}, flagged {row["flagged"]}', flush=True)
        rows.append(row)
    print(json.dumps(dict(device=ctx.device_info()['name'], rows=rows)))


if __name__ == '__main__':
    main()
