"""Speed of the sky background of whole frames: lc_background_frames (kernel time from HIP events and wall time of the whole
call, copies included) and lc_background_map, beside the NumPy restatement of the SPEC (tests/_background.py) on this
host's CPU and the copy bandwidth the box measures.

    python tools/background_speed.py [--reps 5] [--no-cpu]

Batches: K x (h, w) = 1 x 2048^2, 8 x 2048^2, 1 x 4096 x 2048, n_boxes = 10 (the reference's box = min(shape) // 10); sky
plane, noise and 300 stars per 2048^2 pixels.  Medians of --reps calls.  The kernels of a call share one pair of HIP
events, so they are told apart by what a call is asked for: meshes alone runs the statistics and the mesh
post-processing, sub as well adds the map kernel; lc_background_map runs the y-direction spline and the map kernel
without the read of the frame."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib, sep  # noqa: E402
if os.environ.get('LCMI_DBG_LIB'): _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), os.environ['LCMI_DBG_LIB'])
from tests import _background as B  # noqa: E402


def frames(K, h, w, seed):
    """K frames: the test scene's sky plane and noise; the stars of one frame are drawn as 32 x 32 stamps (a full-frame
    Gaussian per star takes minutes at this size)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((K, h, w), np.float32)
    yy, xx = np.mgrid[-16:16, -16:16]
    for k in range(K):
        img = 50.0 + 0.1 * x + 0.05 * y + rng.normal(0.0, 3.0, (h, w)).astype(np.float32)
        for _ in range(int(300 * h * w / 2048 ** 2)):
            cy, cx = int(rng.integers(16, h - 16)), int(rng.integers(16, w - 16))
            peak = np.exp(rng.uniform(np.log(200.0), np.log(5000.0)))
            img[cy - 16:cy + 16, cx - 16:cx + 16] += (peak * np.exp(-(xx ** 2 + yy ** 2) / 8.0)).astype(np.float32)
        out[k] = img
    return out


def timed(reps, call):
    """(median wall ms, median kernel ms, last result) of reps calls of call() -> (result, kernel_ms)."""
    wall, kms = [], []
    for _ in range(reps):
        t = time.perf_counter()
        out, k = call()
        wall.append((time.perf_counter() - t) * 1e3)
        kms.append(k)
    return float(np.median(wall)), float(np.median(kms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true', help='leave the CPU restatement out')
    a = ap.parse_args()
    ctx = _lib.Context(0)
    bw_gbs = C.c_float()
    ctx.check(_lib.lib().lc_copy_bandwidth(ctx.h, 1 << 28, 10, C.byref(bw_gbs)), 'lc_copy_bandwidth')
    print(f'device copy bandwidth (read + write): {bw_gbs.value:.0f} GB/s', flush=True)
    rows = []
    for K, h, w in ((1, 2048, 2048), (8, 2048, 2048), (1, 4096, 2048)):
        d = frames(K, h, w, seed=K + h)
        box = min(h, w) // 10
        ny, nx = sep.mesh_shape(h, w, box, box)
        frame_bytes = K * h * w * 4

        def run(sub, back):
            r = sep.background_frames(d, bw=box, bh=box, sub=sub, back=back, ctx=ctx)
            return r, r['kernel_ms']

        def map_alone(mesh):
            ms = C.c_float()
            out = np.empty(d.shape, np.float32)
            ctx.check(_lib.lib().lc_background_map(ctx.h, K, h, w, box, box, _lib.ptr(mesh), _lib.ptr(out), C.byref(ms)),
                      'lc_background_map')
            return out, ms.value
        run(True, True)                                                  # warm-up (code object load)
        meshes = timed(a.reps, lambda: run(False, False))
        with_sub = timed(a.reps, lambda: run(True, False))
        both = timed(a.reps, lambda: run(True, True))
        mesh = meshes[2]['mesh_back']
        map_alone(mesh)
        mapped = timed(a.reps, lambda: map_alone(mesh))
        stats_ms, map_ms = meshes[1], with_sub[1] - meshes[1]
        row = dict(K=K, h=h, w=w, box=box, ny=ny, nx=nx, stats_post_kernels_ms=stats_ms, map_kernel_sub_ms=map_ms,
                   map_kernel_sub_and_back_ms=both[1] - meshes[1], map_kernel_back_alone_ms=mapped[1],
                   stats_gbs=3 * frame_bytes / stats_ms / 1e6, map_sub_gbs=2 * frame_bytes / map_ms / 1e6,
                   map_back_alone_gbs=frame_bytes / mapped[1] / 1e6, call_meshes_ms=meshes[0], call_sub_ms=with_sub[0],
                   call_sub_back_ms=both[0], frame_megabytes=frame_bytes / 1e6, copy_bandwidth_gbs=bw_gbs.value)
        line = (f'{K} x {h} x {w}, box {box} ({ny} x {nx} meshes): statistics + post {stats_ms:.3f} ms (3 reads of the frames: '
                f'{row["stats_gbs"]:.0f} GB/s) | map with sub {map_ms:.3f} ms (read + write: {row["map_sub_gbs"]:.0f} GB/s), '
                f'back alone {mapped[1]:.3f} ms (write: {row["map_back_alone_gbs"]:.0f} GB/s) | call: meshes {meshes[0]:.2f} ms, '
                f'+ sub {with_sub[0]:.2f} ms, + sub + back {both[0]:.2f} ms')
        if not a.no_cpu:
            t = time.perf_counter()
            want = [B.background(d[k], bw=box, bh=box) for k in range(K)]
            row['cpu_restatement_ms'] = (time.perf_counter() - t) * 1e3
            got = with_sub[2]
            unit = max(float(x['globalrms']) for x in want)
            row['mesh_back_diff_in_globalrms'] = max(float(np.abs(got['mesh_back'][k] - want[k]['mesh_back']).max())
                                                     for k in range(K)) / unit
            row['sub_diff_in_globalrms'] = max(float(np.abs(got['sub'][k] - want[k]['sub']).max()) for k in range(K)) / unit
            line += (f' | CPU restatement {row["cpu_restatement_ms"]:.0f} ms ({row["cpu_restatement_ms"] / with_sub[0]:.0f} x the '
                     f'call with sub); largest mesh difference {row["mesh_back_diff_in_globalrms"]:.2g}, largest pixel '
                     f'difference of sub {row["sub_diff_in_globalrms"]:.2g} of globalrms')
        print(line, flush=True)
        rows.append(row)
    print(json.dumps(dict(device=ctx.device_info()['name'], rows=rows)))


if __name__ == '__main__':
    main()
