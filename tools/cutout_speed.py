"""Speed of import + cut + mask of a set of frames, for the ROI size and the star size, on two paths:

  resident   FrameSet: the frames go up once, import_frames runs where they lie (sub is not downloaded), and
             cut_stamps cuts, forms the noise maps and masks every stamp of one size in one call;
  host cut   processes.frame_importation.import_frames with sub downloaded, NumPy slices per stamp, prepare_stamps for
             the noise maps, mask_cutout_batch for the masks (the stamps go up twice).

    python tools/cutout_speed.py [--frames 8] [--size 2048] [--stars 40] [--roi-size 64] [--star-size 32] [--reps 3]

Prints, per path, the wall time of the whole chain (copies and host steps included) and the sum of kernel_ms (HIP events
around the kernels) of its device calls, medians of --reps runs; for the resident path also the cut calls alone.  The
two paths give the same stamps, which is checked.  Nothing is asserted on the times."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib  # noqa: E402
from lightcurver_amd.frames import FrameSet  # noqa: E402
from lightcurver_amd.processes.cutout_making import cutout_origin, mask_cutout_batch  # noqa: E402
from lightcurver_amd.processes.frame_importation import import_frames  # noqa: E402
from lightcurver_amd.processes.preprocessing import prepare_stamps  # noqa: E402
from tests import _extract as E  # noqa: E402


def frames(K, h, w, seed):
    out = np.empty((K, h, w), np.float32)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    for k in range(K):
        out[k] = E.fast_scene(h, w, int(400 * h * w / 2048 ** 2), seed + k)[0] + (50.0 + 0.01 * x + 0.005 * y)
    return out


def resident(stack, t, jobs, ctx):
    """jobs: [(frame_index (S,), positions (S, 2), size)].  Returns (cuts, kernel_ms of the import, of the cuts, wall ms of the cuts)."""
    with FrameSet(stack, ctx) as fs:
        imp = fs.import_frames(t)
        t0 = time.perf_counter()
        cuts = [fs.cut_stamps(index, pos, n, do_mask_bad_columns=True, do_mask_cosmics=True) for index, pos, n in jobs]
        cut_wall = (time.perf_counter() - t0) * 1e3
        bare = sum(fs.cut_stamps(index, pos, n)['kernel_ms'] for index, pos, n in jobs)   # the cut kernel alone; not in the wall time
    return cuts, imp['kernel_ms'], sum(c['kernel_ms'] for c in cuts), cut_wall, bare


def host_cut(stack, t, jobs, ctx):
    imp = import_frames(stack, t, ctx=ctx)
    sub, (h, w) = imp['sub'], stack.shape[1:]
    kms, cuts = imp['kernel_ms'], []
    for index, pos, n in jobs:
        origin, _ = cutout_origin(pos, n, (h, w))
        data = np.full((len(pos), n, n), np.nan, np.float32)
        for s, (k, (x0, y0)) in enumerate(zip(index, origin)):
            xs, xe, ys, ye = max(0, x0), min(w, x0 + n), max(0, y0), min(h, y0 + n)
            data[s, ys - y0:ye - y0, xs - x0:xe - x0] = sub[k, ys:ye, xs:xe]
        prep = prepare_stamps(data, rms=imp['globalrms'][index], exptime=t[index], ctx=ctx, want=('noisemap',))
        noise = prep['noisemap']
        noise[np.isnan(data)] = np.nan          # prepare_stamps cleans the pixels outside the frame; the stamps keep them
        mask = mask_cutout_batch(data, noise, True, True, ctx=ctx)
        kms += prep['kernel_ms']
        cuts.append(dict(data=data, noisemap=noise, mask=mask))
    return cuts, kms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--stars', type=int, default=40, help='star stamps per frame')
    ap.add_argument('--roi-size', type=int, default=64)
    ap.add_argument('--star-size', type=int, default=32)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    K, h, w = a.frames, a.size, a.size
    stack = frames(K, h, w, seed=7)
    t = np.linspace(20.0, 60.0, K).astype(np.float32)
    rng = np.random.default_rng(1)
    roi = (np.arange(K), np.column_stack([w / 2 + rng.uniform(-2, 2, K), h / 2 + rng.uniform(-2, 2, K)]), a.roi_size)
    stars = (np.repeat(np.arange(K), a.stars),
             np.column_stack([rng.uniform(0, w, K * a.stars), rng.uniform(0, h, K * a.stars)]), a.star_size)
    jobs = [roi, stars]
    resident(stack[:1], t[:1], [(j[0][:1] * 0, j[1][:1], j[2]) for j in jobs], ctx)          # warm-up of both paths
    host_cut(stack[:1], t[:1], [(j[0][:1] * 0, j[1][:1], j[2]) for j in jobs], ctx)
    rows = dict(resident_wall_ms=[], resident_import_kernel_ms=[], resident_cut_kernel_ms=[], resident_cut_wall_ms=[],
                resident_cut_kernel_alone_ms=[], host_wall_ms=[], host_kernel_ms_without_masks=[])
    for _ in range(a.reps):
        t0 = time.perf_counter()
        cuts_r, imp_ms, cut_ms, cut_wall, bare = resident(stack, t, jobs, ctx)
        rows['resident_wall_ms'].append((time.perf_counter() - t0) * 1e3)
        rows['resident_cut_kernel_alone_ms'].append(bare)
        rows['resident_import_kernel_ms'].append(imp_ms)
        rows['resident_cut_kernel_ms'].append(cut_ms)
        rows['resident_cut_wall_ms'].append(cut_wall)
        t0 = time.perf_counter()
        cuts_h, kms = host_cut(stack, t, jobs, ctx)
        rows['host_wall_ms'].append((time.perf_counter() - t0) * 1e3)
        rows['host_kernel_ms_without_masks'].append(kms)
    for r, hc in zip(cuts_r, cuts_h):
        for key in ('data', 'noisemap', 'mask'):
            assert r[key].tobytes() == hc[key].tobytes(), key
    med = {k: float(np.median(v)) for k, v in rows.items()}
    print(f'{K} x {h} x {w}, per frame 1 ROI stamp of {a.roi_size} and {a.stars} star stamps of {a.star_size}, both masks on')
    print(f'  resident: wall {med["resident_wall_ms"]:.1f} ms (upload, import, two cut calls); kernels: import '
          f'{med["resident_import_kernel_ms"]:.2f} ms, cut + noise + masks {med["resident_cut_kernel_ms"]:.3f} ms, of it the cut '
          f'kernel {med["resident_cut_kernel_alone_ms"]:.4f} ms; the two cut calls alone {med["resident_cut_wall_ms"]:.2f} ms wall')
    print(f'  host cut: wall {med["host_wall_ms"]:.1f} ms (import with sub downloaded, slices, prepare_stamps, '
          f'mask_cutout_batch); kernels without the masks {med["host_kernel_ms_without_masks"]:.2f} ms')
    print(json.dumps(dict(device=ctx.device_info()['name'], K=K, h=h, w=w, stars=a.stars, roi_size=a.roi_size,
                          star_size=a.star_size, reps=a.reps, **med)))


if __name__ == '__main__':
    main()
