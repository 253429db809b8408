"""Speed of the arithmetic of importing frames on the device: processes.frame_importation.characterize_frames (one
lc_import_frames call per stack: sky, variance map, catalogue; then the sources table and the seeing on the host) beside a
float64 host form of the same chain on this host's CPU (the restated sky of tests/_background.py, matched_filter_snr on
sqrt(var), scipy.ndimage labels and snr-weighted moments; one frame of the batch, since it takes seconds).

    python tools/extract_speed.py [--reps 3] [--no-cpu] [--mask-sources-first] [--deblend]

--deblend: about 10 % of the stars get a close companion, and characterize_frames(deblend=True) (lc_import_frames_deblended)
is timed beside the same call with deblend=False on the same frames; the host form then adds
processes.source_masking._deblend on the box of every parent of one frame.

Batches: K x (h, w) = 16 x 2048^2 and 1 x 4096^2, 400 stars per 2048^2 pixels.  Wall time of the whole call (copies and
host steps included) and kernel_ms (HIP events around all kernels of the call), medians of --reps calls."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib  # noqa: E402
if os.environ.get('LCMI_DBG_LIB'): _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), os.environ['LCMI_DBG_LIB'])
from lightcurver_amd.processes.frame_importation import characterize_frames, import_frames  # noqa: E402
from tests import _background as B  # noqa: E402
from tests import _extract as E  # noqa: E402


def frames(K, h, w, seed, companions=False):
    out = np.empty((K, h, w), np.float32)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    n = int(400 * h * w / 2048 ** 2)
    for k in range(K):
        if companions:
            from tests import _deblend as D
            sub = D.pairs_scene(h, w, n - n // 10, n // 10, seed + k)[0]
        else:
            sub = E.fast_scene(h, w, n, seed + k)[0]
        out[k] = sub + (50.0 + 0.01 * x + 0.005 * y)
    return out


def host_deblend(frame, exptime):
    """The float64 host form of the de-blending alone: source_masking._deblend on the box of every parent."""
    from scipy import ndimage
    from lightcurver_amd.processes.source_masking import _deblend
    box = min(frame.shape) // 10
    bg = B.background(frame, bw=box, bh=box)
    sub = bg['sub'].astype(np.float64)
    var = ((float(bg['globalrms']) * exptime) ** 2 + np.abs(sub * exptime)) / exptime ** 2
    H = E.host_form(sub, var, 3.0, 10)
    sizes = np.bincount(H['lab'].ravel(), minlength=H['ncomp'] + 1)
    t = time.perf_counter()
    leaves = 0
    for c, sl in enumerate(ndimage.find_objects(H['lab']), start=1):
        if sizes[c] >= 10 and max(sl[0].stop - sl[0].start, sl[1].stop - sl[1].start) <= 64:
            leaves += len(_deblend(H['snr'][sl], H['lab'][sl] == c, 3.0, 32, 0.005, 10))
    return (time.perf_counter() - t) * 1e3, leaves


def host_form(frame, exptime):
    box = min(frame.shape) // 10
    bg = B.background(frame, bw=box, bh=box)
    sub = bg['sub'].astype(np.float64)
    var = ((float(bg['globalrms']) * exptime) ** 2 + np.abs(sub * exptime)) / exptime ** 2
    H = E.host_form(sub, var, 3.0, 10)
    sizes = np.bincount(H['lab'].ravel(), minlength=H['ncomp'] + 1)
    from scipy import ndimage
    n = 0
    for c, sl in enumerate(ndimage.find_objects(H['lab']), start=1):
        if sizes[c] >= 10:
            yy, xx = np.nonzero(H['lab'][sl] == c)
            E.host_moments(H['snr'], yy + sl[0].start, xx + sl[1].start)
            n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-cpu', action='store_true', help='leave the host form out')
    ap.add_argument('--mask-sources-first', action='store_true')
    ap.add_argument('--deblend', action='store_true', help='frames with companions, deblend=True beside deblend=False')
    a = ap.parse_args()
    ctx = _lib.Context(0)
    rows = []
    for K, h, w in ((16, 2048, 2048), (1, 4096, 4096)):
        d = frames(K, h, w, seed=h + K, companions=a.deblend)
        characterize_frames(d[:1], 30.0, mask_sources_first=a.mask_sources_first, ctx=ctx)          # warm-up
        wall, kms, calls = [], [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            res = characterize_frames(d, 30.0, mask_sources_first=a.mask_sources_first, ctx=ctx)
            wall.append((time.perf_counter() - t) * 1e3)
            kms.append(res[0]['kernel_ms'])
            t = time.perf_counter()
            import_frames(d, 30.0, mask_sources_first=a.mask_sources_first, ctx=ctx)
            calls.append((time.perf_counter() - t) * 1e3)
        row = dict(K=K, h=h, w=w, mask_sources_first=a.mask_sources_first, wall_ms=float(np.median(wall)),
                   device_call_ms=float(np.median(calls)), kernel_ms=float(np.median(kms)),
                   sources=[len(r['sources_table']) for r in res], seeing=[r['seeing_pixels'] for r in res])
        line = (f'{K} x {h} x {w}: characterize_frames {row["wall_ms"]:.1f} ms, of it the device call {row["device_call_ms"]:.1f} ms, '
                f'kernels {row["kernel_ms"]:.2f} ms; {int(np.mean(row["sources"]))} sources per frame, seeing '
                f'{np.median(row["seeing"]):.2f} px')
        if a.deblend:
            characterize_frames(d[:1], 30.0, mask_sources_first=a.mask_sources_first, ctx=ctx, deblend=True)
            wall, kms = [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                res = characterize_frames(d, 30.0, mask_sources_first=a.mask_sources_first, ctx=ctx, deblend=True)
                wall.append((time.perf_counter() - t) * 1e3)
                kms.append(res[0]['kernel_ms'])
            row.update(deblend_wall_ms=float(np.median(wall)), deblend_kernel_ms=float(np.median(kms)),
                       deblend_sources=[len(r['sources_table']) for r in res])
            line += (f' | deblend=True {row["deblend_wall_ms"]:.1f} ms, kernels {row["deblend_kernel_ms"]:.2f} ms, '
                     f'{int(np.mean(row["deblend_sources"]))} sources per frame')
            if not a.no_cpu:
                row['host_deblend_one_frame_ms'], leaves = host_deblend(d[0], 30.0)
                line += f' | host de-blending of one frame {row["host_deblend_one_frame_ms"]:.0f} ms ({leaves} leaves)'
        if not a.no_cpu:
            t = time.perf_counter()
            n = host_form(d[0], 30.0)
            row['host_form_one_frame_ms'] = (time.perf_counter() - t) * 1e3
            line += (f' | host form of one frame {row["host_form_one_frame_ms"]:.0f} ms ({n} objects): '
                     f'{K * row["host_form_one_frame_ms"] / row["wall_ms"]:.0f} x for the batch')
        print(line, flush=True)
        rows.append(row)
    print(json.dumps(dict(device=ctx.device_info()['name'], rows=rows)))


if __name__ == '__main__':
    main()
