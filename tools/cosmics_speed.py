"""Speed of the cosmic-ray detection: the device call (lc_detect_cosmics: kernel time from HIP events and wall time of the
whole call, copies included) against the float32 NumPy restatement of the SPEC (tests/_lacosmic.py) on the same inputs,
vectorised over the batch and as a per-stamp loop (the reference's call pattern: one detect_cosmics per stamp).

    python tools/cosmics_speed.py [--reps 5] [--loop-stamps 400]

Batches: 800 x 32^2 (the stamps of C2) and 8000 x 24^2, star stamps with 0 - 3 injected cosmics each, invar = noisemap^2
as the reference passes it.  The per-stamp loop runs over the first --loop-stamps stamps and is scaled to the batch."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib  # noqa: E402
from lightcurver_amd.astroscrappy import lacosmic  # noqa: E402
from lightcurver_amd.synthetic import make_psf_dataset  # noqa: E402
from tests import _lacosmic as LA  # noqa: E402


def batch(K, n, seed):
    ds = make_psf_dataset(F=K // 8, S=8, n=n, seed=seed)
    d = ds['data'].reshape(-1, n, n)
    nm = ds['noisemap'].reshape(-1, n, n)
    d, _ = LA.inject_cosmics(d, nm, np.random.default_rng(seed + 1))
    return d, (nm ** 2).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--loop-stamps', type=int, default=400)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    rows = []
    for K, n in ((800, 32), (8000, 24)):
        d, iv = batch(K, n, seed=K + n)
        lacosmic(d, invar=iv, ctx=ctx)                                   # warm-up (code object load)
        kms, wall = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            got = lacosmic(d, invar=iv, ctx=ctx)
            wall.append((time.perf_counter() - t) * 1e3)
            kms.append(got['kernel_ms'])
        t = time.perf_counter()
        want = LA.lacosmic(d, invar=iv)
        cpu_vec = (time.perf_counter() - t) * 1e3
        m = min(a.loop_stamps, K)
        t = time.perf_counter()
        for k in range(m):
            LA.lacosmic(d[k], invar=iv[k])
        cpu_loop = (time.perf_counter() - t) * 1e3 * K / m
        same = bool(np.array_equal(got['crmask'], want['crmask']) and np.array_equal(got['iters'], want['iters'])
                    and np.array_equal(got['clean'].view(np.uint32), want['clean'].view(np.uint32)))
        row = dict(K=K, n=n, kernel_ms=float(np.median(kms)), call_wall_ms=float(np.median(wall)),
                   cpu_vectorised_ms=cpu_vec, cpu_per_stamp_loop_ms=cpu_loop, loop_stamps_timed=m,
                   flagged=int(want['crmask'].sum()), bit_equal=same,
                   speedup_call_vs_vectorised=cpu_vec / float(np.median(wall)),
                   speedup_call_vs_loop=cpu_loop / float(np.median(wall)))
        print(f'{K} x {n}^2: kernel {row["kernel_ms"]:.3f} ms, call {row["call_wall_ms"]:.2f} ms | CPU restatement '
              f'vectorised {cpu_vec:.0f} ms, per-stamp loop {cpu_loop:.0f} ms ({m} stamps timed) | '
              f'{row["speedup_call_vs_vectorised"]:.1f} x / {row["speedup_call_vs_loop"]:.1f} x, bit-equal {same}',
              flush=True)
        rows.append(row)
    print(json.dumps(dict(device=ctx.device_info()['name'], rows=rows)))


if __name__ == '__main__':
    main()
