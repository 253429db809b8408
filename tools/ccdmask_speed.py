"""Speed of the bad row / column mask and of the fused mask_cutout call: lc_ccdmask_stamps and lc_mask_cutouts (kernel
time from HIP events and wall time of the whole call, copies included) beside lc_detect_cosmics on the same stamps, the
sum of two separate calls (the lines alone through lc_mask_cutouts, which copies one mask back, plus the cosmics), and
the float32 NumPy restatement of the SPEC (tests/_ccdmask.py) on this host's CPU.

    python tools/ccdmask_speed.py [--reps 5]

Batches: 800 x 32^2 (the stamps of C2) and 8000 x 24^2, star stamps with one injected bad column each (and a bad row on
every second one) and 0 - 3 injected cosmics, noise maps as the reference passes them.  Medians of --reps calls."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib  # noqa: E402
if os.environ.get('LCMI_DBG_LIB'): _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), os.environ['LCMI_DBG_LIB'])
from lightcurver_amd.astroscrappy import _cfg as cosmics_cfg, lacosmic  # noqa: E402
from lightcurver_amd.ccdproc import _cfg as ccdmask_cfg, ccdmask_stamps  # noqa: E402
from lightcurver_amd.synthetic import make_psf_dataset  # noqa: E402
from tests import _ccdmask as CM  # noqa: E402
from tests import _lacosmic as LA  # noqa: E402


def batch(K, n, seed):
    ds = make_psf_dataset(F=K // 8, S=8, n=n, seed=seed)
    d = ds['data'].reshape(-1, n, n)
    nm = np.ascontiguousarray(ds['noisemap'].reshape(-1, n, n))
    d, _, _ = CM.inject_lines(d, nm, np.random.default_rng(seed + 1))
    d, _ = LA.inject_cosmics(d, nm, np.random.default_rng(seed + 2))
    return d, nm


def mask_cutouts(ctx, d, nm, bad_columns, cosmics):
    """lc_mask_cutouts as processes.cutout_making calls it, with the kernel time."""
    mask = np.zeros(d.shape, np.uint8)
    ms = C.c_float()
    ccfg, bcfg = cosmics_cfg(4.5, 0.3, 5.0, 1.0, 6.5, 65536.0, 4, True), ccdmask_cfg()
    ctx.check(_lib.lib().lc_mask_cutouts(ctx.h, d.shape[0], d.shape[1], _lib.ptr(d), _lib.ptr(nm), int(bad_columns),
                                         int(cosmics), C.byref(ccfg), C.byref(bcfg),
                                         mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(ms)), 'lc_mask_cutouts')
    return mask.astype(bool), ms.value


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
    a = ap.parse_args()
    ctx = _lib.Context(0)
    rows = []
    for K, n in ((800, 32), (8000, 24)):
        d, nm = batch(K, n, seed=K + n)
        iv = (nm ** 2).astype(np.float32)

        def lines():
            r = ccdmask_stamps(d, ctx=ctx)
            return r, r['kernel_ms']

        def cosmics():
            r = lacosmic(d, invar=iv, ctx=ctx)
            return r, r['kernel_ms']
        calls = dict(ccdmask=lines, cosmics=cosmics, fused=lambda: mask_cutouts(ctx, d, nm, True, True),
                     fused_lines_only=lambda: mask_cutouts(ctx, d, nm, True, False))
        res = {}
        for name, call in calls.items():
            call()                                                       # warm-up (code object load)
        for name, call in calls.items():
            res[name] = timed(a.reps, call)
        t = time.perf_counter()
        want = CM.ccdmask(d)
        cpu_ms = (time.perf_counter() - t) * 1e3
        got = res['ccdmask'][2]
        same = bool(all(np.array_equal(got[key], want[key]) for key in ('mask', 'rowcol', 'bad_cols', 'bad_rows'))
                    and np.array_equal(got['sigma'], want['sigma'], equal_nan=True))
        fused_same = bool(np.array_equal(res['fused'][2], got['rowcol'] | res['cosmics'][2]['crmask']))
        row = dict(K=K, n=n, ccdmask_kernel_ms=res['ccdmask'][1], ccdmask_call_ms=res['ccdmask'][0],
                   cosmics_kernel_ms=res['cosmics'][1], cosmics_call_ms=res['cosmics'][0],
                   fused_kernels_ms=res['fused'][1], fused_call_ms=res['fused'][0],
                   fused_lines_only_call_ms=res['fused_lines_only'][0],
                   two_calls_ms=res['fused_lines_only'][0] + res['cosmics'][0], cpu_restatement_ms=cpu_ms,
                   stamps_with_lines=int((want['bad_cols'].any(1) | want['bad_rows'].any(1)).sum()),
                   equal_to_restatement=same, fused_equals_or_of_calls=fused_same)
        print(f'{K} x {n}^2: ccdmask kernel {row["ccdmask_kernel_ms"]:.3f} ms, call {row["ccdmask_call_ms"]:.2f} ms | '
              f'cosmics kernel {row["cosmics_kernel_ms"]:.3f} ms, call {row["cosmics_call_ms"]:.2f} ms | fused kernels '
              f'{row["fused_kernels_ms"]:.3f} ms, call {row["fused_call_ms"]:.2f} ms against {row["two_calls_ms"]:.2f} ms '
              f'for the two calls | CPU restatement {cpu_ms:.0f} ms ({cpu_ms / row["ccdmask_call_ms"]:.0f} x the call) | '
              f'equal {same}, fused equal {fused_same}', flush=True)
        rows.append(row)
    print(json.dumps(dict(device=ctx.device_info()['name'], rows=rows)))


if __name__ == '__main__':
    main()
