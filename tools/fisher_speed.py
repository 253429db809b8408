"""Ad-hoc timing of the flux errors: the diagonal Fisher call (fisher_flux_sigma, M epoch launches) against the full Fisher
information (fisher_flux_covariance: the same M launches writing the template slab, the Gram-and-solve kernel, three copies
back).  python tools/fisher_speed.py [reps] - at the C4 size (200 epochs of 64 x 64, M = 4) and one C5 shard (125 epochs of
128 x 128, M = 8), background non-zero (the FFT epoch kernels) and zero (the point-source kernel where the size has one).
Then the information with the positions free (fisher_positions: template kernel, Gram kernel on the matrix cores, the float64
arrowhead solve, one copy back) beside the flux-only covariance, at 200 x 64 x 64 and 125 x 128 x 128 with M = 4.
Last the information with the epochs' shifts free (fisher_shifts: the same plus the background pass of the dx, dy columns)
beside fisher_positions, at 200 x 64 x 64 with M = 2 and 125 x 128 x 128 with M = 4; the background pass on its own comes
from a kernel trace of this script (rocprofv3 --kernel-trace --stats: joint_fisher_shift_field_kernel + ..._cols_kernel).
python tools/fisher_speed.py [reps] shifts runs that part alone.
Last the batched star photometry (StarPhotometryBatch.fisher_shifts_per_star, mean free: all stars in one call) beside the
loop over one JointFit per star doing the same (fisher_shifts(mean=True) on objects that exist already - their creation
and upload not counted), 30 stars x 100 epochs at 24 x 24 and 32 x 32, M = 1, with and without per-star backgrounds.
python tools/fisher_speed.py [reps] batch runs that part alone."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from lightcurver_amd import _lib
from lightcurver_amd.joint import JointFit, StarPhotometryBatch
from lightcurver_amd.synthetic import make_roi_dataset

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
only = sys.argv[2] if len(sys.argv) > 2 else None
shifts_only = only in ('shifts', 'batch')
ctx = _lib.Context(0)
for name, E, n, M in () if shifts_only else (('C4', 200, 64, 4), ('C5-shard', 125, 128, 8)):
    ds = make_roi_dataset(E=E, M=M, n=n, ss=2, seed=11, with_background=True)
    p = {k: np.asarray(v, np.float64) for k, v in ds['truth'].items()}
    for bg in (True, False):
        q = dict(p) if bg else dict(p, h=np.zeros_like(p['h']))
        j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], 2, M, ctx)
        j.set_params(**q)
        j.set_free(['a'])
        j.fisher_flux_sigma()
        j.fisher_flux_covariance()   # (first call: the template slab is allocated)
        ctx.synchronize()
        res = {}
        for label, fn in (('diagonal', j.fisher_flux_sigma), ('covariance', j.fisher_flux_covariance)):
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                t.append(time.perf_counter() - t0)
            res[label] = float(np.median(t)) * 1e3
        j.close()
        print(f'{name} E={E} n={n} M={M} background={"on " if bg else "off"}: diagonal {res["diagonal"]:.3f} ms, '
              f'covariance {res["covariance"]:.3f} ms, ratio {res["covariance"] / res["diagonal"]:.2f}', flush=True)

for name, E, n, M in () if shifts_only else (('C4', 200, 64, 4), ('C5-shard', 125, 128, 4)):
    ds = make_roi_dataset(E=E, M=M, n=n, ss=2, seed=11, with_background=True)
    p = {k: np.asarray(v, np.float64) for k, v in ds['truth'].items()}
    j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], 2, M, ctx)
    j.set_params(**p)
    j.set_free(['a'])
    calls = (('flux covariance', j.fisher_flux_covariance), ('positions free', j.fisher_positions),
             ('positions + mean free', lambda: j.fisher_positions(mean=True)),
             ('fluxes only, new path', lambda: j.fisher_positions(positions=False)))
    for _, fn in calls:
        fn()                         # (first calls: the slabs are allocated)
    ctx.synchronize()
    res = {}
    for label, fn in calls:
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        res[label] = float(np.median(t)) * 1e3
    j.close()
    print(f'{name} E={E} n={n} M={M}: ' + ', '.join(f'{k} {v:.3f} ms' for k, v in res.items()), flush=True)

for name, E, n, M in () if only == 'batch' else (('C4', 200, 64, 2), ('C5-shard', 125, 128, 4)):
    ds = make_roi_dataset(E=E, M=M, n=n, ss=2, seed=11, with_background=True)
    p = {k: np.asarray(v, np.float64) for k, v in ds['truth'].items()}
    j = JointFit(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf'], 2, M, ctx)
    j.set_params(**p)
    j.set_free(['a'])
    j.set_loss(prior={'c_x_mean': p['c_x'], 'c_x_sigma': np.full(M, 0.05), 'c_y_mean': p['c_y'], 'c_y_sigma': np.full(M, 0.05)})
    calls = (('positions free', j.fisher_positions), ('fluxes only', lambda: j.fisher_positions(positions=False)),
             ('shifts free', j.fisher_shifts), ('shifts + positions + mean free', lambda: j.fisher_shifts(positions=True, mean=True)))
    for _, fn in calls:
        fn()
    ctx.synchronize()
    res = {}
    for label, fn in calls:
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        res[label] = float(np.median(t)) * 1e3
    j.close()
    N = 2 * n
    print(f'{name} E={E} n={n} M={M}: ' + ', '.join(f'{k} {v:.3f} ms' for k, v in res.items())
          + f'; background pass: {2 * E * n * n * N * N / 1e9:.2f} G multiply-adds', flush=True)

G, E, M = 30, 100, 1
for n in () if only == 'shifts' else (24, 32):
    sets = [make_roi_dataset(E=E, M=M, n=n, ss=2, seed=100 + g, with_background=True) for g in range(G)]
    for bg in (False, True):
        stacks = [(ds['data'], ds['noisemap'].astype(np.float64) ** 2, ds['psf']) for ds in sets]
        truth = [{k: np.asarray(v, np.float64) for k, v in ds['truth'].items()} for ds in sets]
        par = {k: np.concatenate([t[k] for t in truth]) for k in ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha', 'mean')}
        b = StarPhotometryBatch(stacks, 2, M, ctx, background=bg)
        b.set_params(h=np.concatenate([t['h'] for t in truth]) if bg else np.zeros(b.N * b.N), **par)
        fits = []
        for stack, t in zip(stacks, truth):   # (the batch without backgrounds holds h = 0: so do its stars' own objects)
            j = JointFit(*stack, 2, M, ctx)
            j.set_params(**(t if bg else dict(t, h=np.zeros_like(t['h']))))
            j.set_free(['a'])
            fits.append(j)
        calls = (('batch', lambda: b.fisher_shifts_per_star(mean=True)),
                 ('loop over the stars', lambda: [j.fisher_shifts(mean=True) for j in fits]))
        for _, fn in calls:
            fn()
        ctx.synchronize()
        res = {}
        for label, fn in calls:
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                t.append(time.perf_counter() - t0)
            res[label] = float(np.median(t)) * 1e3
        b.close()
        for j in fits:
            j.close()
        print(f'star batch G={G} E={E} n={n} M={M} backgrounds={"per star" if bg else "none    "}: '
              + ', '.join(f'{k} {v:.3f} ms' for k, v in res.items()), flush=True)
