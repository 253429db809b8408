"""stack_data_diagnostic on the host (scipy shift + rotate per epoch and cube, NumPy stack) against on_device=True (one
lc_align_stack call over the three cubes): wall clock of both on the same machine at 200 x 64^2 (C4) and 125 x 128^2 (one
rank's share of C5), the device kernels' own time, and the array part alone (without the two forward models both paths
run).  Model and parameters are the truth of the synthetic dataset, rotations of +- 0.5 degrees with every other epoch
flipped by 180: no fit."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from lightcurver_amd import _lib
from lightcurver_amd.processes import roi_modelling as RM
from lightcurver_amd.starred.deconvolution.deconvolution import setup_model
from lightcurver_amd.synthetic import make_roi_dataset


def problem(E, M, n, ss, seed, ctx):
    rng = np.random.default_rng(seed)
    angles = rng.uniform(-0.5, 0.5, E)
    angles[0] = 0.0
    angles[1::2] += 180.0
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=seed, alpha=angles)
    t = ds['truth']
    data, noise = ds['data'].astype(np.float64), ds['noisemap'].astype(np.float64)
    model, k, _, _, _ = setup_model(data, noise ** 2, ds['psf'], t['c_x'], t['c_y'], ss, list(t['a']), ctx=ctx)
    for name in ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha'):
        k['kwargs_analytic'][name] = np.array(t[name], dtype=np.float64)
    for name in ('h', 'mean'):
        k['kwargs_background'][name] = np.array(t[name], dtype=np.float64)
    return data, noise, k, model


def best(fn, repeats):
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        walls.append(time.perf_counter() - t0)
    return min(walls), out


def main():
    ctx = _lib.default_context()
    for E, M, n, seed in ((200, 2, 64, 104), (125, 4, 128, 105)):
        data, noise, k, model = problem(E, M, n, 2, seed, ctx)
        RM.stack_data_diagnostic(data, noise, k, model, on_device=True, ctx=ctx)          # warm-up: the models both paths run
        t_dev, dev = best(lambda: RM.stack_data_diagnostic(data, noise, k, model, on_device=True, ctx=ctx), 5)
        t_host, host = best(lambda: RM.stack_data_diagnostic(data, noise, k, model), 2)
        cubes = np.stack([data, data * 0.5, data * 0.25]).astype(np.float32)
        shift_yx, angle = RM._alignment_of(k)
        t_arr, r = best(lambda: RM.align_stack_batch(cubes, noise, shift_yx, angle, ctx=ctx), 5)
        t_arr_host, _ = best(lambda: [RM.sigma_clipped_weighted_stack(RM.align_data_interpolation(c, k), noise)
                                      for c in cubes.astype(np.float64)], 1)
        worst = max(np.nanmax(np.abs(dev[key] - host[key])) / np.nanmax(np.abs(host[key])) for key in host)
        print(f'{E} x {n}^2: stack_data_diagnostic host {t_host * 1e3:.1f} ms, on_device {t_dev * 1e3:.1f} ms '
              f'({t_host / t_dev:.1f}x); array part alone: host {t_arr_host * 1e3:.1f} ms, lc_align_stack wall '
              f'{t_arr * 1e3:.2f} ms, kernels {r["kernel_ms"]:.3f} ms; largest difference of a stack {worst:.1e} of its peak',
              flush=True)


if __name__ == '__main__':
    main()
