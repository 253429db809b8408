"""mask_surrounding_stars_batch (lc_segment_stamps) against the per-stamp host loop it replaces and against the PSF
build the masks feed: wall clock and kernel time at 800 x 32^2 (the stamps of C2: 100 frames x 8 stars) and
4000 x 64^2 (C3), the host loop over the same stamps (a sample of them, scaled), and build_psf_batch on the C2 frames
as tools/build_psf_e2e.py times it.  The stamps are the C2 / C3 star stamps with one or two neighbours added."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from lightcurver_amd import _lib
if os.environ.get('LCMI_DBG_LIB'): _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), os.environ['LCMI_DBG_LIB'])
from lightcurver_amd.processes.psf_modelling import mask_surrounding_stars, mask_surrounding_stars_batch
from lightcurver_amd.processes.source_masking import segment_batch
from lightcurver_amd.starred.procedures.psf_routines import build_psf_batch
from lightcurver_amd.synthetic import CONFIGS, make_psf_dataset


def stamps(name):
    cfg = dict(CONFIGS[name])
    cfg.pop('kind')
    ds = make_psf_dataset(**cfg)
    n = cfg['n']
    d = ds['data'].reshape(-1, n, n).astype(np.float32)
    nm = ds['noisemap'].reshape(-1, n, n).astype(np.float32)
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:n, 0:n]
    for k in range(len(d)):
        for _ in range(int(rng.integers(1, 3))):
            x0, y0 = rng.uniform(2, n - 3, 2)
            amp = rng.uniform(20, 300) * np.median(nm[k])
            star = amp * np.exp(-0.5 * ((xx - x0) ** 2 + (yy - y0) ** 2) / (1.8 * n / 32) ** 2)
            d[k] += star.astype(np.float32)
    return cfg, ds, d, nm


def main():
    ctx = _lib.default_context()
    out = {}
    for name in ('C2', 'C3'):
        cfg, ds, d, nm = stamps(name)
        mask_surrounding_stars_batch(d[:8], nm[:8], ctx=ctx)
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            masks, n_host = mask_surrounding_stars_batch(d, nm, ctx=ctx)
            walls.append(time.perf_counter() - t0)
        r = segment_batch(d, nm, ctx=ctx)
        sample = range(0, len(d), max(1, len(d) // 100))
        t0 = time.perf_counter()
        agree = sum(np.array_equal(mask_surrounding_stars(d[k], nm[k]), masks[k]) for k in sample)
        host = (time.perf_counter() - t0) / len(sample) * len(d)
        out[name] = min(walls)
        print(f'{name}: {len(d)} x {cfg["n"]}^2: device wall {min(walls) * 1e3:.2f} ms (median {np.median(walls) * 1e3:.2f}), '
              f'kernel {r["kernel_ms"]:.3f} ms, host loop {host:.2f} s (from {len(sample)} stamps), through the host '
              f'{n_host}, objects {np.bincount(r["nobj"]).tolist()}, status {np.bincount(r["status"]).tolist()}, '
              f'host masks equal on {agree} of {len(sample)}')
        if name == 'C2':
            F = cfg['F']
            imgs, nois = [ds['data'][f] for f in range(F)], [ds['noisemap'][f] for f in range(F)]
            ms = [ds['masks'][f] for f in range(F)]
            best = 1e9
            for _ in range(2):
                t0 = time.perf_counter()
                build_psf_batch(imgs, nois, 2, masks=ms, n_iter_analytic=100, n_iter_adabelief=3000,
                                guess_method_star_position='center', guess_fwhm_pixels=ds['fwhm_guess'])
                best = min(best, time.perf_counter() - t0)
            print(f'C2: build_psf_batch of the same {F} frames: {best * 1e3:.1f} ms; masking / PSF build = '
                  f'{out["C2"] / best:.3f}')


if __name__ == '__main__':
    main()
