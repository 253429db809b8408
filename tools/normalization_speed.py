"""Ad-hoc, host only: ``calculate_coefficients`` (star scalings by the direct KKT solve) against a scipy-SLSQP drive of the
same cost, as the reference runs it on its pivot tables, at S = 10 stars, E = 1000 frames.  One run each."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy.optimize import minimize

from lightcurver_amd.processes.normalization_calculation import calculate_coefficients

S, E = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (10, 1000)
rng = np.random.default_rng(0)
F = np.exp(rng.uniform(np.log(1e3), np.log(1e5), S))
t = rng.uniform(0.5, 1.5, E)
f = F[:, None] * t[None, :]
f = f + np.sqrt(f) * rng.standard_normal((S, E))
d = np.sqrt(f)
missing = rng.uniform(size=(S, E)) < 0.1
missing[:2] = False
f[missing] = d[missing] = np.nan


def cost(s, g, dg):
    """cost_function_scatter_in_frame on arrays (NaN = missing)."""
    w = 1.0 / dg
    v = s[:, None] * g
    mean = np.nansum(w * v, axis=0) / np.nansum(w, axis=0)
    return np.sum(np.nansum(w * (v - mean) ** 2, axis=0) / np.nansum(w, axis=0))


t0 = time.perf_counter()
out = calculate_coefficients(f, d)
t_kkt = time.perf_counter() - t0
median = np.nanmedian(f, axis=1, keepdims=True)
g, dg = f / median, d / median
t0 = time.perf_counter()
res = minimize(cost, np.ones(S), args=(g, dg), constraints=({'type': 'eq', 'fun': lambda c: 1 - np.nanmean(c)}), method='SLSQP')
t_slsqp = time.perf_counter() - t0
print(f'S={S} E={E}: calculate_coefficients (all of it) {t_kkt * 1e3:.2f} ms; SLSQP alone {t_slsqp * 1e3:.1f} ms '
      f'({res.nit} iterations, {res.nfev} cost evaluations)')
print(f'cost at the KKT solution {cost(out["star_scaling"], g, dg):.12e}, at SLSQP\'s {cost(res.x / res.x.mean(), g, dg):.12e}; '
      f'largest difference of the scalings {np.abs(out["star_scaling"] - res.x).max():.2e}')
