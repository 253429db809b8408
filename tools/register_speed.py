"""Speed of registering source lists by star triangles on the device: astroalign.find_transforms_batch (one
lc_register_sources call: triangles, matches, consensus, refits and pairs of every problem) beside the float64 NumPy
restatement of the same SPEC (tests/_register.py) on this host's CPU.  The restatement is OUR NumPy, not astroalign, which
is absent here: its time is indicative only.

    python tools/register_speed.py [--problems 1000] [--points 50] [--reps 3] [--cpu-problems 10]

Every problem is a field of --points random stars against itself rotated, scaled, shifted and jittered by 0.3 px, with 20 %
of the target replaced by spurious points.  Wall time of the whole call (copies included) and kernel_ms (HIP events around
both kernels and the wait between them that sizes the table of matches), medians of --reps calls."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lightcurver_amd import _lib, astroalign  # noqa: E402
from tests import _register as R  # noqa: E402


def problems(K, N, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        out.append(R.field_case(N, float(rng.uniform(-180, 180)), float(rng.uniform(0.9, 1.1)), 0.3, 0.2,
                                seed=seed + 1 + k)[:2])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problems', type=int, default=1000)
    ap.add_argument('--points', type=int, default=50)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cpu-problems', type=int, default=10, help='problems the restatement is timed on (0: none)')
    a = ap.parse_args()
    ctx = _lib.Context(0)
    pr = problems(a.problems, a.points)
    S, T = [p[0] for p in pr], [p[1] for p in pr]
    astroalign.find_transforms_batch(S[:2], T[:2], max_control_points=a.points, ctx=ctx)          # warm-up
    wall, kms = [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        r = astroalign.find_transforms_batch(S, T, max_control_points=a.points, ctx=ctx)
        wall.append((time.perf_counter() - t) * 1e3)
        kms.append(r['kernel_ms'])
    row = dict(problems=a.problems, points=a.points, wall_ms=float(np.median(wall)), kernel_ms=float(np.median(kms)),
               solved=int((r['status'] == 0).sum()), matches_mean=float(r['diag'][:, 2].mean()),
               hypotheses_mean=float((r['diag'][:, 3] + 1)[r['status'] == 0].mean()) if (r['status'] == 0).any() else None)
    line = (f'{a.problems} problems of {a.points} x {a.points} points: find_transforms_batch {row["wall_ms"]:.1f} ms, kernels '
            f'{row["kernel_ms"]:.2f} ms ({row["kernel_ms"] / a.problems * 1e3:.1f} us per problem); {row["solved"]} solved, '
            f'{row["matches_mean"]:.0f} matches per problem')
    if a.cpu_problems:
        n = min(a.cpu_problems, a.problems)
        t = time.perf_counter()
        same = 0
        for k in range(n):
            w = R.register(S[k], T[k])
            same += int(w['status'] == r['status'][k] and w['diag'].tolist() == r['diag'][k].tolist())
        row['restatement_ms_per_problem'] = (time.perf_counter() - t) * 1e3 / n
        row['restatement_agrees'] = same
        line += (f' | the NumPy restatement {row["restatement_ms_per_problem"]:.1f} ms per problem on {n} of them '
                 f'({same} with the device\'s diag): indicative only, it is not astroalign')
    print(line, flush=True)
    print(json.dumps(dict(device=ctx.device_info()['name'], **row)))


if __name__ == '__main__':
    main()
