"""Ad-hoc timing of the batched star photometry: python tools/star_batch_speed.py G E n iters [--background]
(--background: every star with its own starlet background grid, lc_joint_create_groups_background, against one one-star fit
of the same problem with h free - the per-iteration figures of the batch and of one star of the loop)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lightcurver_amd import _lib
from lightcurver_amd.joint import JointFit, StarPhotometryBatch
from lightcurver_amd.synthetic import make_roi_dataset
bg = '--background' in sys.argv
G, E, n, iters = [int(x) for x in [a for a in sys.argv[1:] if not a.startswith('--')][:4]]
base = make_roi_dataset(E=E, M=1, n=n, ss=2, seed=77, with_background=bg)
ctx = _lib.Context(0)
sig2 = base['noisemap'].astype(np.float64) ** 2
stacks = [(base['data'], sig2, base['psf'])] * G
t0 = time.perf_counter(); b = StarPhotometryBatch(stacks, 2, 1, ctx, background=bg); ctx.synchronize(); print('create', time.perf_counter() - t0)
a = np.tile(np.asarray(base['truth']['a']) * 0.9, G)
b.set_params(a=a, c_x=np.zeros(G), c_y=np.zeros(G), dx=np.zeros(G * E), dy=np.zeros(G * E), alpha=np.zeros(G * E), mean=np.zeros(G * E))
if bg:
    t0 = time.perf_counter(); W = b.propagate_noise(); print('propagate_noise', time.perf_counter() - t0)
    b.set_loss(W=W, lam_scales=3.0, lam_hf=3.0); b.set_free(['a', 'c_x', 'c_y', 'dx', 'dy', 'h'])
else:
    b.set_loss(); b.set_free(['a', 'c_x', 'c_y', 'dx', 'dy'])
b.run_adabelief(5, init_learning_rate=1e-3); ctx.synchronize()
ctx.timer_start(); t0 = time.perf_counter()
b.run_adabelief(iters, init_learning_rate=1e-3)
ms = ctx.timer_stop(); wall = time.perf_counter() - t0
print(f'G={G} E={E} n={n} background={bg}: {ms / iters * 1e3:.1f} us/iter (device), wall {wall / iters * 1e6:.1f} us/iter')
t0 = time.perf_counter(); h = b.loss_history(); print('history', time.perf_counter() - t0, h[0, 0], h[0, -1])
t0 = time.perf_counter(); m = b.model(); print('model', time.perf_counter() - t0)
t0 = time.perf_counter(); s = b.fisher_flux_sigma(); print('fisher', time.perf_counter() - t0)
b.close()
if bg:   # one star of the loop: the one-star fit of the same problem with h free
    j = JointFit(base['data'], sig2, base['psf'], 2, 1, ctx)
    W1 = j.propagate_noise()
    j.set_params(a=np.asarray(base['truth']['a']) * 0.9, c_x=np.zeros(1), c_y=np.zeros(1), dx=np.zeros(E), dy=np.zeros(E),
                 alpha=np.zeros(E), mean=np.zeros(E), h=np.zeros(j.N * j.N))
    j.set_loss(W=W1, lam_scales=3.0, lam_hf=3.0); j.set_free(['a', 'c_x', 'c_y', 'dx', 'dy', 'h'])
    j.run_adabelief(5, init_learning_rate=1e-3); ctx.synchronize()
    ctx.timer_start(); t0 = time.perf_counter()
    j.run_adabelief(iters, init_learning_rate=1e-3)
    ms = ctx.timer_stop(); wall = time.perf_counter() - t0
    print(f'one star, E={E} n={n}, h free: {ms / iters * 1e3:.1f} us/iter (device), wall {wall / iters * 1e6:.1f} us/iter; '
          f'{G} of them one after the other: {G * ms / iters * 1e3:.0f} us/iter')
    j.close()
