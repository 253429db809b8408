"""Records the bits of a few small PSF, joint and point-source runs into tests/golden/psf_dpp_parent_bits.npz, so that
a change of the lane-exchange code (csrc/starlet_device.h: DPP taps, line and wave sums) can be held to "same operands, same
order, same rounding" (tests/test_psf_dpp_bits_gpu.py compares uint32 views).

usage: python tools/record_psf_bits.py [--lib liblcmi_other.so] [--out file.npz]
  --lib: a library next to lightcurver_amd/liblcmi.so to record from (the parent commit's build), default liblcmi.so.

The inputs of the PSF cases are made from additions, products, divisions and square roots of seeded random numbers only
(no exp / pow, whose last bit depends on the host's maths library); the inputs of the joint cases come from
lightcurver_amd.synthetic and are stored in the file beside the results (keys in_*), and the test feeds those."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'psf_dpp_parent_bits.npz')

STARLET_SIZES = [(16, 1), (16, 2), (32, 2), (24, 2), (64, 2)]   # DPP form: 4 and 8 lanes per line; LDS form: 24, 64
STARLET_KINDS = ['smooth', 'noise']
FITS = {'fit32': dict(n=32, F=3, S=3, iters=25, x0=(-7.5, 0.0, 7.5)),   # P5 window clamped at both ends
        'fit64': dict(n=64, F=1, S=2, iters=5, x0=(-7.5, 7.5))}
FIT_FORMS = ['split', 'single']   # default (two workgroups per frame) and LCMI_PSF_SINGLE_WG=1


def n_scales(N):
    return int(np.log2(N))


def starlet_inputs(n, ss, kind):
    N = n * ss
    J = n_scales(N)
    rng = np.random.default_rng(1000 * N + 10 * ss + len(kind))
    u = np.arange(N, dtype=np.float64)
    if kind == 'smooth':   # a rational bump off the centre on a pedestal: energy in the coarse scales and at the borders
        r2 = ((u[None] - 0.3 * N) / (0.2 * N)) ** 2 + ((u[:, None] - 0.6 * N) / (0.15 * N)) ** 2
        img = 5.0 / (1.0 + r2) + 0.3 + 0.01 * rng.standard_normal((N, N))
    else:
        img = rng.standard_normal((N, N))
    W = rng.uniform(0.5, 2.0, (J, N, N))
    return img.astype(np.float32), W.astype(np.float32)


def run_starlet(ctx, n, ss, kind):
    from lightcurver_amd.psf_batch import PsfBatch
    img, W = starlet_inputs(n, ss, kind)
    b = PsfBatch(np.zeros((1, 1, n, n), np.float32), np.zeros((1, 1, n, n), np.float32), ss, ctx)
    b.set_moffat(np.array([[3.0, 3.0, 0.0, 2.5]]))
    b.set_stars(np.zeros((1, 1, 4)))
    b.set_grid(img[None])
    b.set_regularization(W[None], 1.5, 0.8)
    out = b.evaluate()
    b.close()
    return dict(loss=out['loss'], grad_grid=out['grad_grid'])


def fit_inputs(n, F, S, x0, **_):
    """Stamps of rational (Moffat beta = 2) stars at (x0[s], y0) data pixels from the centre, noise sqrt(rms^2 + clean)."""
    rng = np.random.default_rng(7000 + n + 10 * F + S)
    v = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    data = np.zeros((F, S, n, n))
    noise = np.zeros((F, S, n, n))
    stars = np.zeros((F, S, 4))
    for f in range(F):
        for s in range(S):
            xs, ys = x0[s] + 0.1 * (f - 1), (-x0[s] if s % 2 else 0.4 * x0[s]) + 0.05 * f
            flux = 2000.0 * (1 + s) * (1.0 + 0.1 * f)
            q = 1.0 + ((v[None] - xs) ** 2 + (v[:, None] - ys) ** 2) / 4.0
            clean = flux / (q * q) / (4.0 * 3.0)
            noise[f, s] = np.sqrt(25.0 + clean)
            data[f, s] = clean + noise[f, s] * rng.standard_normal((n, n))
            stars[f, s] = (0.8 * flux, xs, ys, 0.0)
    masks = rng.uniform(size=(F, S, n, n)) >= 0.01
    scale = 1000.0
    data, noise = data / scale, noise / scale
    stars[..., 0] /= scale
    weight = masks / noise ** 2
    moffat = np.tile(np.array([3.1, 2.9, 0.2, 2.5]), (F, 1))
    return data.astype(np.float32), weight.astype(np.float32), stars.astype(np.float32), moffat.astype(np.float32)


def run_fit(ctx, name, form):
    from lightcurver_amd.psf_batch import PsfBatch
    cfg = FITS[name]
    data, weight, stars, moffat = fit_inputs(**cfg)
    old = os.environ.pop('LCMI_PSF_SINGLE_WG', None)
    if form == 'single':
        os.environ['LCMI_PSF_SINGLE_WG'] = '1'
    try:
        b = PsfBatch(data, weight, 2, ctx)
        b.set_moffat(moffat)
        b.set_stars(stars)
        b.set_grid(None)
        b.propagate_noise()
        b.set_regularization(None, 1.0, 1.0)
        b.run_adabelief(cfg['iters'], init_learning_rate=1e-4)
        out = dict(grid=b.get_grid(), stars=b.get_stars(), loss=b.loss_history())
        b.close()
    finally:
        os.environ.pop('LCMI_PSF_SINGLE_WG', None)
        if old is not None:
            os.environ['LCMI_PSF_SINGLE_WG'] = old
    return out


JOINT_PARAMS = ('a', 'c_x', 'c_y', 'dx', 'dy', 'alpha', 'h', 'mean')


def joint_inputs(with_background):
    """3 epochs, n = 16, ss = 2, one source: data, sigma2, psf and the starting parameters, all float32."""
    from lightcurver_amd.synthetic import make_roi_dataset
    ds = make_roi_dataset(E=3, M=1, n=16, ss=2, seed=61 if with_background else 62, with_background=with_background)
    rng = np.random.default_rng(63)
    p = {k: np.array(v, dtype=np.float64) for k, v in ds['truth'].items()}
    p['a'] = 0.9 * p['a']
    p['c_x'] = p['c_x'] + 0.2
    p['c_y'] = p['c_y'] - 0.15
    p['h'] = p['h'] + 1e-3 * rng.standard_normal(p['h'].shape) if with_background else np.zeros_like(p['h'])
    out = dict(data=ds['data'], sigma2=ds['noisemap'].astype(np.float64) ** 2, psf=ds['psf'])
    out.update({k: p[k] for k in JOINT_PARAMS})
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def run_joint(ctx, inp):
    from lightcurver_amd.joint import JointFit
    j = JointFit(inp['data'], inp['sigma2'], inp['psf'], 2, 1, ctx)
    j.set_params(**{k: inp[k] for k in JOINT_PARAMS})
    j.set_loss(lam_scales=1.0, lam_hf=1.0, lam_positivity=10.0)
    j.set_free(['a', 'c_x', 'c_y', 'dx', 'dy', 'h', 'mean'])
    j.run_adabelief(10, init_learning_rate=1e-3)
    out = dict(loss=np.asarray(j.loss_history(), dtype=np.float32))
    j.close()
    return out


def run_ps(ctx, inp):
    from lightcurver_amd.joint import StarPhotometryBatch
    b = StarPhotometryBatch([(inp['data'], inp['sigma2'], inp['psf'])], 2, 1, ctx)
    b.set_params(**{k: inp[k] for k in JOINT_PARAMS})
    b.set_loss(lam_positivity_ps=2.0, lam_flux_uniformity=0.5)
    b.set_free(['a', 'c_x', 'c_y', 'dx', 'dy'])
    b.run_adabelief(10, init_learning_rate=1e-3)
    out = dict(loss=np.asarray(b.loss_history(), dtype=np.float32))
    b.close()
    return out


def case_names():
    names = [f'starlet_{n}_{ss}_{kind}' for n, ss in STARLET_SIZES for kind in STARLET_KINDS]
    names += [f'{name}_{form}' for name in FITS for form in FIT_FORMS]
    return names + ['joint', 'ps']


def run_case(ctx, name, stored=None):
    """Results of one case as {key: array}.  `stored`: the loaded golden file (inputs of the joint cases); None makes them."""
    if name.startswith('starlet_'):
        _, n, ss, kind = name.split('_')
        return run_starlet(ctx, int(n), int(ss), kind)
    if name.startswith('fit'):
        fit, form = name.split('_')
        return run_fit(ctx, fit, form)
    if stored is not None:
        inp = {k[len(name) + 4:]: stored[k] for k in stored.files if k.startswith(f'{name}/in_')}
    else:
        inp = joint_inputs(name == 'joint')
    out = (run_joint if name == 'joint' else run_ps)(ctx, inp)
    if stored is None:
        out.update({f'in_{k}': v for k, v in inp.items()})
    return out


def main():
    sys.path.insert(0, ROOT)
    from lightcurver_amd import _lib
    args = sys.argv[1:]
    out_path = GOLDEN
    while args:
        a = args.pop(0)
        if a == '--lib':
            _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), args.pop(0))
        elif a == '--out':
            out_path = args.pop(0)
        else:
            raise SystemExit(__doc__)
    ctx = _lib.Context(0)
    rec = {}
    for name in case_names():
        for k, v in run_case(ctx, name).items():
            rec[f'{name}/{k}'] = np.ascontiguousarray(v, dtype=np.float32)
        print(name, {k: v.shape for k, v in rec.items() if k.startswith(name + '/')}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **rec)
    print('library', _lib.LIB_PATH, '->', out_path, os.path.getsize(out_path), 'bytes')


if __name__ == '__main__':
    main()
