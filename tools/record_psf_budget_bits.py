"""Records the bits of short PSF fits into tests/golden/psf_budget_parent_bits.npz, so that a change of how the PSF-fit kernel
schedules its work (csrc/psf_kernels.h: operands of the transposed row pass requested a star ahead;
csrc/starlet_device.h: addresses of the transposes kept live) can be held to "same operands, same order, same rounding"
(tests/test_psf_budget_bits_gpu.py compares uint32 views of the star parameters, the pixel grid and the loss history).

usage: python tools/record_psf_budget_bits.py [--lib liblcmi_other.so] [--out file.npz]
  --lib: a library next to lightcurver_amd/liblcmi.so to record from (the parent commit's build), default liblcmi.so.

The inputs are made from additions, products, divisions and square roots of seeded random numbers only (no exp / pow, whose
last bit depends on the host's maths library).

Cases, all at ss = 2:
  n = 32, S = 1, 3, 8, 12 (12: two groups of stars), stars at -8, 0 and +8 data pixels from the centre in x and in y (the
    quarter-stamp limit: the window of the transposed row pass is clamped at both ends), 40 iterations as one launch and as
    7 + 33, in the two-workgroup form and with LCMI_PSF_SINGLE_WG=1;
  n = 16 (4 pixels per lane) and n = 24 (the starlet through LDS): F = 2, S = 3, 20 iterations, two-workgroup form;
  n = 64 (pixel state in global memory): F = 2, S = 2, 6 iterations in both forms;
  one evaluate() at n = 32 with every output requested."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'psf_budget_parent_bits.npz')

FORMS = ['split', 'single']   # default (two workgroups per frame) and LCMI_PSF_SINGLE_WG=1
# offsets of star s in units of the quarter stamp (n / 4 data pixels), x and y: every pair of -1, 0, +1 comes up in 9 stars
OFFSETS = [(-1, 0), (0, 0), (1, 0), (1, -1), (0, 1), (-1, -1), (1, 1), (0, -1), (-1, 1)]


def cases():
    """{name: configuration}.  `same_as`: the case whose results this one repeats bit for bit - the split of a run into two
    launches and the form of the loop change no bits - so the file holds them once, under that name."""
    c = {}
    for S in (1, 3, 8, 12):
        for launches in ((40,), (7, 33)):
            for form in FORMS:
                c[f'fit32_S{S}_{"x".join(map(str, launches))}_{form}'] = dict(n=32, F=2, S=S, launches=launches, form=form,
                                                                          same_as=f'fit32_S{S}_40_split')
    c['fit16_S3_20_split'] = dict(n=16, F=2, S=3, launches=(20,), form='split')
    c['fit24_S3_20_split'] = dict(n=24, F=2, S=3, launches=(20,), form='split')
    for form in FORMS:
        c[f'fit64_S2_6_{form}'] = dict(n=64, F=2, S=2, launches=(6,), form=form, same_as='fit64_S2_6_split')
    c['eval32_S3'] = dict(n=32, F=2, S=3, launches=(), form='split')
    return c


def case_names():
    return list(cases())


def stored_as(name):
    """The name under which the results of a case are stored."""
    return cases()[name].get('same_as', name)


def fit_inputs(n, F, S, **_):
    """Stamps of rational (Moffat beta = 2) stars at the OFFSETS (times n / 4 data pixels), noise sqrt(rms^2 + clean)."""
    rng = np.random.default_rng(9000 + n + 10 * F + S)
    v = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    data = np.zeros((F, S, n, n))
    noise = np.zeros((F, S, n, n))
    stars = np.zeros((F, S, 4))
    for f in range(F):
        for s in range(S):
            ox, oy = OFFSETS[(s + 2 * f) % len(OFFSETS)]
            xs, ys = ox * n / 4.0, oy * n / 4.0
            flux = 2000.0 * (1 + s % 5) * (1.0 + 0.1 * f)
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


def run_case(ctx, name):
    """Results of one case as {key: array}."""
    from lightcurver_amd.psf_batch import PsfBatch
    cfg = cases()[name]
    data, weight, stars, moffat = fit_inputs(**cfg)
    old = os.environ.pop('LCMI_PSF_SINGLE_WG', None)
    if cfg['form'] == 'single':
        os.environ['LCMI_PSF_SINGLE_WG'] = '1'
    try:
        b = PsfBatch(data, weight, 2, ctx)
        b.set_moffat(moffat)
        b.set_stars(stars)
        b.set_grid(None)
        b.propagate_noise()
        b.set_regularization(None, 1.0, 1.0)
        if cfg['launches']:
            for k in cfg['launches']:
                b.run_adabelief(k, init_learning_rate=1e-4)
            out = dict(grid=b.get_grid(), stars=b.get_stars(), loss=b.loss_history())
            assert b.split_fallbacks == 0, name
        else:
            ev = b.evaluate(model=True)
            out = {k: ev[k] for k in ('loss', 'chi2', 'grad_stars', 'grad_grid', 'model')}
        b.close()
    finally:
        os.environ.pop('LCMI_PSF_SINGLE_WG', None)
        if old is not None:
            os.environ['LCMI_PSF_SINGLE_WG'] = old
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
        ref = stored_as(name)
        for k, v in run_case(ctx, name).items():
            v = np.ascontiguousarray(v, dtype=np.float32)
            if ref == name:
                rec[f'{name}/{k}'] = v
            else:   # the library recorded from must itself repeat the bits, or the case needs an entry of its own
                assert np.array_equal(v.view(np.uint32), rec[f'{ref}/{k}'].view(np.uint32)), (name, ref, k)
        print(name, 'stored as', ref, {k: v.shape for k, v in rec.items() if k.startswith(ref + '/')}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **rec)
    print('library', _lib.LIB_PATH, '->', out_path, os.path.getsize(out_path), 'bytes')


if __name__ == '__main__':
    main()
