"""Shared pieces of the PSF-fit geometry tests (tests/test_psf_geometry_gpu.py, tests/test_psf_cpu_port_cpu.py):
stars at offsets up to the quarter-stamp limit, stamps drawn from the oracle's own forward model, and the finer error
norms (per star, border ring) that the global max-norm of helpers.rel_err hides."""
import numpy as np

from oracle import model as om

TIE_EPS = 4e-4   # data pixels: delta = ss * x0 + c_off then lies within 1e-3 of the rounding tie for ss <= 2
RING = 8         # width of the border ring of grad_grid, high-resolution pixels


def tie_offset(n, ss):
    """The x0 (data pixels) of the last rounding tie of delta = ss * x0 + 0.5 inside the limit n / 4: ss * x0 = N / 4 - 1.
    (N is even at every instantiated size, so c_off = 0.5 and delta ties wherever ss * x0 is an integer.)"""
    return (n * ss // 4 - 1) / ss


def offset_frames(n, ss):
    """(3, 8, 2) star offsets (x0, y0) in data pixels, one set per frame:
    frame 0 - the four corners of the allowed square, two edge mid-points, the centre, one star just inside a tie of delta;
    frame 1 - the same figure at half the limit, the tie star's partner just past the tie, one more tie pair member;
    frame 2 - negative offsets only, with a tie pair across the negative tie on both axes."""
    lim, t, e = n / 4.0, tie_offset(n, ss), TIE_EPS
    f0 = [(lim, lim), (lim, -lim), (-lim, lim), (-lim, -lim), (lim, 0.13), (0.2, -lim), (0.0, 0.0), (t - e, -t - e)]
    h = 0.5 * lim
    f1 = [(h, h), (h, -h), (-h, h), (-h, -h), (h, 0.13), (0.2, -h), (t + e, -t + e), (-t + e, t + e)]
    f2 = [(-lim, -lim), (-lim, -0.37), (-0.21, -lim), (-t - e, -t + e), (-t + e, -t - e), (-h, -0.77 * lim),
          (-0.05, -0.02), (-0.9 * lim, -0.3 * lim)]
    return np.array([f0, f1, f2], dtype=np.float64)


def offsets_for(n, ss, S, F=3):
    """(F, S, 2): offset_frames, for S = 16 each frame followed by the next frame's set."""
    base = offset_frames(n, ss)
    assert S in (8, 16) and F <= 3
    if S == 8:
        return base[:F].copy()
    return np.stack([np.concatenate([base[f], base[(f + 1) % 3]]) for f in range(F)])


def draw_dataset(n, ss, xy_true, seed, rms=5.0, masked_fraction=0.01, flux_decades=2.0, brightest=None):
    """Stamps of stars at xy_true (F, S, 2) drawn from oracle.model.psf_model (Moffat only) plus noise
    sqrt(rms^2 + |clean|); 1 % of the pixels masked; fluxes spanning `flux_decades` decades inside every frame, in random
    order - except that star brightest[f] of frame f, where given, gets the largest flux of its frame.
    Same layout and scaling as lightcurver_amd.synthetic.make_psf_dataset, so the helpers of tests/helpers.py apply."""
    rng = np.random.default_rng(seed)
    F, S, _ = xy_true.shape
    N = n * ss
    data = np.zeros((F, S, n, n))
    noise = np.zeros((F, S, n, n))
    flux = np.zeros((F, S))
    moffat = np.zeros((F, 4))
    for f in range(F):
        flux[f] = rng.permutation(10.0 ** np.linspace(5.0 - flux_decades, 5.0, S))
        if brightest is not None and f in brightest:
            k = int(np.argmax(flux[f]))
            flux[f, [brightest[f], k]] = flux[f, [k, brightest[f]]]
        moffat[f] = (rng.uniform(2.8, 3.4), rng.uniform(2.6, 3.0), rng.uniform(-1.0, 1.0), rng.uniform(2.5, 3.5))
        p = dict(fwhm_x=om.T(moffat[f, 0]), fwhm_y=om.T(moffat[f, 1]), phi=om.T(moffat[f, 2]), beta=om.T(moffat[f, 3]),
                 B=om.T(np.zeros(N * N)), a=om.T(flux[f]), x0=om.T(xy_true[f, :, 0]), y0=om.T(xy_true[f, :, 1]),
                 sky=om.T(np.zeros(S)))
        clean = om.psf_model(p, ss, n).numpy()
        noise[f] = np.sqrt(rms ** 2 + np.abs(clean))
        data[f] = clean + noise[f] * rng.standard_normal(clean.shape)
    masks = rng.uniform(size=(F, S, n, n)) >= masked_fraction
    scale = np.percentile(data, 99.9)
    return dict(data=(data / scale).astype(np.float32), noisemap=(noise / scale).astype(np.float32), masks=masks,
                scale=scale, ss=ss, truth=dict(flux=flux / scale, x0=xy_true[..., 0], y0=xy_true[..., 1], moffat=moffat))


def params_at(ds, xy, seed, grid_sigma=2e-4, moffat=None):
    """Oracle parameter dicts (one per frame) with the stars AT xy (F, S, 2) - rounded to fp32 first, so that the oracle
    and the device see the same positions on either side of a rounding tie -, a pixel grid of `grid_sigma` * noise and a
    Moffat a little off the one the stamps were drawn from (or `moffat`).  The fluxes are 20 % below the truth (+- 2 %):
    every pixel's term of dL/da and dL/dsky then has the same sign, so these sums are well conditioned and an fp32
    implementation can meet an element-by-element tolerance on them."""
    rng = np.random.default_rng(seed)
    F, S = xy.shape[:2]
    n = ds['data'].shape[-1]
    N = n * ds['ss']
    out = []
    for f in range(F):
        m = ds['truth']['moffat'][f] * (1.02, 0.99, 1.0, 0.95) + (0.0, 0.0, 0.05, 0.0) if moffat is None else moffat
        xyf = xy[f].astype(np.float32).astype(np.float64)
        a = (0.8 * ds['truth']['flux'][f] * (1.0 + 0.02 * rng.standard_normal(S))).astype(np.float32).astype(np.float64)
        p = dict(fwhm_x=m[0], fwhm_y=m[1], phi=m[2], beta=m[3], B=grid_sigma * rng.standard_normal(N * N), a=a,
                 x0=xyf[:, 0], y0=xyf[:, 1], sky=1e-4 * rng.standard_normal(S))
        out.append({k: om.T(v) for k, v in p.items()})
    return out


def displaced(xy, seed, lo=0.1, hi=0.2):
    """xy moved by lo .. hi data pixels along each axis, either way: where the stamps are drawn when the stars are evaluated
    at xy.  The residual is then dominated by -dx * df/dx, every pixel's term of dL/dx0 has the same sign, and the
    position gradients are well-conditioned sums (see params_at)."""
    rng = np.random.default_rng(seed)
    return xy + rng.choice([-1.0, 1.0], xy.shape) * rng.uniform(lo, hi, xy.shape)


def eval_seed(n, ss, S):
    """Seed of the single-evaluation problem, shared by the GPU test and the C-port test so that both see the same inputs."""
    return 300 + n + ss + S


def case(n, ss, S, F, seed):
    """The evaluation problem of the geometry tests: stars AT offsets_for(n, ss, S, F), stamps drawn with the stars 0.1 to
    0.2 pixels from there.  -> ds, plist, xy."""
    xy = offsets_for(n, ss, S, F)
    ds = draw_dataset(n, ss, displaced(xy, seed + 1), seed)
    return ds, params_at(ds, xy, seed + 2), xy


def ring_mask(N, width=RING):
    m = np.ones((N, N), dtype=bool)
    m[width:N - width, width:N - width] = False
    return m


def ring_err(got, ref, width=RING):
    """Largest error on the outer `width` pixels of an (N, N) map relative to the largest reference element THERE."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    m = ring_mask(ref.shape[-1], width)
    return float(np.abs(got - ref)[..., m].max() / max(np.abs(ref[..., m]).max(), 1e-300))


def per_star_model_err(got, ref):
    """(S,) largest model error of every star relative to that star's own peak."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref).max(axis=(-1, -2)) / np.abs(ref).max(axis=(-1, -2))


def per_element_err(got, ref, floor=1e-3):
    """Element-by-element error of a column relative to |ref|, floored at `floor` of the column's largest element."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / np.maximum(np.abs(ref), floor * np.abs(ref).max())
