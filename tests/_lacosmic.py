"""Checker for lc_detect_cosmics: a NumPy restatement of the L.A.Cosmic SPEC of DESIGN.md §5 ("Cosmic-ray detection").

Not part of the product path.  ``lacosmic(..., dtype=np.float32)`` follows the SPEC's float32 operation order, so the
device kernel must reproduce it bit for bit; ``dtype=np.float64`` is the same algorithm in double precision, for the
float32-against-float64 check of the masks.  Vectorised over a (K, n, n) stack; stamps that stop early drop out of the
remaining iterations."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def _med_rows(X, k):
    h = k // 2
    n = X.shape[-1]
    Y = X.copy()
    if n > 2 * h:
        Y[..., h:n - h] = np.partition(sliding_window_view(X, k, axis=-1), h, axis=-1)[..., h]
    return Y


def _med_cols(X, k):
    return np.swapaxes(_med_rows(np.swapaxes(X, -1, -2), k), -1, -2)


def med_sep(X, k):
    """1 x k median along rows, then k x 1 along columns; (k-1)/2 border pixels keep each pass's input."""
    return _med_cols(_med_rows(X, k), k)


def med_full(X, k):
    """k x k median; pixels closer than (k-1)/2 to an edge keep the input."""
    h = k // 2
    n = X.shape[-1]
    Y = X.copy()
    if n > 2 * h:
        w = sliding_window_view(X, (k, k), axis=(-2, -1))
        w = w.reshape(w.shape[:-2] + (k * k,))
        Y[..., h:n - h, h:n - h] = np.partition(w, (k * k) // 2, axis=-1)[..., (k * k) // 2]
    return Y


def dil3(B):
    """3 x 3 square dilation, clipped at the edges."""
    P = np.pad(B, [(0, 0)] * (B.ndim - 2) + [(1, 1), (1, 1)])
    n0, n1 = B.shape[-2:]
    out = np.zeros_like(B)
    for dy in range(3):
        for dx in range(3):
            out |= P[..., dy:dy + n0, dx:dx + n1]
    return out


def laplacian(C):
    """Step 2a: 4c - (((up + down) + left) + right) on the 2x subsampled grid (outermost ring 0), clipped at 0,
    rebinned as ((a + b) + (c + d)) * 0.25."""
    dt = C.dtype.type
    sub = np.repeat(np.repeat(C, 2, axis=-2), 2, axis=-1)
    lap = np.zeros_like(sub)
    s = sub[..., :-2, 1:-1] + sub[..., 2:, 1:-1]
    s = s + sub[..., 1:-1, :-2]
    s = s + sub[..., 1:-1, 2:]
    lap[..., 1:-1, 1:-1] = dt(4) * sub[..., 1:-1, 1:-1] - s
    lap[lap < 0] = dt(0)
    a, b = lap[..., 0::2, 0::2], lap[..., 0::2, 1::2]
    c, d = lap[..., 1::2, 0::2], lap[..., 1::2, 1::2]
    return ((a + b) + (c + d)) * dt(0.25)


def lower_median(v):
    """Element of rank (m - 1) // 2 of the m values (0 when there are none)."""
    if v.size == 0:
        return v.dtype.type(0)
    return np.sort(v)[(v.size - 1) // 2]


def meanmask(C, CR, M):
    """Step 2h: every CR pixel gets the mean of the good pixels (neither CR nor M) of its 5 x 5 window, clipped to
    the stamp, summed in row-major window order; without any, the lower median of all good pixels of the stamp."""
    dt = C.dtype.type
    good = ~CR & ~M
    n0, n1 = C.shape[-2:]
    pad = [(0, 0)] * (C.ndim - 2) + [(2, 2), (2, 2)]
    Cp, Gp = np.pad(C, pad), np.pad(good, pad)
    acc = np.zeros_like(C)
    cnt = np.zeros(C.shape, np.int32)
    for dy in range(5):
        for dx in range(5):
            g = Gp[..., dy:dy + n0, dx:dx + n1]
            acc = acc + np.where(g, Cp[..., dy:dy + n0, dx:dx + n1], dt(0))
            cnt += g
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = acc / cnt.astype(C.dtype)
    out = np.where(CR, mean, C)
    need = CR & (cnt == 0)
    for k in np.nonzero(need.reshape(len(C), -1).any(axis=1))[0]:
        out[k][need[k]] = lower_median(C[k][good[k]])
    return out


def lacosmic(data, invar=None, inmask=None, sigclip=4.5, sigfrac=0.3, objlim=5.0, gain=1.0, readnoise=6.5,
             satlevel=65536.0, niter=4, sepmed=True, dtype=np.float32, trace=False):
    """data (K, n, n) or (n, n).  Returns dict(crmask bool, clean, iters int32[K], mask = the final M) and, with
    trace=True, 'trace': one entry per iteration, (stamp indices still running, SP, SP / F) of those stamps."""
    dt = np.dtype(dtype).type
    D = np.asarray(data)
    single = D.ndim == 2
    D = np.array(D.reshape((-1,) + D.shape[-2:]), dtype=np.float32).astype(dt)
    K, n = D.shape[0], D.shape[-1]
    m5, m3f, m7f = ((lambda X: med_sep(X, 7)), (lambda X: med_sep(X, 5)), (lambda X: med_sep(X, 9))) if sepmed else \
                   ((lambda X: med_full(X, 5)), (lambda X: med_full(X, 3)), (lambda X: med_full(X, 7)))
    g, rn = dt(gain), dt(readnoise)
    rn2 = rn * rn
    floor = dt(1e-5)
    # 0: counts, variance, mask (NaN rule: non-finite data / invar, invar <= 0 -> masked, C = 0, V = 1e-5 + rn^2)
    C = g * D
    M = np.zeros(D.shape, bool) if inmask is None else np.asarray(inmask, bool).reshape(D.shape).copy()
    with np.errstate(invalid='ignore', over='ignore'):
        hole = ~np.isfinite(D)
        if invar is not None:
            iv = np.array(np.asarray(invar).reshape(D.shape), dtype=np.float32).astype(dt)
            hole |= ~np.isfinite(iv) | (iv <= 0)
            V = iv * (g * g)
    C[hole] = dt(0)
    M |= hole
    if invar is not None:
        V[hole] = floor + rn2
        N = np.sqrt(V)
    # 1: saturation, grown twice
    satg = g * dt(satlevel)
    sat = (C >= satg) & (m5(C) > satg / dt(10))
    M |= dil3(dil3(sat))
    CR = np.zeros(D.shape, bool)
    iters = np.zeros(K, np.int32)
    active = np.arange(K)
    sc, sfl, ol = dt(sigclip), dt(sigfrac) * dt(sigclip), dt(objlim)
    tr = []
    for it in range(int(niter)):
        if active.size == 0:
            break
        Ca, Ma = C[active], M[active]
        L = laplacian(Ca)
        Na = N[active] if invar is not None else np.sqrt(np.maximum(m5(Ca), floor) + rn2)
        S = L / (dt(2) * Na)
        SP = S - m5(S)
        m3 = m3f(Ca)
        F = np.maximum((m3 - m7f(m3)) / Na, dt(0.01))
        ratio = SP / F
        cand = (SP > sc) & ~Ma & (ratio > ol)
        g1 = dil3(cand) & (SP > sc) & ~Ma
        g2 = dil3(g1) & (SP > sfl) & ~Ma
        if trace:
            tr.append((active.copy(), SP, ratio))
        CR[active] |= g2
        iters[active] = it + 1
        found = g2.reshape(len(active), -1).any(axis=1)
        active = active[found]
        if active.size:
            C[active] = meanmask(C[active], CR[active], M[active])
    out = dict(crmask=CR, clean=C / g, iters=iters, mask=M)
    if single:
        out = dict(crmask=CR[0], clean=out['clean'][0], iters=iters, mask=M[0])
    if trace:
        out['trace'] = tr
    return out


def star_stamps(K, n, seed, electrons):
    """K star stamps of make_psf_dataset (electrons: unscaled, for the noise model without invar) with 0 - 3 injected
    cosmics each, 1 % inmask, a partial-cutout NaN border on every fifth stamp; satlevel cuts into the brightest cores.
    Returns (data, noisemap, inmask, satlevel)."""
    from lightcurver_amd.synthetic import make_psf_dataset
    S = 8
    ds = make_psf_dataset(F=(K + S - 1) // S, S=S, n=n, seed=seed)
    scale = np.float32(ds['scale']) if electrons else np.float32(1.0)
    d = (ds['data'].reshape(-1, n, n)[:K] * scale).astype(np.float32)
    nm = (ds['noisemap'].reshape(-1, n, n)[:K] * scale).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    d, _ = inject_cosmics(d, nm, rng)
    inmask = rng.uniform(size=d.shape) < 0.01
    w = max(1, n // 5)
    for k in range(0, K, 5):
        side = k // 5 % 4
        sl = [(slice(None), slice(0, w)), (slice(0, w), slice(None)), (slice(None), slice(n - w, n)),
              (slice(n - w, n), slice(None))][side]
        d[k][sl] = np.nan
        nm[k][sl] = np.nan
    satlevel = float(np.nanpercentile(d, 99.8))
    return d, nm, inmask, satlevel


def inject_cosmics(data, noisemap, rng, max_per_stamp=3, amp=(5.0, 50.0)):
    """0 .. max_per_stamp cosmics per stamp of a (K, n, n) stack, each a 1 - 3 pixel track (horizontal, vertical or
    diagonal) at amp[0] .. amp[1] x the local noise.  Returns (perturbed copy, bool mask of the hit pixels)."""
    d = np.array(data, dtype=np.float32)
    hit = np.zeros(d.shape, bool)
    K, n = d.shape[0], d.shape[-1]
    steps = [(0, 1), (1, 0), (1, 1), (1, -1)]
    for k in range(K):
        for _ in range(int(rng.integers(0, max_per_stamp + 1))):
            length = int(rng.integers(1, 4))
            sy, sx = steps[int(rng.integers(0, 4))]
            y, x = int(rng.integers(3, n - 3)), int(rng.integers(3, n - 3))
            a = rng.uniform(*amp)
            for t in range(length):
                yy, xx = y + t * sy, x + t * sx
                d[k, yy, xx] += np.float32(a * noisemap[k, yy, xx])
                hit[k, yy, xx] = True
    return d, hit


# ---- settings other than the defaults --------------------------------------------------------------------------------
# label -> (settings changed, the settings they are changed from (beyond the defaults), the output that must differ).
# 'satlevel' is given as a factor of the percentile value star_stamps returns.  A case exists to catch a kernel that
# ignores or mis-uses that setting, so the restatement's ``differs`` output at (base + changed) must not equal the one at
# base on the case's input (for 'iters' also: some stamp runs past iteration 4); tests/test_cosmics_cpu.py asserts it
# for every entry of SETTINGS_CASES.
SETTINGS = {
    'sigclip 2': (dict(sigclip=2.0), {}, 'crmask'),
    'sigclip 8': (dict(sigclip=8.0), {}, 'crmask'),
    'sigclip 0.5 objlim 0.5': (dict(sigclip=0.5, objlim=0.5), {}, 'crmask'),      # the load case of meanmask
    'sigfrac 0': (dict(sigfrac=0.0), {}, 'crmask'),
    'sigfrac 1': (dict(sigfrac=1.0), {}, 'crmask'),
    'objlim 1': (dict(objlim=1.0), {}, 'crmask'),
    'objlim 50': (dict(objlim=50.0), {}, 'crmask'),
    'niter 0': (dict(niter=0), {}, 'crmask'),
    'niter 1': (dict(niter=1), {}, 'crmask'),
    'niter 12': (dict(niter=12), {}, 'iters'),
    'niter 12 sigclip 2': (dict(niter=12), dict(sigclip=2.0), 'iters'),
    'readnoise 0': (dict(readnoise=0.0), {}, 'crmask'),
    'readnoise 30': (dict(readnoise=30.0), {}, 'crmask'),
    'readnoise 0 sigclip 1': (dict(readnoise=0.0), dict(sigclip=1.0), 'crmask'),   # with invar: through vhole alone
    'readnoise 30 sigclip 1': (dict(readnoise=30.0), dict(sigclip=1.0), 'crmask'),
    'gain 0.37': (dict(gain=0.37), {}, 'clean'),
    'satlevel inf': (dict(satlevel=float('inf')), {}, 'clean'),
    'satlevel low': (dict(satlevel=0.05), {}, 'crmask'),
}


def settings_input(n, K, with_invar, variant='plain', seed=None):
    """(data, keyword arguments of lacosmic at the defaults) of one settings input.  'plain': star_stamps(K, n, 10 n + K)
    as tests/test_cosmics_gpu.py runs them (gain 1 with invar, 1.5 on electrons without).  'blocks': a square block of
    hot pixels on every third stamp on top, which the iterations peel ring by ring (niter).  'holes': 5 % of invar NaN
    at random, the invalid pixels whose variance readnoise sets (with invar only).  'electron holes': the same on the
    unscaled stamps, whose noise is of the size of readnoise, so that readnoise 30 differs from 6.5 there too."""
    seed = 10 * n + K if seed is None else seed
    d, nm, inmask, satlevel = star_stamps(K, n, seed=seed, electrons=not with_invar or variant == 'electron holes')
    rng = np.random.default_rng(seed + 2)
    invar = nm ** 2
    if variant == 'blocks':
        side = 5 if n < 32 else 7
        for k in range(1, K, 3):
            y, x = (int(v) for v in rng.integers(1, n - side - 1, 2))
            amp = rng.uniform(40.0, 60.0, (side, side)) * float(np.nanmedian(nm[k]))
            d[k, y:y + side, x:x + side] += amp.astype(np.float32)
    elif variant in ('holes', 'electron holes'):
        invar[rng.uniform(size=invar.shape) < 0.05] = np.nan
    elif variant != 'plain':
        raise ValueError(variant)
    return d, dict(invar=invar if with_invar else None, inmask=inmask, satlevel=satlevel, gain=1.0 if with_invar else 1.5)


def settings_kwargs(label, kw):
    """(keyword arguments of the case, of its base) for lacosmic, from the input's default keyword arguments kw."""
    changed, base, _ = SETTINGS[label]
    base = dict(kw, **base)
    case = dict(base, **changed)
    if 'satlevel' in changed:
        case['satlevel'] = changed['satlevel'] * kw['satlevel']
    return case, base


def settings_differ(label, want, base):
    """The condition of a case on the restatement's outputs ``want`` (the case) and ``base``."""
    key = SETTINGS[label][2]
    if key == 'clean':
        return not np.array_equal(want['clean'].view(np.uint32), base['clean'].view(np.uint32))
    if key == 'iters':
        return not np.array_equal(want['iters'], base['iters']) and int(want['iters'].max()) > 4
    return not np.array_equal(want[key], base[key])


# (n, K, with_invar, sepmed) -> the labels that do not run on the 'plain' input there: the variant on which the
# restatement meets the condition, as its name or (name, seed) where the input's own seed 10 n + K does not meet it
# either, or None where no variant at the seeds 1 - 8 does (the case is then not run on that input).  None occurs at
# n = 65 alone: niter 12 without sigclip 2 on three inputs, readnoise 30 at the default sigclip with invar and the full
# medians.  Sizes: the LDS path (16, 33) and the global planes (65).  With invar readnoise enters through the variance
# of the invalid pixels alone, so it is told apart only on an input with scattered invalid pixels, by many pixels at a
# low sigclip; 30 against the default 6.5 only where the noise is of that size ('electron holes'): on the scaled stamps
# both are far above every pixel's noise and no input found tells them apart.
SETTINGS_VARIANTS = {
    (16, 40, True, True): {'niter 1': 'blocks', 'readnoise 0': ('holes', 2), 'readnoise 30': ('electron holes', 2),
                           'readnoise 0 sigclip 1': 'holes', 'readnoise 30 sigclip 1': 'electron holes'},
    (16, 40, True, False): {'niter 1': 'blocks', 'niter 12': 'holes', 'readnoise 0': ('electron holes', 2),
                            'readnoise 30': ('electron holes', 7), 'readnoise 0 sigclip 1': 'holes',
                            'readnoise 30 sigclip 1': 'electron holes'},
    (16, 40, False, True): {},
    (16, 40, False, False): {'niter 1': 'blocks', 'niter 12': 'blocks'},
    (33, 24, True, True): {'objlim 1': 'blocks', 'niter 1': 'blocks', 'niter 12': 'holes', 'readnoise 0': 'holes',
                           'readnoise 30': 'electron holes', 'readnoise 30 sigclip 1': 'electron holes'},
    (33, 24, True, False): {'niter 1': 'blocks', 'niter 12': 'holes', 'niter 12 sigclip 2': 'blocks',
                            'readnoise 0': 'holes', 'readnoise 30': 'electron holes',
                            'readnoise 30 sigclip 1': 'electron holes', 'satlevel inf': 'blocks'},
    (33, 24, False, True): {'niter 1': 'blocks', 'niter 12': 'blocks'},
    (33, 24, False, False): {'niter 1': ('blocks', 5), 'niter 12': 'blocks', 'satlevel inf': 'blocks'},
    (65, 8, True, True): {'objlim 1': 'blocks', 'niter 1': 'blocks', 'niter 12': None, 'niter 12 sigclip 2': 'blocks',
                          'readnoise 0': ('holes', 2), 'readnoise 30': ('electron holes', 2),
                          'readnoise 30 sigclip 1': 'electron holes', 'satlevel inf': 'holes'},
    (65, 8, True, False): {'objlim 1': 'blocks', 'objlim 50': 'blocks', 'niter 1': 'blocks', 'niter 12': None,
                           'niter 12 sigclip 2': 'blocks', 'readnoise 0': ('holes', 2), 'readnoise 30': None,
                           'readnoise 30 sigclip 1': 'electron holes', 'satlevel inf': ('blocks', 3)},
    (65, 8, False, True): {'objlim 1': 'blocks', 'niter 1': 'blocks', 'niter 12': 'blocks',
                           'niter 12 sigclip 2': 'blocks', 'satlevel inf': ('blocks', 3)},
    (65, 8, False, False): {'objlim 1': 'blocks', 'niter 1': ('blocks', 7), 'niter 12': None,
                            'niter 12 sigclip 2': 'blocks', 'satlevel inf': ('blocks', 3)},
}
SETTINGS_INPUTS = tuple(SETTINGS_VARIANTS)
# the cases that run nowhere at their input: tests/test_cosmics_cpu.py holds the table to exactly these
SETTINGS_NOT_MET = {(65, 8, True, True): {'niter 12'}, (65, 8, True, False): {'niter 12', 'readnoise 30'},
                    (65, 8, False, False): {'niter 12'}}


def settings_cases(n, K, with_invar, sepmed):
    """[(label, variant, seed)] of one entry of SETTINGS_INPUTS; seed None: the input's own, 10 n + K."""
    out = []
    for label in SETTINGS:
        spec = SETTINGS_VARIANTS[n, K, with_invar, sepmed].get(label, 'plain')
        if spec is not None:
            out.append((label,) + (spec if isinstance(spec, tuple) else (spec, None)))
    return out


_settings_wanted = {}


def settings_wanted(n, K, with_invar, sepmed):
    """[(label, data, keyword arguments of the case, the restatement's result with them, its result at the base)] of
    one entry of SETTINGS_INPUTS, computed once and shared by the CPU and the device tests."""
    key = (n, K, with_invar, sepmed)
    if key not in _settings_wanted:
        inputs, bases, out = {}, {}, []
        for label, variant, seed in settings_cases(*key):
            if (variant, seed) not in inputs:
                inputs[variant, seed] = settings_input(n, K, with_invar, variant, seed)
            d, kw = inputs[variant, seed]
            case, base = settings_kwargs(label, kw)
            bkey = (variant, seed, repr(sorted((k, v) for k, v in base.items() if k not in ('invar', 'inmask'))))
            if bkey not in bases:
                bases[bkey] = lacosmic(d, sepmed=sepmed, **base)
            out.append((label, d, dict(case, sepmed=sepmed), lacosmic(d, sepmed=sepmed, **case), bases[bkey]))
        _settings_wanted[key] = out
    return _settings_wanted[key]
