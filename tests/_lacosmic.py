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
