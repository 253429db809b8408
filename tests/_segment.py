"""Checker for lc_segment_stamps: a NumPy restatement of the source-masking SPEC of DESIGN.md §5 ("Source masking")
and a generator of the scenes the tests run it on.

Not part of the product path.  ``segment`` follows the SPEC operation for operation: the per-pixel stage in float32
with every operation rounded on its own, every sum that decides something as exact integers of the 2^-20 fixed point,
the per-object scalar stage in float64 (Python floats: one rounding per operation).  The device kernel must give its
bits.  It also reports, per stamp, which paths it took (``paths``: split, depth, merged, zero), so that the tests can
assert their inputs exercise them."""
import math

import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), dtype=int)
KERNEL = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=np.float32)
FIX = 1048576.0          # 2^20: the fixed point of every deciding sum
SNR_LIMIT = 65536.0      # a detected pixel at or above 2^16 (or not finite): status 3
OBJ_CAP = 32             # leaves of the de-blending trees of one stamp (= objects before clean)
NODE_CAP = 64            # nodes of those trees, the groups included (the work list)
CLEAN_ZONE = 10.0
F32 = np.float32


class _Full(Exception):
    pass


def snr_image(data, noisemap):
    """Per-pixel stage on a (..., n, n) stack, float32: validity, w = 1 / (s s), the 3 x 3 filter with zero padding and
    the taps in raster order, snr = num / sqrt(den2) (0 where den2 <= 0)."""
    d = np.asarray(data, dtype=F32)
    s = np.asarray(noisemap, dtype=F32)
    with np.errstate(all='ignore'):
        ok = np.isfinite(d) & np.isfinite(s) & (s > 0)
        w = np.where(ok, F32(1) / (s * s), F32(0)).astype(F32)
        dw = np.where(ok, d * w, F32(0)).astype(F32)
        pad = [(0, 0)] * (d.ndim - 2) + [(1, 1), (1, 1)]
        wp, dwp = np.pad(w, pad), np.pad(dw, pad)
        n0, n1 = d.shape[-2:]
        num = np.zeros(d.shape, F32)
        den2 = np.zeros(d.shape, F32)
        for dy in range(3):
            for dx in range(3):
                k = KERNEL[dy, dx]
                num = num + k * dwp[..., dy:dy + n0, dx:dx + n1]
                den2 = den2 + (k * k) * wp[..., dy:dy + n0, dx:dx + n1]
        snr = np.where(den2 > 0, num / np.sqrt(den2), F32(0)).astype(F32)
    return snr


def quantise(v):
    """q = (int64) rint(v 2^20) of float32 values (v 2^20 is exact in float32 and in float64)."""
    return np.rint(np.asarray(v, dtype=F32).astype(np.float64) * FIX).astype(np.int64)


def fixed_sums(snr, m):
    """The integer sums of one pixel set: area, sum q, q x, q y, q x^2, q y^2, q x y (x = column)."""
    yy, xx = np.nonzero(m)
    q = quantise(snr[yy, xx])
    return (int(yy.size), int(q.sum()), int((q * xx).sum()), int((q * yy).sum()), int((q * xx * xx).sum()),
            int((q * yy * yy).sum()), int((q * xx * yy).sum()))


def levels(peak, thresh, nthresh):
    """lev_1 .. lev_{nthresh-1}: r = the nthresh-th root of peak / thresh by successive float32 sqrt, lev_k = lev_{k-1} r."""
    r = F32(peak) / F32(thresh)
    for _ in range({4: 2, 8: 3, 16: 4, 32: 5}[nthresh]):
        r = np.sqrt(r)
    out, lev = [], F32(thresh)
    for _ in range(1, nthresh):
        lev = F32(lev * r)
        out.append(lev)
    return out


def _deblend(snr, q, region, thresh, nthresh, cont, st, depth):
    area = int(region.sum())
    qt = int(quantise(thresh))
    total = int(q[region].sum()) - area * qt
    peak = snr[region].max()
    if not (peak > thresh) or total <= 0:
        return [region]
    for lev in levels(peak, thresh, nthresh):
        lab, k = ndimage.label(region & (snr > lev), structure=EIGHT)
        if k < 2:
            continue
        flux = np.zeros(k + 1, np.int64)
        np.add.at(flux, lab[lab > 0], q[lab > 0] - qt)
        good = [g for g in range(1, k + 1) if float(flux[g]) >= cont * float(total)]
        if len(good) < 2:
            continue
        st['nodes'] += len(good)
        if st['nodes'] > NODE_CAP:
            raise _Full
        st['depth'] = max(st['depth'], depth + 1)
        leaves, inside = [], np.zeros_like(region)
        for g in good:
            b = lab == g
            inside |= b
            f = float(flux[g])
            leaves.extend(_deblend(snr, q, b, lev, max(nthresh // 2, 4), cont * float(total) / f if f > 0 else 0.0,
                                   st, depth + 1))
        yy, xx = np.nonzero(region & ~inside)
        if yy.size:
            d2 = np.empty((yy.size, len(leaves)))
            for i, m in enumerate(leaves):
                py, px = np.unravel_index(np.argmax(np.where(m, snr, -np.inf)), snr.shape)
                size = max(math.sqrt(float(int(m.sum())) / math.pi), 1.0)
                d2[:, i] = ((yy - py) * (yy - py) + (xx - px) * (xx - px)).astype(np.float64) / (size * size)
            owner = np.argmin(d2, axis=1)
            leaves = [m.copy() for m in leaves]
            for i, m in enumerate(leaves):
                m[yy[owner == i], xx[owner == i]] = True
        return leaves
    return [region]


def _shape(snr, m, thresh, minarea):
    npix, s0, sx, sy, sxx, syy, sxy = fixed_sums(snr, m)
    t = float(s0)
    mx, my = float(sx) / t, float(sy) / t
    x2 = max(float(sxx) / t - mx * mx, 1.0 / 12.0)
    y2 = max(float(syy) / t - my * my, 1.0 / 12.0)
    xy = float(sxy) / t - mx * my
    det = x2 * y2 - xy * xy
    if det < 1.0 / 144.0:
        xy, det = 0.0, x2 * y2
    half, dif = 0.5 * (x2 + y2), x2 - y2
    root = math.sqrt(max(0.25 * (dif * dif) + xy * xy, 0.0))
    a, b = math.sqrt(half + root), math.sqrt(max(half - root, 1.0 / 12.0))
    mthresh = 0.0
    if npix >= minarea:
        kth = np.sort(snr[m])[npix - minarea]
        mthresh = max(float(kth) - float(thresh), 0.0)
    unitarea = math.pi * a * b
    tot = t * (1.0 / FIX)
    return dict(s0=s0, mx=mx, my=my, a=a, cxx=y2 / det, cyy=x2 / det, cxy=-2.0 * xy / det, npix=npix, unitarea=unitarea,
                amp=tot / (2.0 * unitarea), mthresh=mthresh)


def _clean(snr, masks, thresh, minarea):
    """-> target[i]: the object i is merged into, or -1.  Faintest first (ties: lower index first), shapes not updated."""
    target = [-1] * len(masks)
    if len(masks) < 2:
        return target
    sh = [_shape(snr, m, thresh, minarea) for m in masks]
    th = float(thresh)
    for i in sorted(range(len(masks)), key=lambda i: (sh[i]['s0'], i)):
        best, into = 0.0, -1
        for j in range(len(masks)):
            if j == i or target[j] >= 0 or sh[j]['s0'] <= sh[i]['s0']:
                continue
            dx, dy = sh[i]['mx'] - sh[j]['mx'], sh[i]['my'] - sh[j]['my']
            zone = CLEAN_ZONE * (sh[i]['a'] + sh[j]['a'])
            if dx * dx + dy * dy >= zone * zone:
                continue
            o = sh[j]
            ratio = o['amp'] / th
            if ratio <= 1.0:
                continue
            alpha = (ratio - 1.0) * o['unitarea'] / float(o['npix'])
            val = 1.0 + alpha * (o['cxx'] * dx * dx + o['cyy'] * dy * dy + o['cxy'] * dx * dy)
            wing = o['amp'] / val if 1.0 < val < 1e10 else 0.0
            if wing > sh[i]['mthresh'] and wing > best:
                best, into = wing, j
        target[i] = into
    return target


def segment_one(data, noisemap, thresh=3.0, minarea=15, deblend_nthresh=32, deblend_cont=0.001, clean=True,
                obj_cap=OBJ_CAP):
    """One stamp.  -> dict(mask bool (True = good), segmap int32, nobj, xy float64 (nobj, 2) barycentres (x, y), npix,
    status, paths)."""
    snr = snr_image(data, noisemap)
    n = snr.shape[0]
    thresh = F32(thresh)
    paths = dict(split=False, depth=0, merged=0, zero=False, central_fainter=False)
    out = dict(mask=np.ones((n, n), bool), segmap=np.zeros((n, n), np.int32), nobj=0, xy=np.zeros((0, 2)),
               npix=np.zeros(0, np.int32), status=0, paths=paths, snr=snr)
    det = snr > thresh
    if np.any(det & ~(snr < F32(SNR_LIMIT))):
        out['status'] = 3
        return out
    q = quantise(snr)
    lab, k = ndimage.label(det, structure=EIGHT)
    groups = [lab == g for g in range(1, k + 1)]
    groups = [g for g in groups if int(g.sum()) >= minarea]
    st = dict(nodes=len(groups), depth=0)
    leaves = []
    try:
        if st['nodes'] > NODE_CAP:
            raise _Full
        for g in groups:
            leaves.extend(_deblend(snr, q, g, thresh, deblend_nthresh, float(F32(deblend_cont)), st, 0))
        if len(leaves) > obj_cap:
            raise _Full
    except _Full:
        out['status'] = 1
        return out
    paths['split'], paths['depth'] = st['depth'] > 0, st['depth']
    target = _clean(snr, leaves, thresh, minarea) if clean else [-1] * len(leaves)
    paths['merged'] = sum(t >= 0 for t in target)
    final = []
    for i, m in enumerate(leaves):
        if target[i] >= 0:
            continue
        final.append((i, m.copy()))
    index = {i: r for r, (i, _) in enumerate(final)}
    for i, m in enumerate(leaves):
        j = i
        while target[j] >= 0:
            j = target[j]
        if j != i:
            final[index[j]][1][m] = True
    paths['zero'] = len(final) == 0
    if not final:
        return out
    xy, npix, s0s = [], [], []
    for r, (_, m) in enumerate(final):
        a, s0, sx, sy = fixed_sums(snr, m)[:4]
        s0s.append(s0)
        xy.append((float(sx) / float(s0), float(sy) / float(s0)))
        npix.append(a)
        out['segmap'][m] = r + 1
    c = (n - 1) / 2.0
    d2 = [(x - c) * (x - c) + (y - c) * (y - c) for x, y in xy]
    central = int(np.argmin(d2))
    paths['central_fainter'] = s0s[central] < max(s0s)
    out['mask'] = (out['segmap'] == 0) | (out['segmap'] == central + 1)
    out.update(nobj=len(final), xy=np.array(xy), npix=np.array(npix, np.int32), central=central)
    return out


def segment(datas, noisemaps, **kw):
    """A (K, n, n) stack.  -> dict(mask (K, n, n) bool, segmap int32, nobj int32 (K,), xy float32 (K, cap, 2) (zero past
    nobj), status int32 (K,), paths list of dicts)."""
    cap = kw.get('obj_cap', OBJ_CAP)
    res = [segment_one(d, s, **kw) for d, s in zip(datas, noisemaps)]
    K = len(res)
    xy = np.zeros((K, cap, 2), F32)
    for k, r in enumerate(res):
        xy[k, :r['nobj']] = r['xy'].astype(F32)
    return dict(mask=np.stack([r['mask'] for r in res]), segmap=np.stack([r['segmap'] for r in res]),
                nobj=np.array([r['nobj'] for r in res], np.int32), xy=xy,
                status=np.array([r['status'] for r in res], np.int32), paths=[r['paths'] for r in res])


# ---- scenes ---------------------------------------------------------------------------------------------------------

SCENES = ('single', 'blend', 'chain', 'wing_fragment', 'noise_only', 'nan_border', 'offcentre_bright', 'random')


def _star(n, x0, y0, amp, s):
    yy, xx = np.mgrid[0:n, 0:n]
    return amp * np.exp(-0.5 * ((xx - x0) ** 2 + (yy - y0) ** 2) / s ** 2)


def make_scene(kind, n, rng):
    """One stamp (data, noisemap), float32: a central star with 0 - 3 neighbours on unit-variance noise plus the photon
    noise of the stars.  Lengths scale with n / 32 so that every kind exists at every size."""
    u = n / 32.0
    c = (n - 1) / 2.0
    s = max(1.0, 1.8 * u)
    jx, jy = rng.uniform(-0.5, 0.5, 2)
    model = np.zeros((n, n))
    if kind == 'noise_only':
        pass
    elif kind == 'single':
        model = _star(n, c + jx, c + jy, rng.uniform(100, 2000), s)
    elif kind == 'blend':          # the neighbour's wings join the central star's group: the split path
        model = _star(n, c + jx, c + jy, 400.0, s) + _star(n, c + 7.0 * u + jx, c + 1.5 * u, rng.uniform(100, 250), s)
    elif kind == 'chain':          # three in a row, the saddles at different heights: a second level of recursion
        model = (_star(n, c - 6.5 * u, c + jy, 500.0, s) + _star(n, c, c + jy, 700.0, s)
                 + _star(n, c + 8.5 * u, c + 1.0 * u, 300.0, s))
    elif kind == 'wing_fragment':  # a bright star and a faint wide one far out on its wing: fragments for clean
        model = _star(n, c + jx, c + jy, 3000.0, 2.0 * u) + _star(n, c + 11.0 * u, c + jy, 3.0, 2.5 * u)
    elif kind == 'nan_border':
        model = _star(n, c + jx, c + jy, 600.0, s) + _star(n, c - 8.0 * u, c + 5.0 * u, 200.0, s)
    elif kind == 'offcentre_bright':  # the faint star sits at the centre, the brightest one does not
        model = _star(n, c + jx, c + jy, 60.0, s) + _star(n, c + 9.0 * u, c - 7.0 * u, 1500.0, s)
    else:
        model = _star(n, c + jx, c + jy, rng.uniform(100, 2000), s)
        for _ in range(int(rng.integers(0, 4))):
            model += _star(n, rng.uniform(1, n - 2), rng.uniform(1, n - 2), rng.uniform(20, 800), s * rng.uniform(0.8, 1.3))
    noise = np.sqrt(1.0 + model / 4.0)
    data = model + noise * rng.standard_normal((n, n))
    if kind == 'nan_border':
        w = max(1, n // 6)
        sl = [(slice(None), slice(0, w)), (slice(0, w), slice(None)), (slice(None), slice(n - w, n)),
              (slice(n - w, n), slice(None))][int(rng.integers(0, 4))]
        data[sl] = np.nan
        noise[sl] = np.nan
    return data.astype(F32), noise.astype(F32)


def make_scenes(K, n, seed):
    """K stamps cycling through SCENES.  -> (data, noisemap) float32 (K, n, n), kinds list."""
    rng = np.random.default_rng(seed)
    kinds = [SCENES[k % len(SCENES)] for k in range(K)]
    pairs = [make_scene(kind, n, rng) for kind in kinds]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), kinds


def crowded_stamp(n=64, blob=5, pitch=9, seed=0):
    """More separate small objects than the table holds: a grid of blob x blob plateaus (25 pixels each, above minarea)."""
    rng = np.random.default_rng(seed)
    model = np.zeros((n, n))
    for y in range(1, n - blob, pitch):
        for x in range(1, n - blob, pitch):
            model[y:y + blob, x:x + blob] = 40.0 + 3.0 * rng.uniform()
    data = model + 0.3 * rng.standard_normal((n, n))
    return data.astype(F32), np.ones((n, n), F32)


# ---- settings other than the defaults --------------------------------------------------------------------------------
SETTINGS_SIZES = ((24, 24), (33, 12))          # (n, K) of make_scenes(K, n, seed=100 n + K) and make_pairs(K, n, the same)
# (what differs from thresh 3, minarea 15, deblend_nthresh 32, deblend_cont 0.001, clean on; the settings it is
# compared with beyond those defaults; the input; the sizes it runs at).  A case exists to catch a kernel that ignores or
# mis-uses that setting, so the restatement's segmap with it must differ from the one at its base, and from the one
# at the defaults (tests/test_segment_cpu.py asserts both for every entry).  On the scenes deblend_cont 0.05 and 1e-6
# change nothing, so they run on make_pairs.  Cleaning merges every fragment of a share below 0.001 into the primary
# (whose wing at a distance d is about 3 npix / (pi d^2) above the threshold, more than such a fragment's pixels), so
# 1e-6 is told apart from 0.001 with cleaning off only.
SETTINGS = (
    (dict(thresh=1.5), {}, 'scenes', (24, 33)),
    (dict(thresh=6.0), {}, 'scenes', (24, 33)),
    (dict(minarea=1), {}, 'scenes', (24, 33)),
    (dict(minarea=5), {}, 'scenes', (24, 33)),
    (dict(minarea=40), {}, 'scenes', (24,)),
    (dict(deblend_cont=1.0), {}, 'scenes', (24, 33)),
    (dict(clean=False), {}, 'scenes', (24, 33)),
    (dict(thresh=1.5, minarea=3, deblend_cont=1e-5), {}, 'scenes', (24, 33)),
    (dict(deblend_nthresh=4), {}, 'scenes', (24, 33)),
    (dict(deblend_nthresh=8), {}, 'scenes', (24, 33)),
    (dict(deblend_nthresh=16), {}, 'scenes', (24, 33)),
    (dict(deblend_cont=0.05), {}, 'pairs', (24, 33)),
    (dict(deblend_cont=1e-6), dict(clean=False), 'pairs', (24, 33)),
)


def make_pairs(K, n, seed):
    """K blended pairs for deblend_cont, float32 (data, noisemap) (K, n, n), with the noise model of make_scene.  Even
    stamps: a secondary of about 1 % of the pair's flux, which 0.05 merges and 0.001 splits.  Odd stamps: a faint wide
    secondary on the rim of the primary's group, its share between 1e-6 and 1e-3, the noise drawn at a tenth of the
    noise map so that the share is the designed one."""
    rng = np.random.default_rng(seed)
    u = n / 32.0
    c = (n - 1) / 2.0
    s = max(1.0, 1.8 * u)
    share = ((1000.0, 20.0, 10.0), (1000.0, 80.0, 8.0), (3000.0, 40.0, 10.0), (3000.0, 300.0, 8.0))
    datas, noises = [], []
    for k in range(K):
        jx, jy = rng.uniform(-0.5, 0.5, 2)
        ang = rng.uniform(0.0, 2.0 * np.pi)
        amp1, amp2, sep, s2, level = (share[k // 2 % 4] + (s, 1.0)) if k % 2 == 0 else (1000.0, 2.0, 10.0, 1.2 * s, 0.1)
        model = _star(n, c + jx, c + jy, amp1, s)
        model += _star(n, c + jx + sep * u * np.cos(ang), c + jy + sep * u * np.sin(ang), amp2, s2)
        noise = np.sqrt(1.0 + model / 4.0)
        datas.append(model + level * noise * rng.standard_normal((n, n)))
        noises.append(noise)
    return np.stack(datas).astype(F32), np.stack(noises).astype(F32)


_settings_wanted = {}


def settings_wanted(n, K):
    """[(settings of the case, data, noisemap, the restatement with them, at their base, at the defaults)] of one
    SETTINGS_SIZES entry, computed once and shared by the CPU and the device tests."""
    if (n, K) not in _settings_wanted:
        d, s, _ = make_scenes(K, n, seed=100 * n + K)
        inputs = dict(scenes=(d, s), pairs=make_pairs(K, n, seed=100 * n + K))
        plain = {name: segment(*pair) for name, pair in inputs.items()}
        out = []
        for changed, base, name, sizes in SETTINGS:
            if n in sizes:
                d, s = inputs[name]
                out.append((dict(base, **changed), d, s, segment(d, s, **dict(base, **changed)),
                            segment(d, s, **base) if base else plain[name], plain[name]))
        _settings_wanted[n, K] = out
    return _settings_wanted[n, K]
