"""Checker for lc_extract_frames_deblended: a NumPy restatement of the SPEC of DESIGN.md §5 ("De-blending and cleaning of
frame objects") and the scenes its tests run on.

Not part of the product path.  ``extract`` applies ``_extract.extract`` (the parents), ``_segment._deblend`` on each
parent's box (items 4 and 5 of the "Source masking" SPEC, word for word), the frame-level clean of item 5 and
``_extract.measure`` on the final pixel sets.  It reports the paths it took (``paths``: split, depth, merged, chain,
nodeblend_size, nodeblend_capacity) so that the tests can assert their inputs exercise them."""
import functools
import math

import numpy as np
from scipy import ndimage

from . import _extract as E
from . import _segment as S

F32 = np.float32
BOX = 64                 # the longest side of a parent's box that is de-blended
LEAF_CAP = S.OBJ_CAP     # leaves of one parent
NODE_CAP = S.NODE_CAP    # nodes of one parent's tree, the parent included
FLAG_NODEBLEND = 8
CLEAN_ZONE = S.CLEAN_ZONE


def deblend_parents(snr, segmap, nparents, thresh, nthresh, cont):
    """Item 2 and 3: -> list of dict(sl, region, leaves: bool masks of the box, nodeblend: '', 'size' or 'capacity',
    depth) per parent, in the parents' order."""
    thresh = F32(thresh)
    q = S.quantise(snr)
    out = []
    for num, sl in enumerate(ndimage.find_objects(segmap, max_label=nparents), start=1):
        region = segmap[sl] == num
        bh, bw = region.shape
        sub = snr[sl]
        rec = dict(sl=sl, region=region, leaves=[region], nodeblend='', depth=0)
        if bw > BOX or bh > BOX:
            rec['nodeblend'] = 'size'
        elif (sub[region] < F32(E.SNR_LIMIT)).all():       # a parent flagged RANGE stays whole, without the bit
            st = dict(nodes=1, depth=0)
            try:
                leaves = S._deblend(sub, q[sl], region, thresh, nthresh, cont, st, 0)
                if len(leaves) > LEAF_CAP:
                    raise S._Full
                rec['leaves'], rec['depth'] = leaves, st['depth']
            except S._Full:
                rec['nodeblend'] = 'capacity'
        out.append(rec)
    return out


def clean_shape(snr, yy, xx, thresh, minarea):
    """Item 5 (a): the shape of one object from the measurement's integer sums, or None for an object that takes no
    part (LARGE, RANGE, or a zero sum)."""
    s = snr[yy, xx]
    xmin, xmax, ymin, ymax = int(xx.min()), int(xx.max()), int(yy.min()), int(yy.max())
    if xmax - xmin + 1 > E.LARGE_BOX or ymax - ymin + 1 > E.LARGE_BOX or not (s < F32(E.SNR_LIMIT)).all():
        return None
    q = [int(t) for t in np.rint(s.astype(np.float64) * E.FIX)]
    dx = [int(t) - xmin for t in xx]
    dy = [int(t) - ymin for t in yy]
    s0 = sum(q)
    if s0 <= 0:
        return None
    t = float(s0)
    mx = float(sum(a * b for a, b in zip(q, dx))) / t
    my = float(sum(a * b for a, b in zip(q, dy))) / t
    x2 = max(float(sum(a * b * b for a, b in zip(q, dx))) / t - mx * mx, 1.0 / 12.0)
    y2 = max(float(sum(a * b * b for a, b in zip(q, dy))) / t - my * my, 1.0 / 12.0)
    xy = float(sum(a * b * c for a, b, c in zip(q, dx, dy))) / t - mx * my
    det = x2 * y2 - xy * xy
    if det < 1.0 / 144.0:
        xy, det = 0.0, x2 * y2
    half, dif = 0.5 * (x2 + y2), x2 - y2
    root = math.sqrt(max(0.25 * (dif * dif) + xy * xy, 0.0))
    a, b = math.sqrt(half + root), math.sqrt(max(half - root, 1.0 / 12.0))
    npix = int(yy.size)
    mthresh = 0.0
    if npix >= minarea:
        mthresh = max(float(np.sort(s)[npix - minarea]) - float(F32(thresh)), 0.0)
    unit = math.pi * a * b
    return dict(s0=s0, x=float(xmin) + mx, y=float(ymin) + my, a=a, cxx=y2 / det, cyy=x2 / det, cxy=-2.0 * xy / det,
                npix=npix, unit=unit, amp=(t * (1.0 / E.FIX)) / (2.0 * unit), mthresh=mthresh)


def clean_targets(shapes, thresh, sequential=False):
    """Item 5: target[i] = the object i merges into, or -1.  ``sequential``: item 6 of "Source masking" as it stands,
    faintest first with the "not yet merged" condition, which item 5 (c) says never acts."""
    n = len(shapes)
    target = [-1] * n
    if n < 2:
        return target
    th = float(F32(thresh))
    order = range(n)
    if sequential:
        order = sorted((i for i in range(n) if shapes[i] is not None), key=lambda i: (shapes[i]['s0'], i))
    for i in order:
        me = shapes[i]
        if me is None:
            continue
        best, into = 0.0, -1
        for j in range(n):
            o = shapes[j]
            if j == i or o is None or o['s0'] <= me['s0'] or (sequential and target[j] >= 0):
                continue
            dx, dy = me['x'] - o['x'], me['y'] - o['y']
            zone = CLEAN_ZONE * (me['a'] + o['a'])
            if dx * dx + dy * dy >= zone * zone:
                continue
            ratio = o['amp'] / th
            if ratio <= 1.0:
                continue
            alpha = (ratio - 1.0) * o['unit'] / float(o['npix'])
            val = 1.0 + alpha * (o['cxx'] * dx * dx + o['cyy'] * dy * dy + o['cxy'] * dx * dy)
            wing = o['amp'] / val if 1.0 < val < 1e10 else 0.0
            if wing > me['mthresh'] and wing > best:
                best, into = wing, j
        target[i] = into
    return target


def extract(data, var, thresh, minarea=5, filt=1, deblend_nthresh=32, deblend_cont=0.005, clean=True, max_objects=None):
    """One frame.  -> dict(objects, nobj, segmap, mask, status, snr, paths, parents (deblend_parents), sets: the final
    pixel sets [(yy, xx)], targets: of the objects before clean, sequential_targets)."""
    d = np.asarray(data, dtype=F32)
    h, w = d.shape
    base = E.extract(d, var, thresh, minarea, filt)
    snr = base['snr']
    parents = deblend_parents(snr, base['segmap'], base['nobj'], thresh, deblend_nthresh, float(F32(deblend_cont)))
    sets = []
    for p in parents:
        y0, x0 = p['sl'][0].start, p['sl'][1].start
        for m in p['leaves']:
            yy, xx = np.nonzero(m)
            sets.append([yy + y0, xx + x0, p['nodeblend'] != ''])
    sets.sort(key=lambda s: int(s[0][0]) * w + int(s[1][0]))
    paths = dict(split=sum(len(p['leaves']) > 1 for p in parents), depth=max([p['depth'] for p in parents] + [0]),
                 merged=0, chain=0, nodeblend_size=sum(p['nodeblend'] == 'size' for p in parents),
                 nodeblend_capacity=sum(p['nodeblend'] == 'capacity' for p in parents))
    targets = sequential = [-1] * len(sets)
    if clean and len(sets) >= 2:
        shapes = [clean_shape(snr, yy, xx, thresh, minarea) for yy, xx, _ in sets]
        targets = clean_targets(shapes, thresh)
        sequential = clean_targets(shapes, thresh, sequential=True)
        paths['merged'] = sum(t >= 0 for t in targets)
        paths['chain'] = sum(t >= 0 and targets[t] >= 0 for t in targets)
        union = {}
        for i in range(len(sets)):
            j = i
            while targets[j] >= 0:
                j = targets[j]
            union.setdefault(j, []).append(i)
        merged = []
        for members in union.values():
            yy = np.concatenate([sets[i][0] for i in members])
            xx = np.concatenate([sets[i][1] for i in members])
            order = np.lexsort((xx, yy))
            merged.append([yy[order], xx[order], any(sets[i][2] for i in members)])
        sets = sorted(merged, key=lambda s: int(s[0][0]) * w + int(s[1][0]))
    segmap = np.zeros((h, w), np.int32)
    objs = []
    for num, (yy, xx, nodeblend) in enumerate(sets, start=1):
        segmap[yy, xx] = num
        if max_objects is None or num <= max_objects:
            o = E.measure(d, snr, yy, xx, h, w)
            if nodeblend:
                o['flag'] |= FLAG_NODEBLEND
            objs.append(o)
    nobj = len(sets)
    objects = np.array(objs, E.OBJECT_DTYPE) if objs else np.zeros(0, E.OBJECT_DTYPE)
    status = 1 if max_objects is not None and nobj > max_objects else 0
    return dict(objects=objects, nobj=nobj, segmap=segmap, mask=(segmap > 0).astype(np.uint8), status=status, snr=snr,
                paths=paths, parents=parents, sets=[(yy, xx) for yy, xx, _ in sets], targets=targets,
                sequential_targets=sequential, base=base)


# ---- scenes -------------------------------------------------------------------------------------------------------------

MERGE_SETTINGS = dict(minarea=15, deblend_cont=0.001)      # on the mosaics these give clean merges; sep's defaults none


def mosaic(rows, cols, n=32, seed=1):
    """(a) rows x cols stamps of _segment.make_scenes pasted into one frame: (data, var) float32, var = noise map^2."""
    d, s, _ = S.make_scenes(rows * cols, n, seed)
    data = np.zeros((rows * n, cols * n), F32)
    var = np.ones((rows * n, cols * n), F32)
    for k in range(rows * cols):
        r, c = divmod(k, cols)
        data[r * n:(r + 1) * n, c * n:(c + 1) * n] = d[k]
        var[r * n:(r + 1) * n, c * n:(c + 1) * n] = s[k] * s[k]
    return data, var


def pairs_scene(h, w, nstars, npairs, seed, sky_rms=3.0, exptime=30.0, sigma=2.0):
    """(b) _extract.fast_scene with npairs close pairs added away from the borders: (sub, var, pairs) with pairs
    (npairs, 2, 2) the (x, y) of both stars of every pair."""
    sub, _ = E.fast_scene(h, w, nstars, seed, sky_rms, exptime, sigma)
    rng = np.random.default_rng(seed + 7919)
    img = sub.astype(np.float64)
    r = int(math.ceil(6 * sigma)) + 8
    pairs = np.zeros((npairs, 2, 2))
    for k in range(npairs):
        cx, cy = rng.uniform(r, w - r), rng.uniform(r, h - r)
        ang, dist = rng.uniform(0, 2 * np.pi), rng.uniform(2.6, 3.6) * sigma
        pairs[k] = (cx, cy), (cx + dist * np.cos(ang), cy + dist * np.sin(ang))
        peak = math.exp(rng.uniform(math.log(400.0), math.log(3000.0)))
        for (px, py), amp in zip(pairs[k], (peak, peak * rng.uniform(0.4, 0.9))):
            x0, x1, y0, y1 = max(int(px) - r, 0), min(int(px) + r + 1, w), max(int(py) - r, 0), min(int(py) + r + 1, h)
            y, x = np.mgrid[y0:y1, x0:x1].astype(np.float64)
            img[y0:y1, x0:x1] += amp * np.exp(-((x - px) ** 2 + (y - py) ** 2) / (2.0 * sigma ** 2))
    sub = img.astype(F32)
    return sub, E.variance_map(sub, sky_rms, exptime), pairs


def _blob(img, cx, cy, amp, sigma):
    h, w = img.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma ** 2))


# (c) hand-made frames: filter 0 and variance 1, so that snr is the frame itself.  name -> (frame, settings)
HAND_BASE = dict(thresh=3.0, minarea=5, filt=0)
HAND_MADE = ('straddle', 'box64', 'box65', 'overflow', 'chain', 'small_children', 'edge_blend', 'noise_only')


@functools.lru_cache(maxsize=None)
def hand_made(name):
    s = dict(HAND_BASE)
    if name == 'straddle':          # a blend across the corner of four 64 x 16 tiles, where a block of 256 pixels ends too
        img = np.zeros((40, 300))   # raster index 16 * 300 + 64 = 19 * 256
        _blob(img, 60.5, 15.0, 60.0, 2.0)
        _blob(img, 67.5, 17.0, 35.0, 2.0)
    elif name in ('box64', 'box65'):    # a bar with a star at each end: the box is 64 (de-blended) or 65 wide (kept whole)
        wide = 64 if name == 'box64' else 65
        img = np.zeros((30, 100))
        img[10:15, 10:10 + wide] = 4.0
        for cx in (13, 10 + wide - 4):
            img[11:14, cx - 1:cx + 2] = 20.0
            img[12, cx] = 50.0
    elif name == 'overflow':        # 49 plateaus on a faint bridge: one parent of 64 x 64 with more than 32 leaves
        d, _ = S.crowded_stamp()
        img = np.zeros((80, 80))
        img[8:72, 8:72] = d.astype(np.float64) + 3.5
    elif name == 'chain':           # i -> j -> k: a line of 5 pixels, a 3 x 3 and a bright 5 x 5, each barely above thresh
        img = np.zeros((30, 40))
        img[10:15, 10] = 3.01
        img[11:14, 13:16] = 3.01
        img[10:15, 18:23] = 100.0
    elif name == 'small_children':  # a bright block with a spike of 1 and one of 2 pixels on faint one-pixel bridges
        img = np.zeros((30, 40))
        img[9:16, 12:17] = 20.0
        img[12, 14] = 30.0
        img[12, 11] = img[12, 17] = 3.5
        img[12, 10] = 40.0
        img[12:14, 18] = 40.0
        s.update(clean=False)       # clean merges a child below minarea (its mthresh is 0) into the block
    elif name == 'edge_blend':
        img = np.zeros((40, 50))
        _blob(img, 1.0, 20.0, 60.0, 2.0)
        _blob(img, 7.5, 21.0, 40.0, 2.0)
        _blob(img, 30.0, 0.0, 50.0, 2.0)
        _blob(img, 36.0, 1.0, 50.0, 2.0)
    elif name == 'noise_only':
        img = np.random.default_rng(5).normal(0.0, 1.0, (70, 90))
    else:
        raise ValueError(name)
    return img.astype(F32), s


@functools.lru_cache(maxsize=None)
def hand_made_wanted(name):
    img, s = hand_made(name)
    return extract(img, F32(1.0), **s)
