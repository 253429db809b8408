"""Checker for lc_register_sources: a float64 NumPy restatement of the SPEC of DESIGN.md §5 ("Frame registration"), the
generator of its random cases and the rendered frames of the end-to-end test.

Not part of the product path.  ``register`` follows the SPEC step by step: every elementwise operation is one float64
rounding (NumPy never fuses a product into a sum), the sums are ``numpy.sum``.  The device must give its decisions (the
triangles, the matches, the winning hypothesis, the inliers, the pairs) and its transform but for the order of the sums.
It also returns its decision margins: how far the closest comparison was from going the other way."""
import itertools
import math

import numpy as np

NUM_NEAREST_NEIGHBORS = 5
PIXEL_TOL = 2.0
INVARIANT_RADIUS = 0.1
MIN_MATCHES_FRACTION = 0.8
MAX_MATCHES = 65536
OPPOSITE = (2, 0, 1)          # the vertex of (p0, p1, p2) that the sides p0p1, p1p2, p0p2 do not touch


def _gap(margins, values):
    """Relative gaps between neighbours of the ascending squared distances ``values``; exact ties do not count."""
    v = np.asarray(values, np.float64)
    g = v[1:] - v[:-1]
    ok = g > 0
    if ok.any():
        margins['d2'] = min(margins['d2'], float((g[ok] / v[1:][ok]).min()))


def _d2(p, q):
    dx, dy = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1]
    return dx * dx + dy * dy


def triangles(P, margins=None):
    """Step 1.  Returns (vertices int (T, 3) in the order a, b, c; invariants float64 (T, 2))."""
    P = np.asarray(P, np.float64).reshape(-1, 2)
    margins = margins if margins is not None else new_margins()
    n = len(P)
    k = min(n, NUM_NEAREST_NEIGHBORS)
    verts, invs = [], []
    for i in range(n):
        d2 = _d2(P, P[i])
        order = np.argsort(d2, kind='stable')          # ties: the lower index
        _gap(margins, d2[order[:k + 1]])
        for cmb in itertools.combinations([int(t) for t in order[:k]], 3):
            p0, p1, p2 = P[cmb[0]], P[cmb[1]], P[cmb[2]]
            s2 = np.array([_d2(p0, p1), _d2(p1, p2), _d2(p0, p2)])
            sides = np.sqrt(s2)
            o = np.argsort(sides, kind='stable')
            _gap(margins, s2[o])
            L1, L2, L3 = sides[o]
            if L1 == 0:
                continue
            verts.append((cmb[OPPOSITE[o[2]]], cmb[OPPOSITE[o[0]]], cmb[OPPOSITE[o[1]]]))
            invs.append((L3 / L2, L2 / L1))
    keep, seen = [], set()
    for t in range(len(verts) - 1, -1, -1):              # dropped if a LATER one has the same vertex set
        key = frozenset(verts[t])
        if key not in seen:
            seen.add(key)
            keep.append(t)
    keep.reverse()
    return (np.array([verts[t] for t in keep], np.int64).reshape(-1, 3),
            np.array([invs[t] for t in keep], np.float64).reshape(-1, 2))


def match_triangles(inv_s, inv_t, radius=INVARIANT_RADIUS, margins=None):
    """Step 2: the (i, j) of every pair of triangles within ``radius``, by i, then j."""
    if not len(inv_s) or not len(inv_t):
        return np.zeros((0, 2), np.int64)
    dx = inv_s[:, None, 0] - inv_t[None, :, 0]
    dy = inv_s[:, None, 1] - inv_t[None, :, 1]
    dist = np.sqrt(dx * dx + dy * dy)
    if margins is not None:
        margins['radius'] = min(margins['radius'], float(np.abs(dist - radius).min()))
    i, j = np.nonzero(dist <= radius)
    return np.stack([i, j], axis=1)


def fit(s, t):
    """Step 3 on pairs s, t (m, 2).  Returns (a, b, tx, ty), or None for an empty set or d == 0."""
    s, t = np.asarray(s, np.float64).reshape(-1, 2), np.asarray(t, np.float64).reshape(-1, 2)
    m = len(s)
    if m == 0:
        return None
    msx, msy, mtx, mty = s[:, 0].sum() / m, s[:, 1].sum() / m, t[:, 0].sum() / m, t[:, 1].sum() / m
    sx, sy, tx, ty = s[:, 0] - msx, s[:, 1] - msy, t[:, 0] - mtx, t[:, 1] - mty
    A = (sx * tx + sy * ty).sum()
    B = (sx * ty - sy * tx).sum()
    d = (sx * sx + sy * sy).sum()
    if d == 0:
        return None
    a, b = A / d, B / d
    return a, b, mtx - (a * msx - b * msy), mty - (b * msx + a * msy)


def vertex_errors(tr, s, t):
    """|M s + t - t_q| of points s against t_q (both (..., 2))."""
    a, b, tx, ty = tr
    ex = a * s[..., 0] - b * s[..., 1] + tx - t[..., 0]
    ey = b * s[..., 0] + a * s[..., 1] + ty - t[..., 1]
    return np.sqrt(ex * ex + ey * ey)


def new_margins():
    return dict(d2=math.inf, radius=math.inf, error=math.inf)


def register(S, T, max_matches=MAX_MATCHES, pixel_tol=PIXEL_TOL, radius=INVARIANT_RADIUS, fraction=MIN_MATCHES_FRACTION):
    """One problem.  Returns dict(status, transform (6,): a, -b, tx, b, a, ty (NaN unless status 0), pairs int (npairs, 2),
    diag (5,): source triangles, target triangles, matches, winning hypothesis or -1, final inlier matches; margins)."""
    S, T = np.asarray(S, np.float64).reshape(-1, 2), np.asarray(T, np.float64).reshape(-1, 2)
    margins = new_margins()
    out = dict(status=0, transform=np.full(6, np.nan), pairs=np.zeros((0, 2), np.int64),
               diag=np.array([0, 0, 0, -1, 0], np.int64), margins=margins)

    def fail(status):
        out['status'] = status
        return out

    if len(S) < 3 or len(T) < 3:
        return fail(3)
    vs, inv_s = triangles(S, margins)
    vt, inv_t = triangles(T, margins)
    ij = match_triangles(inv_s, inv_t, radius, margins)
    n = len(ij)
    out['diag'][:3] = len(vs), len(vt), n
    if n > max_matches:
        return fail(2)
    if n == 0:
        return fail(1)
    ms, mt = vs[ij[:, 0]], vt[ij[:, 1]]              # (n, 3) vertex indices
    ps, pt = S[ms], T[mt]                            # (n, 3, 2)

    def errors(tr):
        e = vertex_errors(tr, ps, pt)
        margins['error'] = min(margins['error'], float(np.abs(e - pixel_tol).min()))
        return e.max(axis=1)

    if (len(S) == 3 or len(T) == 3) and n == 1:
        cur = fit(ps[0], pt[0])
        if cur is None:
            return fail(1)
        winner, inl = 0, np.array([0])
    else:
        min_matches = max(1, min(10, int(fraction * n)))
        winner = -1
        for h in range(n):
            tr = fit(ps[h], pt[h])
            if tr is None:
                continue
            ok = errors(tr) < pixel_tol
            ok[h] = False
            if int(ok.sum()) >= min_matches:
                winner = h
                ok[h] = True
                break
        if winner < 0:
            return fail(1)
        cur = fit(ps[ok].reshape(-1, 2), pt[ok].reshape(-1, 2))
        for _ in range(3):
            if cur is None:
                return fail(1)
            inl = np.nonzero(errors(cur) < pixel_tol)[0]
            cur = fit(ps[inl].reshape(-1, 2), pt[inl].reshape(-1, 2))
        if cur is None:
            return fail(1)
    best = {}
    for s_i, t_i in sorted(set(zip(ms[inl].ravel().tolist(), mt[inl].ravel().tolist()))):
        e = float(vertex_errors(cur, S[s_i], T[t_i]))
        if s_i not in best or e < best[s_i][1]:         # visited by ascending t: a tie keeps the lower one
            best[s_i] = (t_i, e)
    a, b, tx, ty = cur
    out['transform'] = np.array([a, -b, tx, b, a, ty])
    out['pairs'] = np.array([(s_i, best[s_i][0]) for s_i in sorted(best)], np.int64).reshape(-1, 2)
    out['diag'][3:] = winner, len(inl)
    return out


def umeyama(s, t):
    """skimage's estimate_transform('similarity') (Umeyama 1991) through numpy.linalg.svd: the 3 x 3 matrix."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    m, dim = s.shape
    ms, mt = s.mean(axis=0), t.mean(axis=0)
    sc, tc = s - ms, t - mt
    A = tc.T @ sc / m
    d = np.ones(dim)
    if np.linalg.det(A) < 0:
        d[dim - 1] = -1
    U, sv, Vt = np.linalg.svd(A)
    R = U @ np.diag(d) @ Vt
    scale = (sv @ d) / sc.var(axis=0).sum()
    M = np.eye(3)
    M[:2, :2] = scale * R
    M[:2, 2] = mt - scale * (R @ ms)
    return M


# ---- cases ---------------------------------------------------------------------------------------------------------------

FIELD = 2000.0


def field_case(N, rotation_deg, scale, sigma, replaced, seed, shift=(37.5, -21.25), n_target=None):
    """A field of N random points as the source; the target is the field rotated about its centre, scaled, shifted and
    jittered by sigma, with a fraction ``replaced`` of its points replaced by spurious ones and its order perturbed (a few
    neighbouring rows swapped, as the brightness order of two exposures differs).  ``n_target``: the target is a field of
    that many points whose first min(N, n_target) are the source's.  Returns (S, T, (a, b, tx, ty))."""
    rng = np.random.default_rng(seed)
    M = max(N, n_target or N)
    pts = rng.uniform(0.0, FIELD, (M, 2))
    th = math.radians(rotation_deg)
    a, b = scale * math.cos(th), scale * math.sin(th)
    c = FIELD / 2
    tx = c - (a * c - b * c) + shift[0]
    ty = c - (b * c + a * c) + shift[1]
    S = pts[:N].copy()
    nt = n_target or N
    T = np.stack([a * pts[:nt, 0] - b * pts[:nt, 1] + tx, b * pts[:nt, 0] + a * pts[:nt, 1] + ty], axis=1)
    T += rng.normal(0.0, sigma, T.shape)
    bad = rng.choice(nt, int(round(replaced * nt)), replace=False)
    T[bad] = rng.uniform(T.min(), T.max(), (len(bad), 2))
    for i in rng.choice(nt - 1, max(nt // 5, 1), replace=False):
        T[[i, i + 1]] = T[[i + 1, i]]
    return S, T, (a, b, tx, ty)


def unrelated_case(N, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, FIELD, (N, 2)), rng.uniform(0.0, FIELD, (N, 2))


def lattice_case(nx=5, ny=4, pitch=10.0, shear=1, shift=(30.0, -20.0)):
    """An integer lattice and its image under an integer shear and shift: every squared distance is exact, neighbours tie
    and triangles are congruent in numbers."""
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    S = np.stack([x.ravel(), y.ravel()], axis=1) * pitch
    T = np.stack([S[:, 0] + shear * S[:, 1] + shift[0], S[:, 1] + shift[1]], axis=1)
    return S, T


# name -> (S, T, max_matches, truth or None, expected status); the seeds are chosen so that the margins hold
def cases():
    out = {}
    table = [('n50_plain', 50, 0.0, 1.0, 0.1, 0.0), ('n50_rot25', 50, 25.0, 1.02, 0.3, 0.3),
             ('n50_rot170', 50, 170.0, 0.98, 0.3, 0.3), ('n12_rot40', 12, 40.0, 1.0, 0.2, 0.2),
             ('n6_rot10', 6, 10.0, 1.0, 0.1, 0.0), ('n50_scale1p5', 50, 3.0, 1.5, 0.3, 0.2),
             ('n50_rot90', 50, 90.0, 1.0, 0.5, 0.4)]
    for name, N, rot, sc, sig, rep in table:
        S, T, truth = field_case(N, rot, sc, sig, rep, seed=SEEDS[name])
        out[name] = (S, T, MAX_MATCHES, truth, 0)
    for name, N in (('n3', 3), ('n4', 4), ('n5', 5)):
        S, T, truth = field_case(N, 15.0, 1.0, 0.05, 0.0, seed=SEEDS[name])
        out[name] = (S, T, MAX_MATCHES, truth, 0)
    S, T, truth = field_case(50, 12.0, 1.0, 0.2, 0.1, seed=SEEDS['n128_vs_50'], n_target=128)
    out['n128_vs_50'] = (T, S, MAX_MATCHES, None, 0)                # 128 points against 50: the inverse of truth
    out['n128_cut_to_50'] = (T[:50], S, MAX_MATCHES, None, 0)       # what max_control_points = 50 makes of it
    S, T, truth = field_case(50, 12.0, 1.0, 0.1, 0.0, seed=SEEDS['n7_vs_50'])
    clump = np.argsort(_d2(S, S[0]), kind='stable')[:7]            # a star and its six nearest: 7 points against 50
    out['n7_vs_50'] = (S[clump], T, MAX_MATCHES, truth, 0)
    S, T = unrelated_case(50, seed=SEEDS['unrelated'])
    out['unrelated'] = (S, T, MAX_MATCHES, None, 1)
    out['n12_vs_unrelated'] = (out['n12_rot40'][0], T, MAX_MATCHES, None, 1)
    out['two_points'] = (out['n12_rot40'][0][:2], out['n12_rot40'][1], MAX_MATCHES, None, 3)
    out['too_many'] = (out['n50_plain'][0], out['n50_plain'][1], 64, None, 2)
    S, T = lattice_case()
    out['lattice'] = (S, T, MAX_MATCHES, None, None)
    return out


SEEDS = dict(n50_plain=104, n50_rot25=102, n50_rot170=103, n12_rot40=104, n6_rot10=105, n50_scale1p5=106, n50_rot90=107,
             n3=108, n4=200, n5=200, n128_vs_50=111, n7_vs_50=300, unrelated=113)

_solved = {}


def solved(name):
    """The restatement's result of a case, computed once and shared."""
    if name not in _solved:
        S, T, mm = cases()[name][:3]
        _solved[name] = register(S, T, max_matches=mm)
    return _solved[name]


# ---- the end-to-end frames --------------------------------------------------------------------------------------------------

def rendered_frames(h=256, w=256, nstars=40, seed=5, sigma=1.8, sky_rms=1.0):
    """Four frames of one field of Gaussian stars: the identity, rotated 20 degrees about the centre, shifted (9.3, -6.8)
    px with a quarter of the stars removed, and an unrelated field.  Returns (stack float32 (4, h, w), centres: list of
    four (n_k, 2) arrays of the true (x, y) of the stars inside each frame, truth: the (a, b, tx, ty) of frames 0 - 2 from
    frame 0, reference_xy: the field's stars in frame 0)."""
    rng = np.random.default_rng(seed)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    # stars on a jittered grid over a disc that stays inside every frame, so that no two blend
    side = int(math.ceil(math.sqrt(nstars * 4 / math.pi))) + 1
    r_max = min(h, w) / 2.0 - 26.0
    cand = []
    for gy in range(side):
        for gx in range(side):
            px = cx - r_max + (gx + 0.5) * 2 * r_max / side + rng.uniform(-3.0, 3.0)
            py = cy - r_max + (gy + 0.5) * 2 * r_max / side + rng.uniform(-3.0, 3.0)
            if math.hypot(px - cx, py - cy) < r_max:
                cand.append((px, py))
    cand = np.array(cand)
    field = cand[rng.permutation(len(cand))[:nstars]]
    peaks = np.exp(rng.uniform(math.log(300.0), math.log(3000.0), len(field)))
    th = math.radians(20.0)
    ca, sa = math.cos(th), math.sin(th)
    truth = [(1.0, 0.0, 0.0, 0.0), (ca, sa, cx - (ca * cx - sa * cy), cy - (sa * cx + ca * cy)), (1.0, 0.0, 9.3, -6.8)]
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)

    def render(xy, pk, k):
        img = np.random.default_rng(seed + 100 + k).normal(0.0, sky_rms, (h, w))
        for (px, py), p in zip(xy, pk):
            img += p * np.exp(-((x - px) ** 2 + (y - py) ** 2) / (2.0 * sigma ** 2))
        return img

    stack, centres = [], []
    for k, (a, b, tx, ty) in enumerate(truth):
        xy = np.stack([a * field[:, 0] - b * field[:, 1] + tx, b * field[:, 0] + a * field[:, 1] + ty], axis=1)
        keep = np.ones(len(field), bool)
        if k == 2:
            keep[rng.choice(len(field), len(field) // 4, replace=False)] = False
        stack.append(render(xy[keep], peaks[keep], k))
        centres.append(xy[keep])
    other = np.stack([rng.uniform(20, w - 20, nstars), rng.uniform(20, h - 20, nstars)], axis=1)
    stack.append(render(other, np.exp(rng.uniform(math.log(300.0), math.log(3000.0), nstars)), 3))
    centres.append(other)
    return np.stack(stack).astype(np.float32), centres, truth, field


EXPTIME = 30.0
_rendered = {}


def rendered():
    """rendered_frames() once, with the restated import of every frame beside it: dict(stack, centres, truth, field,
    tables: per frame the (n, 2) positions of tests/_extract.extract, brightest first, as register_frames orders them)."""
    if not _rendered:
        from . import _background as B
        from . import _extract as E
        stack, centres, truth, field = rendered_frames()
        tables = []
        for frame in stack:
            box = min(frame.shape) // 10
            bg = B.background(frame, bw=box, bh=box)
            sub = bg['sub'].astype(np.float32)
            o = E.extract(sub, E.variance_map(sub, bg['globalrms'], EXPTIME), 3.0, 10)['objects']
            o = o[np.isfinite(o['x']) & np.isfinite(o['y'])]
            o = o[np.argsort(-o['flux'], kind='stable')]
            tables.append(np.stack([o['x'], o['y']], axis=1))
        _rendered.update(stack=stack, centres=centres, truth=truth, field=field, tables=tables)
    return _rendered


def worst_centroid_error():
    """The largest distance of a true star centre of frames 0 - 2 from the nearest object of the restated extraction."""
    r = rendered()
    worst = 0.0
    for k in range(3):
        d = np.sqrt(((r['centres'][k][:, None, :] - r['tables'][k][None, :, :]) ** 2).sum(axis=2))
        worst = max(worst, float(d.min(axis=1).max()))
    return worst
