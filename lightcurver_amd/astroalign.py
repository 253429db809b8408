"""``find_transform`` with astroalign's signature for lists of points, on the device (``lc_register_sources``,
include/lcmi.h).

The reference gives a frame its WCS from another frame's, or from Gaia positions, with one ``astroalign.find_transform``
per frame (lightcurver/processes/alternate_plate_solving_adapt_existing_wcs.py:24, alternate_plate_solving_with_gaia.py:66).
Here the SPEC of DESIGN.md §5 ("Frame registration") runs as HIP kernels, one workgroup per problem:
``find_transforms_batch`` solves every frame of a set in one call, ``find_transform`` is one problem with astroalign's
return value and exceptions.  astroalign visits its hypotheses in a random order; here the order is that of the matches,
which is one of its outcomes.  Parity with astroalign itself is not pinned (it is absent here).  Image inputs, which
astroalign passes through its own source detection, raise ``NotImplementedError``: extract the sources first
(``sep.extract``, ``processes.frame_importation``).  There is no CPU fallback."""
import ctypes as C
import math

import numpy as np

from . import _lib

MAX_CONTROL_POINTS = 50
PIXEL_TOL = 2
MIN_MATCHES_FRACTION = 0.8
NUM_NEAREST_NEIGHBORS = 5
INVARIANT_RADIUS = 0.1          # the radius of astroalign's query_ball_tree, which it does not name
MAX_MATCHES = 65536
MAX_POINTS = 128                # the most control points the kernels take (lc_register_supported)
STATUS_OK, STATUS_NO_CONSENSUS, STATUS_TOO_MANY_MATCHES, STATUS_TOO_FEW_POINTS = 0, 1, 2, 3

_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)


class MaxIterError(RuntimeError):
    """astroalign.MaxIterError: no hypothesis gathered enough matching triangles."""


class SimilarityTransform:
    """The part of skimage.transform.SimilarityTransform that astroalign's callers use: ``params`` (3 x 3, homogeneous),
    ``scale``, ``rotation`` (radians), ``translation``, ``inverse`` and ``transform(coords)`` for (n, 2) coordinates."""

    def __init__(self, matrix=None):
        self.params = np.eye(3) if matrix is None else np.array(matrix, dtype=np.float64).reshape(3, 3)

    @classmethod
    def from_row(cls, row):
        """From the six numbers of ``lc_register_sources``: a, -b, tx, b, a, ty."""
        return cls(np.vstack([np.asarray(row, np.float64).reshape(2, 3), [0.0, 0.0, 1.0]]))

    @property
    def scale(self):
        return math.hypot(self.params[0, 0], self.params[1, 0])

    @property
    def rotation(self):
        return math.atan2(self.params[1, 0], self.params[0, 0])

    @property
    def translation(self):
        return self.params[:2, 2].copy()

    @property
    def inverse(self):
        return SimilarityTransform(np.linalg.inv(self.params))

    def __call__(self, coords):
        c = np.asarray(coords, np.float64).reshape(-1, 2)
        return c @ self.params[:2, :2].T + self.params[:2, 2]


def supported(max_control_points):
    """True if the kernels take that many control points (3 .. 128; no device needed)."""
    return bool(_lib.lib().lc_register_supported(int(max_control_points)))


def _is_one_list(side):
    """One (n, 2) list of points, as against a sequence of such lists."""
    if isinstance(side, np.ndarray):
        return side.ndim == 2
    return len(side) == 0 or np.ndim(side[0]) <= 1


def _control_points(points, max_control_points):
    """(the first max_control_points rows with finite x and y, their row numbers)."""
    p = np.asarray(points, np.float64)
    if p.size == 0:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise NotImplementedError('find_transform takes (n, 2) lists of (x, y) points; images, which astroalign passes '
                                  'through its own source detection, are not built')
    rows = np.nonzero(np.isfinite(p).all(axis=1))[0][:max_control_points]
    return p[rows], rows


def find_transforms_batch(sources, targets, max_control_points=MAX_CONTROL_POINTS, max_matches=MAX_MATCHES,
                          pixel_tol=PIXEL_TOL, min_matches_fraction=MIN_MATCHES_FRACTION, ctx=None):
    """K problems in one device call.  ``sources``, ``targets``: a sequence of K (n, 2) lists of (x, y), brightest first, or
    one such list shared by all problems (one side at least must be a sequence).  Rows with a non-finite x or y are dropped,
    then the first ``max_control_points`` are taken.  Never raises for a frame that fails: returns dict(transform float64
    (K, 6): a, -b, tx, b, a, ty with target = [[a, -b], [b, a]] source + (tx, ty), NaN where status != 0; transforms: list
    of ``SimilarityTransform`` or None; pairs: list of int (npairs, 2) arrays of matched (source row, target row) in the
    caller's numbering, by source row; diag int32 (K, 5): source triangles, target triangles, matching triangle pairs,
    winning hypothesis or -1, final inlier matches; status int32 (K,): 0 solved, 1 no consensus, 2 more than
    ``max_matches`` matching triangle pairs, 3 fewer than three points on a side; kernel_ms)."""
    mcp = int(max_control_points)
    if mcp > MAX_POINTS:
        raise NotImplementedError(f'find_transform: more than {MAX_POINTS} control points are not built')
    if mcp < 1:
        raise ValueError(f'max_control_points = {max_control_points}')
    one_s, one_t = _is_one_list(sources), _is_one_list(targets)
    if one_s and one_t:
        sources, one_s = [sources], False
    K = len(targets) if one_s else len(sources)
    if not one_s and not one_t and len(sources) != len(targets):
        raise ValueError(f'{len(sources)} source lists against {len(targets)} target lists')
    shared_s = _control_points(sources, mcp) if one_s else None
    shared_t = _control_points(targets, mcp) if one_t else None
    S = [shared_s if one_s else _control_points(sources[k], mcp) for k in range(K)]
    T = [shared_t if one_t else _control_points(targets[k], mcp) for k in range(K)]
    out = dict(transform=np.full((K, 6), np.nan), transforms=[None] * K, pairs=[np.zeros((0, 2), np.int64)] * K,
               diag=np.zeros((K, 5), np.int32), status=np.zeros(K, np.int32), kernel_ms=0.0)
    if not K:
        return out
    P = max(3, max(len(p) for p, _ in S + T))
    src, tgt = np.zeros((K, P, 2)), np.zeros((K, P, 2))
    ns, nt = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for k in range(K):
        ns[k], nt[k] = len(S[k][0]), len(T[k][0])
        src[k, :ns[k]], tgt[k, :nt[k]] = S[k][0], T[k][0]
    cfg = _lib.RegisterCfg(int(max_matches), float(pixel_tol), INVARIANT_RADIUS, float(min_matches_fraction))
    pairs = np.empty((K, P, 2), np.int32)
    npairs = np.zeros(K, np.int32)
    ms = C.c_float()
    ctx = ctx or _lib.default_context()
    ctx.check(_lib.lib().lc_register_sources(
        ctx.h, K, P, src.ctypes.data_as(_f64p), ns.ctypes.data_as(_i32p), tgt.ctypes.data_as(_f64p), nt.ctypes.data_as(_i32p),
        C.byref(cfg), out['transform'].ctypes.data_as(_f64p), pairs.ctypes.data_as(_i32p), npairs.ctypes.data_as(_i32p),
        out['diag'].ctypes.data_as(_i32p), out['status'].ctypes.data_as(_i32p), C.byref(ms)), 'lc_register_sources')
    out['kernel_ms'] = ms.value
    out['pairs'] = []
    for k in range(K):
        pr = pairs[k, :npairs[k]].astype(np.int64)
        out['pairs'].append(np.stack([S[k][1][pr[:, 0]], T[k][1][pr[:, 1]]], axis=1))
        if out['status'][k] == 0:
            out['transforms'][k] = SimilarityTransform.from_row(out['transform'][k])
    return out


def find_transform(source, target, max_control_points=MAX_CONTROL_POINTS, detection_sigma=5, min_area=5, ctx=None):
    """astroalign.find_transform for two lists of (x, y) points: returns ``(transform, (source_points, target_points))``,
    the matched points as (npairs, 2) arrays.  Raises ``ValueError`` with fewer than three points on a side,
    ``MaxIterError`` without a consensus (and for more matching triangle pairs than ``MAX_MATCHES``, which astroalign would
    grind through), ``NotImplementedError`` for image inputs and more than 128 control points.  ``detection_sigma`` and
    ``min_area`` belong to the image inputs and are accepted for signature compatibility only."""
    s, t = np.asarray(source, np.float64), np.asarray(target, np.float64)
    r = find_transforms_batch([s], [t], max_control_points, ctx=ctx)
    status = int(r['status'][0])
    if status == STATUS_TOO_FEW_POINTS:
        side = 'source' if np.isfinite(s.reshape(-1, 2)).all(axis=1).sum() < 3 else 'target'
        raise ValueError(f'Reference stars in {side} image are less than the minimum value (3).')
    if status == STATUS_TOO_MANY_MATCHES:
        raise MaxIterError(f'more than {MAX_MATCHES} matching triangle pairs: the lists are too regular to register')
    if status != STATUS_OK:
        raise MaxIterError('List of matching triangles exhausted before an acceptable transformation was found')
    pr = r['pairs'][0]
    return r['transforms'][0], (s.reshape(-1, 2)[pr[:, 0]], t.reshape(-1, 2)[pr[:, 1]])
