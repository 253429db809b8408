"""The geometry the reference does on sky footprints (lightcurver/utilities/footprint.py and
processes/frame_star_assignment.py), restated on pixel positions of a reference frame: host NumPy in float64, no device.

The reference takes ``WCS.calc_footprint`` of every plate-solved frame and hands the quadrilaterals to shapely.  Here a
frame's astrometry is the similarity transform of ``plate_solving.register_frames`` (reference pixels -> the frame's
pixels), its footprint the frame's outer pixel centres brought back into reference pixels through the inverse, and the
polygon work is written out (shapely is not a dependency): the quadrilaterals are convex, since the transforms are
similarities, so the intersection is Sutherland-Hodgman clipping and membership a sign test per edge.  Positions are
(x, y) with the pixel centres at integers throughout."""
import math

import numpy as np


def _matrix_of(result):
    """The 3 x 3 matrix of a result of ``register_frames``, of a transform (anything with ``params``) or of an array;
    None for a frame that failed."""
    t = result
    if isinstance(result, dict):
        if not result.get('success', result.get('transform') is not None):
            return None
        t = result['transform']
    if t is None:
        return None
    m = np.asarray(getattr(t, 'params', t), dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError(f'expected a transform or a 3 x 3 matrix, got an array of shape {m.shape}')
    return m if np.isfinite(m).all() else None


def frame_footprints(results, frame_shape):
    """(K, 4, 2): the corners (0, 0), (w-1, 0), (w-1, h-1), (0, h-1) of the outer pixel centres of every frame, in pixels of
    the reference frame (through the inverse of the frame's transform); NaN for a frame that failed.  ``results``: what
    ``register_frames`` returns, or transforms / 3 x 3 matrices; ``frame_shape``: (rows, columns) = (h, w).  Stands in for
    ``WCS.calc_footprint``."""
    h, w = (int(v) for v in frame_shape)
    corners = np.array([[0.0, 0.0], [w - 1.0, 0.0], [w - 1.0, h - 1.0], [0.0, h - 1.0]])
    out = np.full((len(results), 4, 2), np.nan)
    for k, r in enumerate(results):
        m = _matrix_of(r)
        if m is None:
            continue
        inv = np.linalg.inv(m)
        out[k] = corners @ inv[:2, :2].T + inv[:2, 2]
    return out


def _signed_area(poly):
    x, y = poly[:, 0], poly[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def _counter_clockwise(poly):
    return poly if _signed_area(poly) >= 0 else poly[::-1]


def _clip(subject, a, b):
    """Sutherland-Hodgman: the part of the convex polygon ``subject`` on the left of (or on) the line a -> b."""
    e = b - a
    side = e[0] * (subject[:, 1] - a[1]) - e[1] * (subject[:, 0] - a[0])
    out = []
    n = len(subject)
    for i in range(n):
        j = (i + 1) % n
        p, q, sp, sq = subject[i], subject[j], side[i], side[j]
        if sp >= 0:
            out.append(p)
        if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
            out.append(p + (q - p) * (sp / (sp - sq)))
    return np.array(out).reshape(-1, 2)


def _finite_footprints(footprints):
    fp = np.asarray(footprints, dtype=np.float64)
    if fp.ndim != 3 or fp.shape[1:] != (4, 2):
        raise ValueError(f'expected footprints of shape (K, 4, 2), got {fp.shape}')
    return fp[np.isfinite(fp).all(axis=(1, 2))]


def common_footprint(footprints):
    """The intersection of the frames' quadrilaterals (K, 4, 2) as a convex polygon (V, 2), counter-clockwise (x to the
    right, y up); None when it is empty (or has no area), or when no frame has a footprint.  Frames whose footprint is NaN
    (no registration) do not take part.  The common half of the reference's ``calc_common_and_total_footprint``; the total
    half (the union polygon) only serves the reference's Gaia query and is not built: ``total_bounds`` gives its
    bounding box."""
    fp = _finite_footprints(footprints)
    if not len(fp):
        return None
    poly = _counter_clockwise(fp[0])
    for quad in fp[1:]:
        quad = _counter_clockwise(quad)
        for i in range(4):
            poly = _clip(poly, quad[i], quad[(i + 1) % 4])
            if len(poly) < 3:
                return None
    # vertices that clipping produced twice (a corner that lies on a clipping line)
    keep = [i for i in range(len(poly)) if np.abs(poly[i] - poly[i - 1]).max() > 0.0]
    poly = poly[keep]
    if len(poly) < 3 or not _signed_area(poly) > 0.0:
        return None
    return poly


def total_bounds(footprints):
    """(xmin, ymin, xmax, ymax) over the corners of all frames that have a footprint: the bounding box of the union of the
    footprints, which is all of the reference's ``largest_footprint`` that is built here.  None without a footprint."""
    fp = _finite_footprints(footprints)
    if not len(fp):
        return None
    lo, hi = fp.reshape(-1, 2).min(axis=0), fp.reshape(-1, 2).max(axis=0)
    return float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1])


def bad_pointings(footprints):
    """(K,) bool, True for a pointing far from the others (the reference's ``identify_and_eliminate_bad_pointings``): the
    distance of each footprint's mean corner from the mean of those over the frames, flagged above the mean + 5 standard
    deviations (population) of the distances.  Frames without a footprint (NaN) take no part and are not flagged."""
    fp = np.asarray(footprints, dtype=np.float64)
    if fp.ndim != 3 or fp.shape[1:] != (4, 2):
        raise ValueError(f'expected footprints of shape (K, 4, 2), got {fp.shape}')
    have = np.isfinite(fp).all(axis=(1, 2))
    out = np.zeros(len(fp), bool)
    if not have.any():
        return out
    centres = fp[have].mean(axis=1)
    distance = np.sqrt(((centres - centres.mean(axis=0)) ** 2).sum(axis=1))
    out[have] = distance > distance.mean() + 5.0 * distance.std()
    return out


def points_in_footprints(points_xy, footprints, margin=0.0):
    """(K, S) bool: whether each of the S points (S, 2) lies strictly inside each frame's quadrilateral shrunk by ``margin``
    pixels the way the reference's ``populate_stars_in_frames`` shrinks it: the intersection of the four copies translated
    by +-margin along x and along y, so a point is inside when p + (margin, 0), p - (margin, 0), p + (0, margin) and
    p - (0, margin) all are.  (The reference's 4 arcseconds become the caller's number of pixels.)  ``margin = 0`` is the
    test of the ROI (``check_in_footprint_for_all_images``).  False for a frame without a footprint (NaN)."""
    fp = np.asarray(footprints, dtype=np.float64)
    if fp.ndim != 3 or fp.shape[1:] != (4, 2):
        raise ValueError(f'expected footprints of shape (K, 4, 2), got {fp.shape}')
    p = np.asarray(points_xy, dtype=np.float64).reshape(-1, 2)
    m = float(margin)
    if not m >= 0.0:
        raise ValueError(f'the margin must be >= 0, not {margin!r}')
    offsets = np.array([[m, 0.0], [-m, 0.0], [0.0, m], [0.0, -m]]) if m > 0 else np.zeros((1, 2))
    q = p[None, :, :] + offsets[:, None, :]                                   # (T, S, 2)
    a = fp                                                                     # (K, 4, 2): edge i goes a[i] -> a[i + 1]
    e = np.roll(fp, -1, axis=1) - fp
    # cross[k, i, t, s] of edge i of frame k with the point: one sign for all edges <=> strictly inside the convex quad
    with np.errstate(invalid='ignore'):
        cross = (e[:, :, None, None, 0] * (q[None, None, :, :, 1] - a[:, :, None, None, 1])
                 - e[:, :, None, None, 1] * (q[None, None, :, :, 0] - a[:, :, None, None, 0]))
        orientation = np.sign(np.sum(fp[:, :, 0] * np.roll(fp[:, :, 1], -1, axis=1)
                                     - np.roll(fp[:, :, 0], -1, axis=1) * fp[:, :, 1], axis=1))
        inside = (cross * orientation[:, None, None, None] > 0.0).all(axis=(1, 2))
    return inside


def frame_angles(results):
    """(K,) degrees: the rotation of every frame's transform, ``degrees(transform.rotation)``; NaN for a frame that failed.
    These are the ``angles_to_north`` of the ROI fit up to the constant that ``model_roi_cutouts`` subtracts (the first
    epoch's).  The sign follows the model as frozen in DESIGN.md section 3: a source at offset c from the stamp centre
    appears at R(alpha) c + (dx, dy) in an epoch, with R(alpha) = [[cos, -sin], [sin, cos]]; the transform takes c to
    s R(theta) c with the same matrix, hence alpha = +theta."""
    out = np.full(len(results), np.nan)
    for k, r in enumerate(results):
        m = _matrix_of(r)
        if m is not None:
            out[k] = math.degrees(math.atan2(m[1, 0], m[0, 0]))
    return out


def frame_scales(results):
    """(K,): the scale of every frame's transform (frame pixels per reference pixel); NaN for a frame that failed."""
    out = np.full(len(results), np.nan)
    for k, r in enumerate(results):
        m = _matrix_of(r)
        if m is not None:
            out[k] = math.hypot(m[0, 0], m[1, 0])
    return out
