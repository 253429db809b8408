"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the SPEC of DESIGN.md section 5 "Stamp cutting": where Cutout2D puts a
stamp, the cut with NaN outside the frame, and the noise map in the float32 steps of the device (prep_pixel's order).
PARITY UNPINNED against astropy, which is not installed here: the arithmetic is restated from its documentation."""
import math

import numpy as np

F32 = np.float32


def cutout_origin(position_xy, size, frame_shape):
    """One position (x, y) -> ((x0, y0), (cx, cy)): plain Python floats, one stamp at a time."""
    x, y = (float(v) for v in position_xy)
    n = int(size)
    h, w = frame_shape
    if not (math.isfinite(x) and math.isfinite(y)):
        raise ValueError('position not finite')
    x0, y0 = int(math.ceil(x - n / 2)), int(math.ceil(y - n / 2))
    if x0 + n <= 0 or x0 >= w or y0 + n <= 0 or y0 >= h:
        raise ValueError('no overlap')
    xs, xe, ys, ye = max(0, x0), min(w, x0 + n), max(0, y0), min(h, y0 + n)
    return (x0, y0), (0.5 * (xs + xe - 1), 0.5 * (ys + ye - 1))


def cut(frames, frame_index, x0, y0, n):
    """(data (S, n, n) float32 with NaN outside the frame, n_inside (S,)): slices of a NaN-padded copy."""
    frames = np.asarray(frames, F32)
    K, h, w = frames.shape
    padded = np.full((K, h + 2 * n, w + 2 * n), np.nan, F32)
    padded[:, n:n + h, n:n + w] = frames
    out = np.empty((len(x0), n, n), F32)
    inside = np.empty(len(x0), np.int64)
    for s, (k, xa, ya) in enumerate(zip(frame_index, x0, y0)):
        assert -n < xa < w and -n < ya < h
        out[s] = padded[k, ya + n:ya + 2 * n, xa + n:xa + 2 * n]
        inside[s] = (min(w, xa + n) - max(0, xa)) * (min(h, ya + n) - max(0, ya))
    return out, inside


def noisemap(data, rms, exptime):
    """data (S, n, n) float32, rms and exptime (S,): every step rounded to float32, in the order of the device."""
    d = np.asarray(data, F32)
    t = np.asarray(exptime, F32).reshape(-1, 1, 1)
    r = np.asarray(rms, F32).reshape(-1, 1, 1)
    with np.errstate(invalid='ignore'):
        e = d * t
        trms = t * r
        trms2 = trms * trms
        s = np.maximum(np.sqrt(trms2 + np.abs(e)), F32(1e-7)) / t
    s = np.where(np.isnan(e), e, s)          # np.maximum already keeps the NaN; the device says it outright
    assert s.dtype == F32
    return s


def close(a, b, tol):
    """The bound of tests/test_prep_gpu.py: same NaN pattern, |a - b| <= tol * max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(b)
    assert np.abs(a[m] - b[m]).max() <= tol * max(np.abs(b[m]).max(), 1e-300)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cut_stamps(frames, frame_index, positions_xy, size, exptimes, background_rms):
    """What FrameSet.cut_stamps returns with both mask switches off, from the restatement."""
    frames = np.asarray(frames, F32)
    K, h, w = frames.shape
    pos = np.asarray(positions_xy, np.float64).reshape(-1, 2)
    S = len(pos)
    index = np.broadcast_to(np.asarray(frame_index).reshape(-1), (S,))
    both = [cutout_origin(p, size, (h, w)) for p in pos]
    origin = np.array([o for o, _ in both], np.int64)
    centre = np.array([c for _, c in both], np.float64)
    data, inside = cut(frames, index, origin[:, 0], origin[:, 1], int(size))
    t = np.broadcast_to(np.asarray(exptimes, F32).reshape(-1), (K,))[index]
    r = np.broadcast_to(np.asarray(background_rms, F32).reshape(-1), (K,))[index]
    return dict(data=data, noisemap=noisemap(data, r, t), mask=np.zeros(data.shape, bool), origin=origin,
                center_original=centre, n_inside=inside, kernel_ms=0.0)
