"""Inputs of the frame form of the cosmic-ray kernels (lc_detect_cosmics_frames, lc_frames_detect_cosmics), shared by
tests/test_cosmics_frames_cpu.py, which holds every input to the property it is built for, and
tests/test_cosmics_frames_gpu.py.  The yardstick is always ``tests/_lacosmic.py::lacosmic`` in float32 on the whole
frame; its results are computed once per input and shared."""
import numpy as np

from tests import _lacosmic as LA

READNOISE = 6.5
SHAPES = ((8, 8), (8, 9), (9, 40), (13, 200), (40, 56), (65, 127), (130, 67), (200, 261))


def sky(shape, seed):
    """Poisson sky of 200 counts plus read noise, float32."""
    rng = np.random.default_rng(seed)
    return (rng.poisson(200.0, shape) + rng.normal(0.0, READNOISE, shape)).astype(np.float32)


def model_invar(d):
    return (np.maximum(d, 0) + np.float32(READNOISE) ** 2).astype(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, keys=('crmask', 'clean', 'iters')):
    """The keys on which the device result differs from the restatement's, bit for bit (NaN-safe)."""
    return [k for k in keys if not np.array_equal(bits(np.asarray(got[k])), bits(np.asarray(want[k])))]


def plain_input(shape, K=2):
    """K frames of sky, one hit of + 3000 on the first: (data, (y, x) of the hit)."""
    h, w = shape
    d = sky((K, h, w), 100 * h + w)
    y, x = h // 2, (2 * w) // 3
    d[0, y, x] += 3000.0
    return d, (y, x)


def fallback_input(shape):
    """One frame whose pixel (cy, cx) is hit by + 5000 and whose 5 x 5 window is masked around it: the cleaning finds no
    good neighbour and takes the lower median of the frame's good pixels.  Returns (data, inmask, (cy, cx))."""
    h, w = shape
    d = sky((1, h, w), 7 * h + w)
    cy, cx = h // 2, w // 2
    inmask = np.zeros(d.shape, bool)
    inmask[0, cy - 2:cy + 3, cx - 2:cx + 3] = True
    inmask[0, cy, cx] = False
    d[0, cy, cx] += 5000.0
    return d, inmask, (cy, cx)


def all_but(shape, cy, cx):
    """inmask of one frame with every pixel masked but (cy, cx)."""
    m = np.ones(shape, bool)
    m[0, cy, cx] = False
    return m


EARLY_EXIT_SHAPE = (130, 67)


def early_exit_input():
    """Three frames that stop at different iterations: plain sky, one pixel + 4000, a 9 x 9 block + 6000 that the
    iterations peel ring by ring."""
    h, w = EARLY_EXIT_SHAPE
    d = sky((3, h, w), 5)
    d[1, 40, 30] += 4000.0
    d[2, 60:69, 20:29] += 6000.0
    return d


STRADDLE_SHAPE = (200, 261)


def straddle_hits():
    """(y, x) of the 55 hits: every interior multiple of 16 with (y // 16 + x // 16) % 3 == 0.  A hit covers the rows
    y - 1, y and the columns x - 1, x, so it crosses the lines y and x: between them the hits cross every multiple of
    16, 32, 48 and 64 in both directions, whatever tile size a kernel uses."""
    h, w = STRADDLE_SHAPE
    return [(y, x) for y in range(16, h - 16, 16) for x in range(16, w - 16, 16) if (y // 16 + x // 16) % 3 == 0]


def straddle_input():
    """(data (2, 200, 261), bool mask of the hit pixels): the hits on frame 0, frame 1 plain sky."""
    h, w = STRADDLE_SHAPE
    d = sky((2, h, w), 4)
    hit = np.zeros(d.shape, bool)
    for y, x in straddle_hits():
        hit[0, y - 1:y + 1, x - 1:x + 1] = True
    d[hit] += 2500.0
    return d, hit


def saturated_input():
    """(65, 127) with a saturated 4 x 6 core of 70000: grown twice, 8 x 10 = 80 pixels are masked, nothing is flagged."""
    d = sky((1, 65, 127), 13)
    d[0, 30:34, 60:66] = 70000.0
    return d


def nan_columns_input():
    """(65, 127) with five NaN columns at the left edge and one hit."""
    d = sky((1, 65, 127), 17)
    d[0, :, :5] = np.nan
    d[0, 20, 50] += 3000.0
    return d


def stars_input():
    """(65, 127) sky with five narrow Gaussian stars (sigma 0.9 pixels, peak 3000): the fine-structure ratio of their
    cores lies between 1 and 5, so objlim = 1 flags what the default 5 leaves alone."""
    d = sky((1, 65, 127), 19)
    yy, xx = np.mgrid[0:65, 0:127]
    for cy, cx in ((10.3, 12.6), (30.0, 47.5), (33.4, 100.2), (50.7, 70.1), (58.2, 120.4)):
        d[0] += (3000.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 0.9 ** 2))).astype(np.float32)
    return d


# The settings other than the defaults: (setting, with invar) -> the input it runs on, by the rule of the settings table of
# tests/_lacosmic.py: a case runs only where the restatement's result differs from the one at the defaults on the same
# input, which tests/test_cosmics_frames_cpu.py asserts for every entry.  On the straddling input objlim = 1 changes
# nothing (a sharp hit has a large ratio anyway) and is run on the stars instead; readnoise enters with invar through the
# invalid pixels alone, of which that input has none (None: the case is not run).
SETTINGS = (dict(sigclip=2.0), dict(sigfrac=0.0), dict(objlim=1.0), dict(niter=1), dict(gain=0.37), dict(readnoise=0.0))
SETTINGS_INPUT = {('sigclip', False): 'straddle', ('sigclip', True): 'straddle', ('sigfrac', False): 'straddle',
                  ('sigfrac', True): 'straddle', ('objlim', False): 'stars', ('objlim', True): 'stars',
                  ('niter', False): 'straddle', ('niter', True): 'straddle', ('gain', False): 'straddle',
                  ('gain', True): 'straddle', ('readnoise', False): 'straddle', ('readnoise', True): None}


def settings_data(name):
    return straddle_input()[0] if name == 'straddle' else stars_input()


def settings_cases():
    """[(label, data, keyword arguments of the case, of its base)] of every case that runs."""
    out = []
    for s in SETTINGS:
        (name, value), = s.items()
        for inv in (False, True):
            where = SETTINGS_INPUT[name, inv]
            if where is None:
                continue
            d = settings_data(where)
            base = dict(invar=model_invar(d)) if inv else {}
            out.append((f'{name} {value:g} {"invar" if inv else "model"} {where}', d, dict(base, **s), base))
    return out


_wanted = {}


def wanted(data, **kw):
    """The restatement's float32 result on the whole frames, computed once per input and settings."""
    key = (data.tobytes(), repr(sorted((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in kw.items())))
    if key not in _wanted:
        _wanted[key] = LA.lacosmic(data, sepmed=True, dtype=np.float32, **kw)
    return _wanted[key]
