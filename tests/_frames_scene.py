"""The scene of tests/test_pipeline_gpu.py: eight frames of 160 x 128 pixels of one field with ten stars and a blend of two
point sources, made by ``lightcurver_amd.synthetic.make_frames`` (which asserts what the tests rely on).  Host only."""
import numpy as np

SHAPE = (160, 128)                       # (h, w): not square, so that a swap of x and y cannot pass
SS, N_STARS, N_ROI = 2, 16, 16           # subsampling, star stamps, ROI stamps
MARGIN = N_STARS / 2.0                   # the driver's default footprint margin: half the star stamp
NOMINAL_EXPOSURE = 60.0
ROI = np.array([70.3, 84.6])
POINT_SOURCES = ROI + np.array([[-1.4, -1.05], [1.4, 1.05]])          # 3.5 pixels apart
# ten stars at asymmetric positions, >= 24 px from one another and from the ROI; the seventh lies 12 px from the right edge
STARS = np.array([[20.4, 22.7], [47.8, 30.2], [16.9, 56.3], [44.1, 68.9], [22.6, 101.4], [46.3, 124.8], [115.0, 40.3],
                  [96.7, 57.1], [99.2, 118.6], [73.5, 141.9]])
EDGE_STAR = 6
STAR_ELECTRONS = np.array([2.0e4, 1.6e5, 4.5e4, 2.0e5, 3.0e4, 9.0e4, 6.0e4, 1.2e5, 2.6e4, 7.5e4])   # in the nominal exposure
ROTATIONS = np.array([0.0, 0.0, 1.5, -2.0, 8.0, -12.0, 0.0, 0.0])
SHIFTS = np.array([[0.0, 0.0], [2.37, -4.21], [4.8, 1.58], [3.25, 2.83], [1.5, -3.46], [-3.6, 4.07], [0.0, 0.0], [70.0, 0.0]])
SEEING = np.array([3.0, 3.4, 2.8, 3.6, 3.2, 2.9, 3.1, 3.3])
T = np.array([1.0, 0.7, 1.3, 0.85, 1.15, 0.6, 1.0, 0.9])             # transparency, as tests/test_calibration_gpu.py's T
EXPTIMES = np.array([60.0, 45.0, 90.0, 60.0, 75.0, 50.0, 60.0, 60.0])
SKY = np.array([12.0, 15.0, 9.0, 20.0, 14.0, 11.0, 13.0, 16.0])
GOOD, BLANK, SHIFTED = (0, 1, 2, 3, 4, 5), 6, 7
K = len(T)


def roi_fluxes(frames=K):
    """(frames, 2) electrons per second at transparency 1: source A varies by +-25 % over the epochs, B is constant."""
    e = np.arange(frames)
    a = 9.0e4 / NOMINAL_EXPOSURE * (1.0 + 0.25 * np.sin(2.0 * np.pi * e / 6.0 + 0.7))
    return np.stack([a, np.full(frames, 6.0e4 / NOMINAL_EXPOSURE)], axis=1)


_scene = {}


def scene():
    """make_frames of the scene, once."""
    if not _scene:
        from lightcurver_amd.synthetic import make_frames
        assert np.sqrt(((STARS[:, None] - STARS[None]) ** 2).sum(-1))[~np.eye(len(STARS), dtype=bool)].min() >= 24.0
        assert np.sqrt(((STARS - ROI) ** 2).sum(-1)).min() >= 24.0
        assert np.diff(np.sort(np.sqrt(((STARS - ROI) ** 2).sum(-1)))).min() > 1.0      # the order by distance is robust
        assert SHAPE[1] - 1 - STARS[EDGE_STAR, 0] == 12.0
        _scene.update(make_frames(SHAPE, STARS, STAR_ELECTRONS / NOMINAL_EXPOSURE, POINT_SOURCES, roi_fluxes(), ROTATIONS, SHIFTS,
                                  SEEING, T, SKY, EXPTIMES, ss=SS, psf_size=N_STARS, blank_frames=(BLANK,), seed=77,
                                  good_frames=GOOD, footprint_margin=MARGIN))
    return _scene


def two_good_frames():
    """Frames 0 and 1 and the blank one: a set of which two frames can survive."""
    s = scene()
    index = [0, 1, BLANK]
    return s['frames'][index], s['exptimes'][index]
