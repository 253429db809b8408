"""The tests' own statement of where a PSF stamp of side P sits on the N x N grid of a joint fit,
written tap by tap and independently of lightcurver_amd.joint.place_psf: tap (a, b) goes to (a + c_N - c_P, b + c_N - c_P),
c_S = (S - 1) // 2 the zero lag of scipy.signal.fftconvolve(., ., 'same'); taps outside the grid are dropped."""
import numpy as np


def place(psf, N):
    """(E, P, P) -> (E, N, N), same dtype."""
    psf = np.asarray(psf)
    E, P, P2 = psf.shape
    assert P == P2
    shift = (N - 1) // 2 - (P - 1) // 2
    taps = np.array([a for a in range(P) if 0 <= a + shift < N], dtype=int)
    out = np.zeros((E, N, N), psf.dtype)
    for e in range(E):
        out[e][np.ix_(taps + shift, taps + shift)] = psf[e][np.ix_(taps, taps)]
    return out


def flux_outside(psf, N):
    """Largest fraction over the epochs of the stamps' flux that ``place`` drops."""
    psf = np.asarray(psf, dtype=np.float64)
    total = psf.reshape(psf.shape[0], -1).sum(axis=1)
    kept = place(psf, N).reshape(psf.shape[0], -1).sum(axis=1)
    return float(((total - kept) / total).max())
