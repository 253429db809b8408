"""The reference's ``estimate_seeing`` (lightcurver/processes/frame_characterization.py:135-202), restated: a seeing value
in pixels from the FWHM column of a table of sources.  Its result is the ``seeing_pixels`` that ``model_all_psfs`` hands
to ``build_psf`` as ``guess_fwhm_pixels``.  Host arithmetic over a few hundred numbers: no kernel."""
import numpy as np

MIN_FWHM, MAX_FWHM, BINS = 1.5, 30.0, 10


def estimate_seeing(sources_table):
    """More than 10 sources: the peak of a 10-bin histogram of the FWHMs between 1.5 and min(30, 3 median), refined by a
    second histogram of +-2 pixels around it, then the median of the FWHMs within 1 pixel of that peak (the peak itself if
    there are none; the plain median if the first peak is in an end bin).  1 - 10 sources: their median.  None: -1.0."""
    fwhms = np.asarray(sources_table['FWHM'], dtype=np.float64)
    if len(fwhms) > 10:
        med = max(float(np.median(fwhms)), MIN_FWHM)
        hist, edges = np.histogram(fwhms, bins=BINS, range=(MIN_FWHM, min(MAX_FWHM, 3.0 * med)))
        top = int(np.argmax(hist))
        if top == 0 or top == len(hist) - 1:
            return np.median(fwhms)
        peak = float(0.5 * (edges[top] + edges[top + 1]))
        hist, edges = np.histogram(fwhms, bins=BINS, range=(peak - 2.0, peak + 2.0))
        top = int(np.argmax(hist))
        peak = 0.5 * (edges[top] + edges[top + 1])
        near = fwhms[(fwhms > peak - 1.0) & (fwhms < peak + 1.0)]
        return np.median(near) if len(near) > 0 else peak
    if len(fwhms) > 0:
        return np.median(fwhms)
    return -1.0
