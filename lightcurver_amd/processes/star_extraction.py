"""The reference's ``extract_stars`` (lightcurver/processes/star_extraction.py:8-55, called once per imported frame at
frame_importation.py:130) over ``lightcurver_amd.sep.extract``: the catalogue of a background-subtracted frame as a table
with the reference's columns.  By default the extraction runs WITHOUT de-blending and cleaning (DESIGN.md §5 "Source
extraction of frames"): a blended pair is then one elongated object, which the elongation cut below mostly removes.
That default differs from the reference's call, which leaves sep's ``deblend_cont=0.005`` and ``clean=True`` in place;
``deblend=True`` is the reference's call (``sep.extract_deblended``, DESIGN.md §5 "De-blending and cleaning of frame
objects"), not pinned against sep itself."""
import numpy as np

from .. import sep

EXTRA_COLUMNS = ('xcentroid', 'ycentroid', 'elongation', 'FWHM', 'ellipticity')
TABLE_DTYPE = np.dtype(sep.OBJECT_DTYPE.descr + [(n, '<f8') for n in EXTRA_COLUMNS])


def sources_table_from_objects(objects):
    """The reference's table from the structured array of ``sep.extract``, as a structured array (``table['FWHM']``
    works as on the reference's astropy Table): xcentroid, ycentroid, elongation = a / b, the cut elongation < median + 3
    std over the whole catalogue, FWHM = 2 sqrt(ln 2 (a^2 + b^2)), ellipticity = 1 - b / a, brightest first.  Rows whose
    moments are NaN (flags LARGE or RANGE) fail the cut; NaN does not enter the median and the std.  An empty catalogue
    gives an empty table with all columns."""
    objects = np.asarray(objects)
    out = np.zeros(len(objects), TABLE_DTYPE)
    for n in objects.dtype.names:
        if n in out.dtype.names:
            out[n] = objects[n]
    if not len(out):
        return out
    out['xcentroid'], out['ycentroid'] = out['x'], out['y']
    elongation = out['a'] / out['b']
    out['elongation'] = elongation
    measured = elongation[np.isfinite(elongation)]
    if not measured.size:
        return out[:0]
    with np.errstate(invalid='ignore'):
        out = out[elongation < np.median(measured) + 3 * np.std(measured)]
    out['FWHM'] = 2 * (np.log(2) * (out['a'] ** 2 + out['b'] ** 2)) ** 0.5
    out['ellipticity'] = 1 - out['b'] / out['a']
    return out[np.argsort(-out['flux'], kind='stable')]


def extract_stars(image_background_subtracted, variance_map, detection_threshold=3, min_area=10, ctx=None, deblend=False):
    """The sources of a background-subtracted frame: ``variance_map`` a map or a scalar variance, the threshold in
    sigma, the least number of pixels of a detection.  ``deblend=True``: with sep's de-blending and cleaning, as the
    reference calls it.  Returns ``sources_table_from_objects`` of the catalogue."""
    extract = sep.extract_deblended if deblend else sep.extract
    objects = extract(image_background_subtracted, detection_threshold, var=variance_map, minarea=min_area, ctx=ctx)
    return sources_table_from_objects(objects)
