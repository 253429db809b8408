"""The reference's ``subtract_background`` (lightcurver/processes/background_estimation.py:5-39, called once per frame at
frame_importation.py:81-91) on the device: the sky model of ``lightcurver_amd.sep.Background``, its subtraction and
``bkg.globalrms`` in one call per frame, or one call per frame shape for a whole list of frames.  The reference's two-pass
form (``mask_sources_first=True``: sky, sources of the subtracted frame, sky again without them) is
``subtract_background_masking_sources``."""
import numpy as np

from .. import sep

MASK_THRESH, MASK_MINAREA = 2, 10          # the reference's sep.extract of the source mask (background_estimation.py:32-33)


def _box_size(shape, n_boxes):
    box = int(min(shape[-2:])) // int(n_boxes)
    if box < 1:
        raise ValueError(f'n_boxes = {n_boxes} leaves no pixel per box in a frame of {tuple(shape[-2:])}')
    return box


def _stack(images, masks, n_boxes, ctx):
    """(subs (K, h, w) float32, [Background per frame]) of one stack."""
    box = _box_size(images.shape, n_boxes)
    r = sep.background_frames(images, masks, bw=box, bh=box, fw=3, fh=3, sub=True, back=False, ctx=ctx)
    shape = images.shape[-2:]
    return r['sub'], [sep.Background._from_result(r, shape, box, box, ctx, frame=k) for k in range(images.shape[0])]


def subtract_background(image, mask_sources_first=False, n_boxes=10, mask=None, ctx=None):
    """Subtracts the smooth sky of the 2-D ``image``: returns (image_sub float32, bkg) as the reference does, bkg being
    a ``sep.Background`` (``bkg.globalrms`` is the frame's background rms).  ``mask`` (non-zero = ignore) takes the place of
    the reference's second pass over a source mask."""
    if mask_sources_first:
        raise NotImplementedError('subtract_background: mask_sources_first=True needs a full-frame sep.extract, which is '
                                  'not built; pass the source mask as mask= instead')
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError(f'subtract_background takes one 2-D frame, got {image.shape}')
    subs, bkgs = _stack(image[None], None if mask is None else np.asarray(mask)[None], n_boxes, ctx)
    return subs[0], bkgs[0]


def subtract_background_batch(images, masks=None, n_boxes=10, ctx=None):
    """The same for many frames: a (K, h, w) stack is one device call; a list of frames of mixed shapes is one call per
    shape, in sorted order of the shapes.  Returns (list of image_sub, list of bkg) in the order of ``images``."""
    if isinstance(images, np.ndarray) and images.ndim == 3:          # a stack is one call as it is
        if masks is not None and len(masks) != len(images):
            raise ValueError('one mask per frame')
        subs, bkgs = _stack(images, None if masks is None else np.asarray(masks), n_boxes, ctx)
        return list(subs), bkgs
    frames = [np.asarray(f, dtype=np.float32) for f in images]
    if masks is not None and len(masks) != len(frames):
        raise ValueError('one mask per frame')
    subs, bkgs = [None] * len(frames), [None] * len(frames)
    for shape in sorted({f.shape for f in frames}):
        idx = [i for i, f in enumerate(frames) if f.shape == shape]
        m = None if masks is None else np.stack([np.asarray(masks[i]) for i in idx])
        s, b = _stack(np.stack([frames[i] for i in idx]), m, n_boxes, ctx)
        for i, si, bi in zip(idx, s, b):
            subs[i], bkgs[i] = si, bi
    return subs, bkgs


def subtract_background_masking_sources_batch(images, n_boxes=10, thresh=MASK_THRESH, minarea=MASK_MINAREA, ctx=None):
    """The reference's ``subtract_background(image, mask_sources_first=True)`` for a (K, h, w) stack: the sky, the
    sources of the subtracted frames above ``thresh`` sigma of the frame's ``globalrms`` (at least ``minarea`` pixels,
    ``sep.extract_frames``), and the sky again with those sources masked.  Returns (list of image_sub, list of bkg,
    masks uint8 (K, h, w))."""
    images = np.asarray(images)
    if images.ndim != 3:
        raise ValueError(f'expected a (K, h, w) stack of frames, got {images.shape}')
    box = _box_size(images.shape, n_boxes)
    first = sep.background_frames(images, None, bw=box, bh=box, fw=3, fh=3, sub=True, back=False, ctx=ctx)
    rms = first['globalrms'].astype(np.float32)
    found = sep.extract_frames(first['sub'], rms * rms, thresh, minarea, objects=False, mask=True, ctx=ctx)
    subs, bkgs = _stack(images, found['mask'], n_boxes, ctx)
    return list(subs), bkgs, found['mask']


def subtract_background_masking_sources(image, n_boxes=10, thresh=MASK_THRESH, minarea=MASK_MINAREA, ctx=None):
    """The same for one 2-D frame: returns (image_sub, bkg) as the reference does."""
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError(f'subtract_background_masking_sources takes one 2-D frame, got {image.shape}')
    subs, bkgs, _ = subtract_background_masking_sources_batch(image[None], n_boxes, thresh, minarea, ctx)
    return subs[0], bkgs[0]
