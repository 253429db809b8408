import numpy as np


def per_shape(fn, stamps, noisemaps):
    """Lists of stamps whose sizes may differ (the ROI and the stars of a frame) through a call that takes stacks:
    fn(stack_of_stamps, stack_of_noisemaps) is called once per stamp shape, in sorted order of the shapes, and returns
    one result per stamp of its stack; the results come back as a list in the order of ``stamps``."""
    stamps = [np.asarray(s, dtype=np.float32) for s in stamps]
    noisemaps = [np.asarray(m, dtype=np.float32) for m in noisemaps]
    if len(stamps) != len(noisemaps):
        raise ValueError('one noise map per stamp')
    out = [None] * len(stamps)
    for shape in sorted({s.shape for s in stamps}):
        idx = [i for i, s in enumerate(stamps) if s.shape == shape]
        results = fn(np.stack([stamps[i] for i in idx]), np.stack([noisemaps[i] for i in idx]))
        for i, r in zip(idx, results):
            out[i] = r
    return out
