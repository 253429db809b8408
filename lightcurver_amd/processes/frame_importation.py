"""The arithmetic of the reference's frame importation (lightcurver/processes/frame_importation.py:81-141) with the frame
uploaded once (``lc_import_frames``): sky, optionally the source mask and the sky again, the variance map, the catalogue,
then on the host the sources table, the seeing and the ellipticity.  Frames are in electrons per second."""
import ctypes as C

import numpy as np

from .. import _lib, sep
from .._lib import f32, ptr
from .background_estimation import MASK_MINAREA, MASK_THRESH, _box_size
from .frame_characterization import estimate_seeing
from .star_extraction import sources_table_from_objects

_i32p = C.POINTER(C.c_int32)


def import_frames(stack, exptimes, n_boxes=10, mask_sources_first=False, detection_threshold=3, min_area=10,
                  max_objects=8192, segmentation_map=False, ctx=None, deblend=False):
    """One ``lc_import_frames`` call over a (K, h, w) stack; with ``deblend`` (True: sep's defaults, the reference's
    call; or a dict as ``sep.extract_frames`` takes) one ``lc_import_frames_deblended`` call.  Returns dict(sub (K, h, w), mesh_back, mesh_rms, globalback,
    globalrms, status (the background's), objects: list of K record arrays, nobj, ex_status, segmap (if asked), box,
    kernel_ms).  A frame with more than ``max_objects`` objects makes the call run once more with the largest count."""
    d = f32(stack)
    if d.ndim != 3:
        raise ValueError(f'expected a (K, h, w) stack of frames, got {d.shape}')
    K, h, w = d.shape

    name = 'lc_import_frames_deblended' if sep.deblend_cfg(deblend) is not None else 'lc_import_frames'

    def call(*args):
        c = ctx or _lib.default_context()
        c.check(getattr(_lib.lib(), name)(c.h, K, h, w, ptr(d), *args), name)

    return _import(call, d.shape, exptimes, n_boxes, mask_sources_first, detection_threshold, min_area, max_objects,
                   segmentation_map, True, deblend)


def _import(call, shape, exptimes, n_boxes, mask_sources_first, detection_threshold, min_area, max_objects,
            segmentation_map, with_sub, deblend=False):
    """The settings, the outputs and the second run on a full object table, shared by ``import_frames`` and
    ``FrameSet.import_frames``: ``call`` takes the arguments of ``lc_import_frames`` from ``exptime`` on, or with
    ``deblend`` those of ``lc_import_frames_deblended``."""
    K, h, w = shape
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(exptimes, np.float32).reshape(-1), (K,)), dtype=np.float32)
    if not (np.isfinite(t) & (t > 0)).all():
        raise ValueError('exposure times must be finite and > 0')
    box = _box_size(shape, n_boxes)
    sep._refuse(shape, box, box, 3, 3, 0.0)
    if not sep.extract_supported(h, w):
        raise NotImplementedError(f'import_frames: {h} x {w} pixels is 2^31 or more')
    bcfg = _lib.BackgroundCfg(box, box, 3, 3, 0.0)
    ecfg = sep.extract_cfg(detection_threshold, min_area)
    mcfg = sep.extract_cfg(MASK_THRESH, MASK_MINAREA)
    dcfg = sep.deblend_cfg(deblend)
    catalogue = (C.byref(ecfg),) if dcfg is None else (C.byref(ecfg), C.byref(dcfg))
    ny, nx = sep.mesh_shape(h, w, box, box)
    out = dict(sub=np.empty(shape, np.float32) if with_sub else None, mesh_back=np.empty((K, ny, nx), np.float32),
               mesh_rms=np.empty((K, ny, nx), np.float32), globalback=np.empty(K, np.float32),
               globalrms=np.empty(K, np.float32), status=np.zeros(K, np.int32), nobj=np.zeros(K, np.int32),
               ex_status=np.zeros(K, np.int32), segmap=np.zeros(shape, np.int32) if segmentation_map else None,
               objects=[], box=box, kernel_ms=0.0)
    if not K:
        return out
    cap = int(max_objects)
    for attempt in range(2):
        table = np.zeros((K, cap), _lib.EXTRACT_OBJECT_DTYPE)
        ms = C.c_float()
        call(ptr(t), C.byref(bcfg), *catalogue, int(bool(mask_sources_first)), C.byref(mcfg), cap,
             ptr(out['sub']), ptr(out['mesh_back']), ptr(out['mesh_rms']), ptr(out['globalback']), ptr(out['globalrms']),
             out['status'].ctypes.data_as(_i32p), table.ctypes.data_as(C.c_void_p), out['nobj'].ctypes.data_as(_i32p),
             out['segmap'].ctypes.data_as(_i32p) if segmentation_map else None, out['ex_status'].ctypes.data_as(_i32p),
             C.byref(ms))
        out['kernel_ms'] += ms.value
        if not (out['ex_status'] == 1).any():
            break
        cap = int(out['nobj'].max())
    out['objects'] = [table[k, :min(int(out['nobj'][k]), cap)].copy() for k in range(K)]
    return out


def _characterize_stack(stack, exptimes, n_boxes, mask_sources_first, detection_threshold, min_area, ctx, deblend=False):
    r = import_frames(stack, exptimes, n_boxes, mask_sources_first, detection_threshold, min_area, ctx=ctx, deblend=deblend)
    out = []
    for k in range(stack.shape[0]):
        if int(r['ex_status'][k]) == 2:
            raise _lib.LcError(f'frame {k}: the iteration guard of the labelling was reached')
        sources = sources_table_from_objects(sep.objects_view(r['objects'][k]))
        with np.errstate(all='ignore'):
            ellipticity = float(np.nanmedian(sources['ellipticity'])) if len(sources) else float('nan')
        out.append(dict(image_sub=r['sub'][k],
                        bkg=sep.Background._from_result(r, stack.shape[-2:], r['box'], r['box'], ctx, frame=k),
                        sources_table=sources, seeing_pixels=float(estimate_seeing(sources)), ellipticity=ellipticity,
                        kernel_ms=r['kernel_ms']))
    return out


def characterize_frames(frames, exptimes, n_boxes=10, mask_sources_first=False, detection_threshold=3, min_area=10, ctx=None,
                        deblend=False):
    """What the reference computes of every frame it imports, for a (K, h, w) stack (one device call) or a list of frames
    of mixed shapes (one call per shape, in sorted order of the shapes).  ``exptimes``: one per frame, or one for all.
    Returns one dict per frame, in the order of ``frames``: image_sub, bkg (a ``sep.Background``), sources_table,
    seeing_pixels (-1.0 without sources), ellipticity (the nanmedian of the table's; NaN without sources).  ``deblend``:
    False for the catalogue without de-blending and cleaning, True for the reference's call (sep's defaults)."""
    if isinstance(frames, np.ndarray) and frames.ndim == 3:
        t = np.broadcast_to(np.asarray(exptimes, np.float32).reshape(-1), (len(frames),))
        return _characterize_stack(frames, t, n_boxes, mask_sources_first, detection_threshold, min_area, ctx, deblend)
    frames = [np.asarray(f, dtype=np.float32) for f in frames]
    if any(f.ndim != 2 for f in frames):
        raise ValueError('characterize_frames takes 2-D frames')
    t = np.broadcast_to(np.asarray(exptimes, np.float32).reshape(-1), (len(frames),))
    out = [None] * len(frames)
    for shape in sorted({f.shape for f in frames}):
        idx = [i for i, f in enumerate(frames) if f.shape == shape]
        res = _characterize_stack(np.stack([frames[i] for i in idx]), t[idx], n_boxes, mask_sources_first,
                                  detection_threshold, min_area, ctx, deblend)
        for i, r in zip(idx, res):
            out[i] = r
    return out
