"""A set of frames that stays on the device (``lc_frames``): uploaded once, imported where it lies, and the stamps of the
ROI and of the stars cut from it later, once the caller has solved the astrometry.

The reference imports a frame, writes the sky-subtracted frame to disk (lightcurver/processes/frame_importation.py:119)
and cuts every stamp from it on the host, one ``Cutout2D`` at a time (cutout_making.py:23-51, from :188 and :238).  Here
``FrameSet.import_frames`` is ``processes.frame_importation.import_frames`` on the resident planes, after which they hold
the sky-subtracted frames, and ``FrameSet.cut_stamps`` cuts every stamp of one size, forms its noise map and masks it in
one call (``lc_frames_cut_stamps``; DESIGN.md section 5 "Stamp cutting").  WCS and sky coordinates stay with the caller:
positions are pixel positions as ``skycoord_to_pixel`` gives them, 0-based with the pixel centres at integers."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import f32, ptr

_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)


def _per_frame(values, K):
    """One float32 per frame of the set from one value or K of them; None stays None."""
    if values is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(values, np.float32).reshape(-1), (K,)), dtype=np.float32)


class FrameSet:
    """K frames of one shape on the device.  ``stack``: (K, h, w), in electrons per second.  Raises without a device:
    there is no CPU fallback."""

    def __init__(self, stack, ctx=None):
        d = f32(stack)
        if d.ndim != 3 or 0 in d.shape:
            raise ValueError(f'expected a (K, h, w) stack of frames, got {d.shape}')
        self.ctx = ctx or _lib.default_context()
        self._l = _lib.lib()
        self.shape = d.shape
        h = _lib.vp()
        K, hh, ww = d.shape
        self.ctx.check(self._l.lc_frames_create(self.ctx.h, K, hh, ww, ptr(d), C.byref(h)), 'lc_frames_create')
        self.h = h

    def __len__(self):
        return self.shape[0]

    @property
    def frame_shape(self):
        return self.shape[1:]

    @property
    def imported(self):
        flag = C.c_int()
        self.ctx.check(self._l.lc_frames_info(self._handle(), None, None, None, C.byref(flag)), 'lc_frames_info')
        return bool(flag.value)

    def _handle(self):
        if not getattr(self, 'h', None):
            raise _lib.LcError('the frame set has been closed')
        return self.h

    def import_frames(self, exptimes, n_boxes=10, mask_sources_first=False, detection_threshold=3, min_area=10,
                      max_objects=8192, download_sub=False, deblend=False):
        """``processes.frame_importation.import_frames`` on the resident planes, which hold ``sub`` afterwards; the same
        dict, with ``sub`` None unless ``download_sub``.  ``deblend``: as there (``lc_frames_import_deblended``).  Exposure times and background rms stay recorded for
        ``cut_stamps``.  A set is imported once: a second call raises."""
        from . import sep
        from .processes.frame_importation import _import
        handle = self._handle()
        name = 'lc_frames_import_deblended' if sep.deblend_cfg(deblend) is not None else 'lc_frames_import'

        def call(*args):
            self.ctx.check(getattr(self._l, name)(handle, *args), name)

        out = _import(call, self.shape, exptimes, n_boxes, mask_sources_first, detection_threshold, min_area,
                      max_objects, False, bool(download_sub), deblend)
        if self.imported:
            self._globalrms = np.array(out['globalrms'], np.float32)      # what ``coadd`` weighs the frames with
        if not download_sub:
            del out['sub']
        return out

    def planes(self, first=0, count=None):
        """The resident planes [first, first + count) as they are now: the frames as uploaded, or ``sub`` after the
        import."""
        K = self.shape[0]
        first = int(first)
        count = K - first if count is None else int(count)
        out = np.empty((max(count, 0),) + self.shape[1:], np.float32)
        self.ctx.check(self._l.lc_frames_get(self._handle(), first, count, ptr(out)), 'lc_frames_get')
        return out

    def cut_stamps(self, frame_index, positions_xy, size, exptimes=None, background_rms=None, do_mask_bad_columns=False,
                   do_mask_cosmics=False, cosmics_masking_params=None):
        """S stamps of ``size`` x ``size`` in one device call.  frame_index: (S,) or one frame for all; positions_xy:
        (S, 2) pixel positions (x, y).  exptimes, background_rms: one per frame of the set, or one for all; after
        ``import_frames`` both default to the recorded values.  Returns dict(data, noisemap (S, n, n) float32 with NaN
        outside the frame, mask (S, n, n) bool as ``mask_cutout_batch`` gives it, origin (S, 2) int (x0, y0),
        center_original (S, 2) float64 (x, y) of the part inside the frame, n_inside (S,), kernel_ms)."""
        from .processes.cutout_making import _mask_settings, cutout_origin
        handle = self._handle()
        K, h, w = self.shape
        n = int(size)
        pos = np.asarray(positions_xy, np.float64).reshape(-1, 2)
        S = len(pos)
        if S < 1:
            raise ValueError('cut_stamps: no position')
        frame = np.ascontiguousarray(np.broadcast_to(np.asarray(frame_index, np.int32).reshape(-1), (S,)), dtype=np.int32)
        if ((frame < 0) | (frame >= K)).any():
            raise ValueError(f'cut_stamps: a frame index outside 0 .. {K - 1}')
        origin, centre = cutout_origin(pos, n, (h, w))
        x0 = np.ascontiguousarray(origin[:, 0], dtype=np.int32)
        y0 = np.ascontiguousarray(origin[:, 1], dtype=np.int32)
        masks = bool(do_mask_bad_columns or do_mask_cosmics)
        if not self._l.lc_cutout_supported(n, int(masks)) or S * n * n >= 2 ** 31:
            raise _lib.LcError(f'lc_frames_cut_stamps takes stamps of 8 .. 128 pixels with masks, any size with '
                               f'S n n < 2^31 without, not {S} of {n}')
        ccfg, bcfg = _mask_settings(dict(cosmics_masking_params or {}))
        t, rms = _per_frame(exptimes, K), _per_frame(background_rms, K)
        if t is not None and not (np.isfinite(t) & (t > 0)).all():
            raise ValueError('exposure times must be finite and > 0')
        data = np.empty((S, n, n), np.float32)
        noise = np.empty((S, n, n), np.float32)
        mask = np.zeros((S, n, n), np.uint8)
        inside = np.zeros(S, np.int32)
        ms = C.c_float()
        self.ctx.check(self._l.lc_frames_cut_stamps(
            handle, S, n, frame.ctypes.data_as(_i32p), y0.ctypes.data_as(_i32p), x0.ctypes.data_as(_i32p), ptr(t), ptr(rms),
            int(bool(do_mask_bad_columns)), int(bool(do_mask_cosmics)), C.byref(ccfg), C.byref(bcfg), ptr(data), ptr(noise),
            mask.ctypes.data_as(_u8p), inside.ctypes.data_as(_i32p), C.byref(ms)), 'lc_frames_cut_stamps')
        return dict(data=data, noisemap=noise, mask=mask.astype(bool), origin=origin, center_original=centre,
                    n_inside=inside, kernel_ms=ms.value)

    def aperture_photometry(self, frame_index, positions_xy, r, with_error=False, exptimes=None, background_rms=None):
        """P exact circular-aperture sums on the resident planes in one device call (``lc_frames_aperture_sums``; DESIGN.md
        section 5 "Aperture sums").  frame_index: (P,) or one frame for all; positions_xy: (P, 2) pixel positions (x, y);
        r: (P,) or one radius for all.  ``with_error``: the per-pixel error is the noise map ``cut_stamps`` would form,
        from exptimes and background_rms (one per frame of the set, or one for all; after ``import_frames`` both default
        to the recorded values).  Returns the dict of ``photutils.aperture_sums_batch``: sum, sum_err (None without
        ``with_error``), area, bad_area float64 (P,), kernel_ms."""
        from .photutils import _aperture_list
        handle = self._handle()
        K = self.shape[0]
        frame, xy, rr = _aperture_list(K, frame_index, positions_xy, r)
        P = len(xy)
        out = dict(sum=np.zeros(P), sum_err=np.zeros(P) if with_error else None, area=np.zeros(P), bad_area=np.zeros(P),
                   kernel_ms=0.0)
        if not P:
            return out
        t, rms = _per_frame(exptimes, K), _per_frame(background_rms, K)
        if t is not None and not (np.isfinite(t) & (t > 0)).all():
            raise ValueError('exposure times must be finite and > 0')
        dptr = lambda a: None if a is None else a.ctypes.data_as(_lib.dp)
        ms = C.c_float()
        self.ctx.check(self._l.lc_frames_aperture_sums(
            handle, P, frame.ctypes.data_as(_i32p), dptr(xy), dptr(rr), ptr(t), ptr(rms), int(bool(with_error)),
            dptr(out['sum']), dptr(out['sum_err']), dptr(out['area']), dptr(out['bad_area']), C.byref(ms)),
            'lc_frames_aperture_sums')
        out['kernel_ms'] = ms.value
        return out

    def coadd(self, frame_index, transforms, shape=None, origin=(0, 0), flux_scale=None, weights=None, order=3,
              combine='sigma_clip', n_sigma=3.0, scratch_rows=0):
        """The frames ``frame_index`` (any order, repeated at will) resampled onto one grid of reference pixels and
        combined per pixel, in one device call (``lc_frames_coadd``; DESIGN.md section 5 "Co-addition of frames").
        transforms: per frame a ``SimilarityTransform`` as ``register_frames`` gives it, a (2, 3) or a (3, 3) array: it
        maps reference pixels (x, y) to the frame's.  shape (H, W) and origin (x0, y0): the grid, by default the frame's
        own.  flux_scale: per frame, the sample is multiplied by it and by |det| of the transform (default 1).  weights:
        per frame, >= 0; by default, after ``import_frames``, 1 / (s rms)^2 with s the factor above and rms the recorded
        ``globalrms``, otherwise 1.  order 1 (bilinear) or 3 (Keys' cubic convolution); combine 'mean', 'median' or
        'sigma_clip' at ``n_sigma``.  ``scratch_rows``: output rows resampled per strip (0: from a budget); the result
        does not depend on it.  Returns dict(image float32 (H, W), NaN where no frame has a sample; weight float32, the sum
        of the weights of the kept samples; count, n_rejected int32; kernel_ms).  The planes stay as they are."""
        handle = self._handle()
        K, h, w = self.shape
        frame = np.ascontiguousarray(np.asarray(frame_index, np.int32).reshape(-1))
        n = len(frame)
        if n < 1:
            raise ValueError('coadd: no frame')
        if ((frame < 0) | (frame >= K)).any():
            raise ValueError(f'coadd: a frame index outside 0 .. {K - 1}')
        if hasattr(transforms, 'params') or (isinstance(transforms, np.ndarray) and transforms.ndim == 2):
            transforms = [transforms]
        if len(transforms) != n:
            raise ValueError(f'coadd: {n} frames but {len(transforms)} transforms')
        affine = np.empty((n, 6), np.float64)
        for k, t in enumerate(transforms):
            m = np.asarray(t.params if hasattr(t, 'params') else t, np.float64)
            if m.shape not in ((2, 3), (3, 3)):
                raise ValueError(f'coadd: a transform of shape {m.shape}, not (2, 3) or (3, 3)')
            affine[k] = m[:2].reshape(6)
        if combine not in _lib.COADD_COMBINE:
            raise ValueError(f'coadd: combine must be one of {tuple(_lib.COADD_COMBINE)}, not {combine!r}')
        H, W = (h, w) if shape is None else (int(shape[0]), int(shape[1]))
        x0, y0 = int(origin[0]), int(origin[1])
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f'coadd: a grid of {H} x {W} pixels')
        per_slot = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32).reshape(-1), (n,)), np.float32)
        g = None if flux_scale is None else per_slot(flux_scale)
        if weights is None and self.imported:
            rms = self._globalrms[frame].astype(np.float64)
            det = np.abs(affine[:, 0] * affine[:, 4] - affine[:, 1] * affine[:, 3])
            s = (1.0 if g is None else g.astype(np.float64)) * det
            with np.errstate(all='ignore'):
                weights = 1.0 / (s * rms) ** 2
        wt = None if weights is None else per_slot(weights)
        cfg = _lib.CoaddCfg(int(order), _lib.COADD_COMBINE[combine], float(n_sigma), int(scratch_rows))
        out = dict(image=np.empty((H, W), np.float32), weight=np.empty((H, W), np.float32),
                   count=np.empty((H, W), np.int32), n_rejected=np.empty((H, W), np.int32))
        ms = C.c_float()
        self.ctx.check(self._l.lc_frames_coadd(
            handle, n, frame.ctypes.data_as(_i32p), affine.ctypes.data_as(_lib.dp), ptr(g), ptr(wt), H, W, x0, y0,
            C.byref(cfg), ptr(out['image']), ptr(out['weight']), out['count'].ctypes.data_as(_i32p),
            out['n_rejected'].ctypes.data_as(_i32p), C.byref(ms)), 'lc_frames_coadd')
        out['kernel_ms'] = ms.value
        return out

    def subtract_reference(self, frame_index, transforms, reference, origin=(0, 0), order=3, r=3, bg_degree=1,
                           regions=(1, 1), clip_iters=2, n_sigma=4.0, sigma=None, mask=None,
                           download=('diff', 'kernel', 'bg', 'scale', 'n_used', 'chi2', 'status'), scratch_frames=0):
        """Difference imaging on the resident planes in one device call (``lc_frames_subtract_reference``; DESIGN.md
        section 5 "Difference imaging").  The frames ``frame_index`` are resampled onto the grid of ``reference`` (H, W)
        at ``origin`` (x0, y0) exactly as ``coadd`` resamples them (transforms, order: as there), and per frame and region
        the reference is matched to the frame and subtracted (r, bg_degree, regions, clip_iters, n_sigma, mask, download
        and the returned dict: as ``processes.difference_imaging.match_and_subtract``; mask (n, H, W), by listed frame).
        sigma: the pixel noise per listed frame, for the clipping and chi2; by default, after ``import_frames``, the
        recorded ``globalrms`` times |det| of the transform; an error when neither is there.  ``scratch_frames``: frames
        per chunk (0: from a budget); the result does not depend on it.  The planes stay as they are."""
        from .processes import difference_imaging as di
        what = 'subtract_reference'
        handle = self._handle()
        K = self.shape[0]
        frame = np.ascontiguousarray(np.asarray(frame_index, np.int32).reshape(-1))
        n = len(frame)
        if n < 1:
            raise ValueError(f'{what}: no frame')
        if ((frame < 0) | (frame >= K)).any():
            raise ValueError(f'{what}: a frame index outside 0 .. {K - 1}')
        if hasattr(transforms, 'params') or (isinstance(transforms, np.ndarray) and transforms.ndim == 2):
            transforms = [transforms]
        if len(transforms) != n:
            raise ValueError(f'{what}: {n} frames but {len(transforms)} transforms')
        affine = np.empty((n, 6), np.float64)
        for k, t in enumerate(transforms):
            m = np.asarray(t.params if hasattr(t, 'params') else t, np.float64)
            if m.shape not in ((2, 3), (3, 3)):
                raise ValueError(f'{what}: a transform of shape {m.shape}, not (2, 3) or (3, 3)')
            affine[k] = m[:2].reshape(6)
        ref = f32(reference)
        if ref.ndim != 2 or 0 in ref.shape:
            raise ValueError(f'{what}: the reference must be a 2-D image, got {ref.shape}')
        H, W = ref.shape
        if order not in (1, 3):
            raise ValueError(f'{what}: order must be 1 or 3, not {order!r}')
        if int(scratch_frames) < 0:
            raise ValueError(f'{what}: scratch_frames must be >= 0')
        cfg, gy, gx = di._settings((H, W), r, bg_degree, regions, clip_iters, n_sigma, download, what)
        if sigma is None:
            if not self.imported:
                raise ValueError(f'{what}: sigma is needed on a set that has not been imported')
            det = np.abs(affine[:, 0] * affine[:, 4] - affine[:, 1] * affine[:, 3])
            sigma = self._globalrms[frame].astype(np.float64) * det
        s = di._per_slot(sigma, n, what)
        m = di._mask(mask, (n, H, W), what)
        arrays, struct = di._outputs(n, (H, W), cfg, download)
        ms = C.c_float()
        self.ctx.check(self._l.lc_frames_subtract_reference(
            handle, n, frame.ctypes.data_as(_i32p), affine.ctypes.data_as(_lib.dp), H, W, int(origin[0]), int(origin[1]),
            int(order), ptr(ref), ptr(s), None if m is None else m.ctypes.data_as(_u8p), C.byref(cfg), int(scratch_frames),
            C.byref(struct), C.byref(ms)), 'lc_frames_subtract_reference')
        arrays['kernel_ms'] = ms.value
        return arrays

    def detect_cosmics(self, frame_index=None, exptimes=None, background_rms=None, noise=None, inmask=None, apply=None,
                       cosmics_masking_params=None, download=('crmask',), scratch_frames=0):
        """The cosmic rays of whole frames, on the resident planes in one device call (``lc_frames_detect_cosmics``;
        DESIGN.md section 5 "Cosmic rays of whole frames").  frame_index: the frames to take (default: all).  noise
        'rms': the variance is the square of the noise map ``cut_stamps`` forms, from exptimes and background_rms (one
        per frame of the set, or one for all; after ``import_frames`` both default to the recorded values); 'model': the
        SPEC's noise model from the data and ``readnoise``.  The default is 'rms' on an imported set and 'model'
        otherwise.  inmask: (n, h, w) bool, one per listed frame.  apply: None leaves the planes as they are; 'nan' sets
        the flagged pixels of the planes to NaN, which ``coadd`` and ``cut_stamps`` treat as missing; 'clean' replaces
        them by the cleaned values (a frame may then be listed once only).  cosmics_masking_params: the reference's
        dict, as ``cut_stamps`` takes it; only ``sepmed=True`` is built for frames.  download: which of 'crmask' and
        'clean' come back to the host: with ``download=()`` no frame-sized array moves.  ``scratch_frames``: frames per
        chunk (0: from a budget); the result does not depend on it.  Returns dict(crmask (n, h, w) bool or None, clean
        (n, h, w) float32 or None, iters, n_flagged int32 (n,), kernel_ms)."""
        from .processes.cutout_making import _mask_settings
        handle = self._handle()
        K, h, w = self.shape
        frame = np.arange(K, dtype=np.int32) if frame_index is None else \
            np.ascontiguousarray(np.asarray(frame_index, np.int32).reshape(-1))
        n = len(frame)
        if n < 1:
            raise ValueError('detect_cosmics: no frame')
        if ((frame < 0) | (frame >= K)).any():
            raise ValueError(f'detect_cosmics: a frame index outside 0 .. {K - 1}')
        if apply not in _lib.COSMICS_APPLY:
            raise ValueError(f'detect_cosmics: apply must be one of {tuple(_lib.COSMICS_APPLY)}, not {apply!r}')
        if apply is not None and len(np.unique(frame)) != n:
            raise ValueError('detect_cosmics: a frame listed twice with apply')
        noise = ('rms' if self.imported else 'model') if noise is None else noise
        if noise not in ('rms', 'model'):
            raise ValueError(f"detect_cosmics: noise must be 'rms' or 'model', not {noise!r}")
        unknown = set(download) - {'crmask', 'clean'}
        if unknown:
            raise ValueError(f'detect_cosmics: download takes crmask and clean, not {sorted(unknown)}')
        ccfg, _ = _mask_settings(dict(cosmics_masking_params or {}))
        if not ccfg.sepmed:
            raise NotImplementedError('detect_cosmics: only the separable medians (sepmed=True) are built for frames')
        if not self._l.lc_cosmics_frames_supported(h, w):
            raise _lib.LcError(f'lc_frames_detect_cosmics takes frames of h, w >= 8 with h w < 2^31, not {h} x {w}')
        t, rms = (_per_frame(exptimes, K), _per_frame(background_rms, K)) if noise == 'rms' else (None, None)
        if t is not None and not (np.isfinite(t) & (t > 0)).all():
            raise ValueError('exposure times must be finite and > 0')
        m = None
        if inmask is not None:
            m = np.ascontiguousarray(np.asarray(inmask).astype(np.uint8))
            if m.shape != (n, h, w):
                raise ValueError(f'detect_cosmics: inmask must have the shape {(n, h, w)}')
        cr = np.empty((n, h, w), np.uint8) if 'crmask' in download else None
        clean = np.empty((n, h, w), np.float32) if 'clean' in download else None
        iters = np.empty(n, np.int32)
        flagged = np.empty(n, np.int32)
        u8 = lambda a: None if a is None else a.ctypes.data_as(_u8p)
        ms = C.c_float()
        self.ctx.check(self._l.lc_frames_detect_cosmics(
            handle, n, frame.ctypes.data_as(_i32p), ptr(t), ptr(rms), int(noise == 'rms'), u8(m), C.byref(ccfg),
            _lib.COSMICS_APPLY[apply], int(scratch_frames), u8(cr), ptr(clean), iters.ctypes.data_as(_i32p),
            flagged.ctypes.data_as(_i32p), C.byref(ms)), 'lc_frames_detect_cosmics')
        return dict(crmask=None if cr is None else cr.astype(bool), clean=clean, iters=iters, n_flagged=flagged,
                    kernel_ms=ms.value)

    def close(self):
        if getattr(self, 'h', None):
            self._l.lc_frames_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        # (as Context.__del__: not while the interpreter shuts down)
        try:
            import sys
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass
