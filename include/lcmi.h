/*
 * lcmi.h - C ABI of liblcmi.so, the MI355X (gfx950) implementation of lightcurver's
 * PSF-fit + joint forward-model hot path.
 *
 * The reference (duxfrederic/lightcurver) has no FFI for this path: it calls the third-party
 * STARRED/JAX package from Python.  Each entry point below therefore cites the reference *call
 * site* whose arithmetic it replaces (paths relative to the reference repository root); the
 * ctypes stub a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, int status (0 = ok, < 0 = error; message through
 *     lc_last_error()).  No torch / numpy types.
 *   - All array arguments are HOST pointers unless the name ends in _dev.  Inputs are copied at
 *     call time, outputs are written into caller-allocated buffers.  float = IEEE fp32, the
 *     arithmetic type of the path (the reference stores stamps as float32:
 *     lightcurver/processes/cutout_making.py:48-49).
 *   - One context per device, one thread per context.
 *   - Layouts are C-contiguous; images are [row = y][col = x]; c_x, dx, x0 run along columns.
 */
#ifndef LCMI_H
#define LCMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_OK 0
#define LC_ERR_INVALID (-1)
#define LC_ERR_DEVICE (-2)
#define LC_ERR_UNSUPPORTED (-3)
#define LC_ERR_NONFINITE (-4)

typedef struct lc_ctx lc_ctx;
typedef struct lc_psf_batch lc_psf_batch;
typedef struct lc_joint lc_joint;

/* ---- context ------------------------------------------------------------------------------ */
int lc_version(void);
int lc_ctx_create(int device, lc_ctx **out);
void lc_ctx_destroy(lc_ctx *ctx);
const char *lc_last_error(const lc_ctx *ctx); /* ctx may be NULL: last error of a failed create */
int lc_ctx_synchronize(lc_ctx *ctx);
/* the hipStream_t every kernel of this context is enqueued on (and its device ordinal), so that a caller can
 * order its own work -- e.g. the RCCL all-reduce of the joint fit's shared block -- without a host sync */
int lc_ctx_stream(lc_ctx *ctx, void **hip_stream, int *device);
/* HIP-event timer on the context's stream (the stream every kernel of this library runs on). */
int lc_timer_start(lc_ctx *ctx);
int lc_timer_stop(lc_ctx *ctx, float *elapsed_ms);
/* device name + CU count, for reports */
int lc_device_info(lc_ctx *ctx, char *name, int name_len, int *n_cu, int64_t *hbm_bytes);

/* measured device copy bandwidth (read + write bytes / s) of a float4 grid-stride copy of `bytes` bytes, `reps`
 * launches: the box's own HBM figure that bench.py reports beside the 8 TB/s specification */
int lc_copy_bandwidth(lc_ctx *ctx, int64_t bytes, int reps, float *gb_per_s);
/* Measurement aid: synchronises the context's stream, launches `lc_marker_kernel` on a grid of `tag` (1 .. 65535) one-wave
 * workgroups and synchronises again - a dispatch whose grid size identifies it in a rocprofv3 trace or counter CSV, so that
 * the rows of a section (the iterations of one workload) can be cut out between two markers (bench.py, roofline.traffic). */
int lc_ctx_marker(lc_ctx *ctx, int tag);

/* ---- stamp pre-processing --------------------------------------------
 * One fused pass over K stamps of npix pixels, replacing the host-side NumPy of the reference:
 *   noise map from the background rms when `noisemap` is NULL: max(sqrt((t rms)^2 + |t data|), 1e-7) / t
 *     (lightcurver/processes/cutout_making.py:43-51; rms[K] in e-/s, exptime[K] = t);
 *   data, noisemap /= coefficient[K] when given (roi_file_preparation.py:162-164);
 *   pixels that are NaN in both inputs: data = 0, noisemap = nan_noise (1.0 at psf_modelling.py:139-143,
 *     1e7 at roi_file_preparation.py:194-196 and star_photometry.py:309-311), counted as masked;
 *   bad[K][npix] (1 = flagged cosmic / bad pixel, may be NULL): masked; with noise_boost > 0 the noise map is
 *     multiplied by it at the flagged pixels (roi_file_preparation.py:201) or, boost_whole_stamp != 0, once over
 *     every stamp that holds a flagged pixel (star_photometry.py:316);
 *   masked_count[K]: masked pixels per stamp, for the 40 % cut of psf_modelling.py:144-153.
 * Outputs (any may be NULL): data_out, noisemap_out, weight_out = good / noisemap^2 (what lc_psf_batch_create
 * takes), masked_count; kernel_ms = device time of the kernel alone (HIP events). */
int lc_prepare_stamps(lc_ctx *ctx, int K, int npix, const float *data, const float *noisemap, const float *rms,
                      const float *exptime, const float *coefficient, const uint8_t *bad, float nan_noise,
                      float noise_boost, int boost_whole_stamp, float *data_out, float *noisemap_out,
                      float *weight_out, int32_t *masked_count, float *kernel_ms);

/* ---- cosmic-ray mask of the stamps: replaces astroscrappy.detect_cosmics ----------------------
 * Reference call site: lightcurver/processes/cutout_making.py:85 (once per stamp, from :194 for the ROI and :247 for each
 * star), with the arguments of config.yaml:209-214.  L.A.Cosmic as frozen in DESIGN.md §5 "Cosmic-ray detection": every
 * float32 operation fixed, so one call over K stamps gives the bits of the SPEC's float32 restatement.
 *   data [K][n][n]; invar [K][n][n] variance (the reference passes noisemap^2) or NULL (noise from the median-filtered
 *   data and readnoise); inmask [K][n][n] (1 = bad) or NULL.  Non-finite data or invar and invar <= 0 are masked, C = 0.
 *   crmask [K][n][n] (1 = cosmic); clean [K][n][n] the meanmask-cleaned stamp / gain; iters [K] iterations done (the loop
 *   stops after the first one that adds nothing); kernel_ms = device time of the kernel (HIP events).
 * Any square n from 8 to 128 (lc_cosmics_supported, no device needed; LC_ERR_UNSUPPORTED otherwise), any K, one launch.
 * cleantype / fsmode other than 0 (astroscrappy's 'meanmask' / 'median') return LC_ERR_UNSUPPORTED. */
typedef struct {
  float sigclip, sigfrac, objlim; /* 4.5, 0.3, 5.0 */
  float gain, readnoise, satlevel; /* 1.0, 6.5, 65536.0 */
  int32_t niter;                   /* 4 */
  int32_t sepmed;                  /* 1: separable medians (7, 5, 9); 0: full (5, 3, 7) */
  int32_t cleantype;               /* 0 = meanmask (the only one built) */
  int32_t fsmode;                  /* 0 = median (the only one built) */
} lc_cosmics_cfg;
int lc_cosmics_supported(int n);
int lc_detect_cosmics(lc_ctx *ctx, int K, int n, const float *data, const float *invar /*nullable*/,
                      const uint8_t *inmask /*nullable*/, const lc_cosmics_cfg *cfg, uint8_t *crmask,
                      float *clean /*nullable*/, int32_t *iters /*nullable*/, float *kernel_ms /*nullable*/);

/* ---- bad rows and columns of the stamps: replaces ccdproc.ccdmask inside mask_cutout ------------
 * Reference call site: lightcurver/processes/cutout_making.py:67-80 (once per stamp, when mask_bad_rows_and_columns is
 * set, config.yaml:208): ccdmask(ccd, findbadcolumns=True), then the columns and rows flagged at both ends of the stamp.
 * ccdmask(byblocks=False) as frozen in DESIGN.md section 5 "Bad rows and columns": R = D - med7x7(D) (scipy's reflect
 * boundary), sigma = (P(69.1) - P(30.9)) / 2 of R (NumPy's linear percentile, in float32), flagged where R < -lsigma sigma
 * or R > hsigma sigma or D is not finite (sigma = NaN for a stamp with such a pixel: nothing else is flagged there), gaps
 * of at most ngood pixels between flagged pixels of a column filled (findbadcolumns).
 *   data [K][n][n].  Outputs, any may be NULL but not all: mask [K][n][n] the ccdmask result (1 = bad); bad_cols [K][n],
 *   bad_rows [K][n]: mask set at both ends of the column / row; rowcol [K][n][n]: those columns and rows, whole (what
 *   mask_cutout ORs into the cosmics mask); sigma [K]; kernel_ms = device time of the kernel (HIP events).
 * Any square n from 8 to 128 (lc_ccdmask_supported, no device needed; LC_ERR_UNSUPPORTED otherwise), any K, one launch.
 * LC_ERR_UNSUPPORTED: byblocks != 0, ncmed or nlmed != 7.  LC_ERR_INVALID: lsigma or hsigma not finite, ngood < 0. */
typedef struct {
  int32_t ncmed, nlmed;   /* 7, 7 (the only window built) */
  float lsigma, hsigma;   /* 9.0, 9.0 */
  int32_t ngood;          /* 5 */
  int32_t byblocks;       /* 0 (the only one built) */
  int32_t findbadcolumns; /* 1: fill the short gaps along columns; 0: the mask of the threshold alone */
} lc_ccdmask_cfg;
int lc_ccdmask_supported(int n);
int lc_ccdmask_stamps(lc_ctx *ctx, int K, int n, const float *data, const lc_ccdmask_cfg *cfg, uint8_t *mask /*nullable*/,
                      uint8_t *rowcol /*nullable*/, uint8_t *bad_cols /*nullable*/, uint8_t *bad_rows /*nullable*/,
                      float *sigma /*nullable*/, float *kernel_ms /*nullable*/);

/* ---- the whole of the reference's mask_cutout (cutout_making.py:54-91) in one call ------------
 * The stack is uploaded once; with do_bad_columns the rowcol of lc_ccdmask_stamps, with do_cosmics the crmask of
 * lc_detect_cosmics(invar = noisemap^2, formed on the device, no inmask), ORed on the device: mask [K][n][n], 1 = masked.
 * noisemap and cosmics_cfg may be NULL without do_cosmics, ccdmask_cfg without do_bad_columns; both switches off gives
 * a zero mask without a device call.  Sizes and error codes are those of the two calls; kernel_ms = device time of all
 * kernels (HIP events). */
int lc_mask_cutouts(lc_ctx *ctx, int K, int n, const float *data, const float *noisemap /*nullable*/, int do_bad_columns,
                    int do_cosmics, const lc_cosmics_cfg *cosmics_cfg /*nullable*/,
                    const lc_ccdmask_cfg *ccdmask_cfg /*nullable*/, uint8_t *mask, float *kernel_ms /*nullable*/);

/* ---- neighbouring sources of the star stamps: replaces sep.extract inside mask_surrounding_stars -----------
 * Reference call site: lightcurver/processes/psf_modelling.py:45 (once per star stamp, loop at :129-133) with
 * thresh = 3, minarea = 15, deblend_cont = 0.001 and sep's defaults deblend_nthresh = 32, clean = True, clean_param = 1.
 * Matched filter, 8-connected groups, multi-threshold de-blending, clean and the choice of the central object as frozen
 * in DESIGN.md §5 "Source masking": one call over K stamps gives the bits of the SPEC's restatement.
 *   data, noisemap [K][n][n]; a pixel with non-finite data or noise, or noise <= 0, carries no weight.
 *   mask [K][n][n]: 1 = good pixel, 0 = a pixel of any object other than the one nearest the stamp centre;
 *   segmap [K][n][n]: pixels of object i carry i + 1, the rest 0; nobj [K]; xy [K][LC_SEGMENT_MAX_OBJECTS][2]: the
 *   barycentres (x = column, y = row) of the objects, 0 past nobj; status [K]: 0 fine, 1 more than
 *   LC_SEGMENT_MAX_OBJECTS objects before clean or more than 64 nodes in the de-blending trees, 2 an iteration bound
 *   was reached, 3 a detected pixel with S/N >= 65536 (outside the fixed-point range of the sums).  A stamp with a
 *   non-zero status has mask = 1, segmap = 0, nobj = 0, xy = 0.  kernel_ms = device time of the kernel (HIP events).
 * Any square n from 8 to 64 (lc_segment_supported, no device needed), any K, one launch.  LC_ERR_UNSUPPORTED: n outside
 * that range, clean_param != 1, deblend_nthresh not 4, 8, 16 or 32, minarea < 1.  LC_ERR_INVALID: thresh <= 0 or
 * deblend_cont < 0 or either not finite. */
#define LC_SEGMENT_MAX_OBJECTS 32
typedef struct {
  float thresh;            /* 3.0 */
  int32_t minarea;         /* 15 */
  int32_t deblend_nthresh; /* 32 */
  float deblend_cont;      /* 0.001 */
  float clean_param;       /* 1.0 (the only one built) */
  int32_t clean;           /* 1 */
} lc_segment_cfg;
int lc_segment_supported(int n);
int lc_segment_stamps(lc_ctx *ctx, int K, int n, const float *data, const float *noisemap, const lc_segment_cfg *cfg,
                      uint8_t *mask, int32_t *segmap /*nullable*/, int32_t *nobj /*nullable*/, float *xy /*nullable*/,
                      int32_t *status /*nullable*/, float *kernel_ms /*nullable*/);

/* ---- alignment and stacking of the ROI epochs (the reference's stack_data_diagnostic, roi_modelling.py:34-125) ---------------
 * Align: every epoch e of every cube goes through scipy's rotate(shift(img, shift_yx[e]), angle_deg[e], reshape=False) with
 *   scipy's defaults: cubic B-spline prefilter (pole sqrt(3) - 2, whole-sample mirror boundaries), resample with 4 x 4
 *   taps, 0 where the coordinate leaves [0, n - 1]; twice, once per step (DESIGN.md section 5 "Align and stack").
 *   Coordinates and the in-range test in double, weights and sums in float.  shift_yx = (-dy, -dx) of the fit, angle = alpha.
 *   shift_yx and angle_deg both NULL: no alignment, the cubes are stacked as they are.
 * Stack: per pixel over the epochs whose (aligned) value is finite: median (exact order statistic, 0.5 (lo + hi) for an even
 *   count), standard deviation (ddof 0, two passes), epoch kept if |v - median| <= n_sigma * deviation or the deviation is
 *   not finite, stack = sum w v / sum w with w = 1 / noisemap over the kept epochs (the noise map as given, not aligned; 0 / 0
 *   = NaN).  clip = 0: every finite epoch is kept.  n_rejected: finite epochs the clip dropped.
 * Any output may be NULL; noisemap may be NULL when stack and n_rejected are; cfg NULL = {3.0, 1}.  kernel_ms = device time
 * of both kernels (HIP events).  Any square n from 8 to 128 (lc_align_stack_supported, no device needed; LC_ERR_UNSUPPORTED
 * otherwise), any C <= 65535, any E.  LC_ERR_INVALID: C or E < 1, a non-finite shift or angle, n_sigma <= 0 or not finite,
 * only one of shift_yx and angle_deg given. */
typedef struct {
  float n_sigma; /* 3.0 */
  int32_t clip;  /* 1 = one rejection pass, 0 = plain weighted mean */
} lc_stack_cfg;
int lc_align_stack_supported(int n);
int lc_align_stack(lc_ctx *ctx, int C, int E, int n, const float *cubes /* [C][E][n][n] */,
                   const float *noisemap /* [E][n][n], shared by the C cubes */,
                   const double *shift_yx /* [E][2] */, const double *angle_deg /* [E] */, const lc_stack_cfg *cfg,
                   float *aligned /* nullable [C][E][n][n] */, float *stack /* nullable [C][n][n] */,
                   float *median /* nullable [C][n][n] */, int32_t *n_rejected /* nullable [C][n][n] */,
                   float *kernel_ms /* nullable */);

/* ---- sky background of whole frames: replaces sep.Background inside subtract_background ---------------
 * Reference call site: lightcurver/processes/background_estimation.py:25 (called at frame_importation.py:81-91):
 * sep.Background(image, bw=box, bh=box, fw=3, fh=3), image - bkg, bkg.globalrms.  SExtractor's mesh background as frozen
 * in DESIGN.md section 5 "Sky background": per mesh of bw x bh pixels the clipped moments, the histogram and its mode;
 * bad meshes filled from the nearest good ones; the fw x fh median of the mesh values; globalback / globalrms the medians
 * of the filtered meshes; the map a natural bicubic spline through the mesh values; sub = data - back.
 *   data [K][h][w]; mask [K][h][w], non-zero = ignore (a non-finite pixel is ignored as well).
 *   nx = (w - 1) / bw + 1, ny = (h - 1) / bh + 1.  Outputs: sub, back [K][h][w]; mesh_back, mesh_rms [K][ny][nx] (after the
 *   median filter); globalback, globalrms [K]; status [K]: 0, or LC_ERR_NONFINITE for a frame without one good mesh (its
 *   outputs are NaN, the other frames of the call are not affected); kernel_ms = device time of all kernels (HIP events).
 * Any h, w >= 1, any K; fw = fh = 1 or 3, fthresh = 0, nx and ny <= 256 and nx * ny <= 2048 (lc_background_supported, no
 * device needed; LC_ERR_UNSUPPORTED otherwise).  LC_ERR_INVALID: K, h, w, bw or bh < 1, fthresh not finite.
 * lc_background_map evaluates the same spline through any mesh values (bkg.rms() of sep: the spline through mesh_rms). */
typedef struct {
  int32_t bw, bh; /* mesh size in pixels; the reference: min(h, w) / 10 for both */
  int32_t fw, fh; /* 3, 3 (1, 1: no filter) */
  float fthresh;  /* 0.0 (the only one built) */
} lc_background_cfg;
int lc_background_supported(int h, int w, int bw, int bh, int fw, int fh);
int lc_background_frames(lc_ctx *ctx, int K, int h, int w, const float *data, const uint8_t *mask /*nullable*/,
                         const lc_background_cfg *cfg, float *sub /*nullable*/, float *back /*nullable*/,
                         float *mesh_back /*nullable [K][ny][nx]*/, float *mesh_rms /*nullable [K][ny][nx]*/,
                         float *globalback /*[K]*/, float *globalrms /*[K]*/, int32_t *status /*[K] nullable*/,
                         float *kernel_ms /*nullable*/);
int lc_background_map(lc_ctx *ctx, int K, int h, int w, int bw, int bh, const float *mesh /*[K][ny][nx]*/,
                      float *map /*[K][h][w]*/, float *kernel_ms /*nullable*/);

/* ---- source extraction of whole frames: replaces sep.extract over frames ------------------------------
 * Reference call sites: lightcurver/processes/star_extraction.py:23 (extract_stars, called at frame_importation.py:130)
 * and background_estimation.py:32 (the source mask of the two-pass sky).  Detection, 8-connected labelling and
 * measurement as frozen in DESIGN.md section 5 "Source extraction of frames": sep.extract WITHOUT de-blending and
 * WITHOUT cleaning (sep's deblend_cont = 1.0, clean = False).
 *   data [K][h][w]; var [K][h][w] (a variance, not an rms), or NULL and var_scalar [K] one variance per frame.
 *   A pixel is valid if data and variance are finite and the variance > 0.  filter 1: sep's default 3 x 3 matched
 *   filter; 0: none.  Detected: snr > thresh.  Objects: the 8-connected components of at least minarea pixels, numbered
 *   from 1 in the raster order of their first pixels.
 *   Outputs: objects [K][max_objects] (rows past nobj are zero); nobj [K] the true count; segmap [K][h][w] the object
 *   number or 0; mask [K][h][w] = segmap > 0; status [K]: 0, 1 = nobj > max_objects (the table holds the first
 *   max_objects objects, segmap and mask are complete), 2 = an iteration guard of the labelling was reached (no input
 *   reaches it; the frame's outputs are zero).  The other frames of a call are not affected by a frame's status.
 *   flag bits: 1 = a bounding-box side > 512 pixels, 2 = a pixel with snr >= 2^16 or not finite (both: x, y, a, b, theta
 *   are NaN), 4 = the box touches the frame border.
 * Any h, w >= 1 with h * w < 2^31 (lc_extract_supported, no device needed; LC_ERR_UNSUPPORTED otherwise, and for a K
 * whose frames do not fit one grid).  LC_ERR_INVALID: K < 1, thresh <= 0 or not finite, minarea < 1, filter not 0 or 1,
 * max_objects < 1, a missing pointer. */
typedef struct {
  float thresh;    /* in units of the pixel's noise; the reference: 3 (catalogue), 2 (source mask) */
  int32_t minarea; /* the reference: 10 */
  int32_t filter;  /* 1: sep's default 3 x 3 kernel, 0: filter_kernel=None */
} lc_extract_cfg;
typedef struct {
  int32_t first; /* raster index y * w + x of the object's first pixel */
  int32_t npix, xmin, xmax, ymin, ymax;
  int32_t xpeak, ypeak; /* first raster position of the largest snr */
  int32_t flag, pad;
  float peak, cpeak; /* largest data value (of the finite ones), largest snr */
  double x, y, a, b, theta, flux;
} lc_extract_object; /* 96 bytes */
int lc_extract_supported(int h, int w);
int lc_extract_frames(lc_ctx *ctx, int K, int h, int w, const float *data, const float *var /*nullable*/,
                      const float *var_scalar /*[K], read when var is null*/, const lc_extract_cfg *cfg, int max_objects,
                      lc_extract_object *objects /*nullable*/, int32_t *nobj /*[K]*/, int32_t *segmap /*nullable*/,
                      uint8_t *mask /*nullable*/, int32_t *status /*[K]*/, float *kernel_ms /*nullable*/);

/* ---- the same with sep's de-blending and cleaning: sep.extract as the reference calls it --------------------
 * DESIGN.md section 5 "De-blending and cleaning of frame objects".  The parents are the objects of lc_extract_frames.  A
 * parent whose box has both sides <= 64 pixels and that is not flagged RANGE is de-blended inside its box by the tree of
 * lc_segment_stamps (deblend_nthresh levels, the contrast deblend_cont, at most LC_SEGMENT_MAX_OBJECTS leaves and 64 tree
 * nodes per parent); its leaves are objects whatever their size.  A parent with a larger box, or one that exceeds a
 * capacity, stays whole and carries flag bit 8 (LC_EXTRACT_FLAG_NODEBLEND); the frame's status is not affected.  With
 * clean != 0 every object is then merged into the brighter neighbour whose Moffat wing exceeds it (sep's clean with
 * clean_param 1), chains followed to their ends.  The final objects are numbered in the raster order of their first
 * pixels and measured as in lc_extract_frames; segmap and mask follow that numbering.  With deblend_cont >= 1 and
 * clean = 0 everything but flag bit 8 equals lc_extract_frames bit for bit.
 *   Arguments, outputs, status and error codes as lc_extract_frames.  LC_ERR_UNSUPPORTED also for clean_param != 1 and a
 *   deblend_nthresh other than 4, 8, 16 or 32; LC_ERR_INVALID also for a deblend_cont that is negative or not finite and
 *   a missing dcfg.  The call waits for the device twice before its last launch, to size its tables. */
#define LC_EXTRACT_FLAG_NODEBLEND 8
typedef struct {
  int32_t deblend_nthresh; /* sep: 32; 4, 8, 16 or 32 */
  float deblend_cont;      /* sep: 0.005; >= 1: no de-blending */
  int32_t clean;           /* sep: 1 */
  float clean_param;       /* sep: 1.0, the only one built */
} lc_deblend_cfg;
int lc_extract_frames_deblended(lc_ctx *ctx, int K, int h, int w, const float *data, const float *var /*nullable*/,
                                const float *var_scalar /*[K], read when var is null*/, const lc_extract_cfg *cfg,
                                const lc_deblend_cfg *dcfg, int max_objects, lc_extract_object *objects /*nullable*/,
                                int32_t *nobj /*[K]*/, int32_t *segmap /*nullable*/, uint8_t *mask /*nullable*/,
                                int32_t *status /*[K]*/, float *kernel_ms /*nullable*/);

/* ---- the arithmetic of importing a frame, with the frame uploaded once -----------------------------------
 * Reference: lightcurver/processes/frame_importation.py:81-141.  data [K][h][w] in electrons per second, exptime [K].
 *   1. the sky background as lc_background_frames (bcfg);
 *   2. if mask_sources_first: lc_extract_frames of sub with the scalar variance globalrms^2 and mcfg (the reference:
 *      thresh 2, minarea 10, filter 1), then the background again with that mask (background_estimation.py:32-37);
 *   3. the variance plane in float32 without fused multiply-adds: rt = globalrms t, v = (rt rt + |sub t|) / (t t);
 *   4. lc_extract_frames of sub with v and ecfg.
 * Outputs: sub [K][h][w]; mesh_back, mesh_rms [K][ny][nx] (nullable); globalback, globalrms [K]; bg_status [K]
 * (nullable) as lc_background_frames; objects, nobj, segmap (nullable), ex_status as lc_extract_frames; kernel_ms.
 * Errors as the two entries it chains; LC_ERR_INVALID also for an exptime that is not finite or <= 0. */
int lc_import_frames(lc_ctx *ctx, int K, int h, int w, const float *data, const float *exptime /*[K]*/,
                     const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg, int mask_sources_first,
                     const lc_extract_cfg *mcfg /*read when mask_sources_first*/, int max_objects, float *sub,
                     float *mesh_back /*nullable*/, float *mesh_rms /*nullable*/, float *globalback, float *globalrms,
                     int32_t *bg_status /*nullable*/, lc_extract_object *objects, int32_t *nobj,
                     int32_t *segmap /*nullable*/, int32_t *ex_status, float *kernel_ms /*nullable*/);
/* The same with step 4 as lc_extract_frames_deblended (dcfg); the source mask of step 2 is never de-blended. */
int lc_import_frames_deblended(lc_ctx *ctx, int K, int h, int w, const float *data, const float *exptime /*[K]*/,
                               const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg, const lc_deblend_cfg *dcfg,
                               int mask_sources_first, const lc_extract_cfg *mcfg /*read when mask_sources_first*/,
                               int max_objects, float *sub, float *mesh_back /*nullable*/, float *mesh_rms /*nullable*/,
                               float *globalback, float *globalrms, int32_t *bg_status /*nullable*/,
                               lc_extract_object *objects, int32_t *nobj, int32_t *segmap /*nullable*/,
                               int32_t *ex_status, float *kernel_ms /*nullable*/);

/* ---- a frame set that stays on the device, and the stamps cut from it -----------------------------------------
 * Reference: lightcurver/processes/cutout_making.py:23-51 (extract_stamp: Cutout2D(mode='partial', fill_value=nan) and the
 * noise map, once per stamp, called at :188 for the ROI and :238 for each star) on the sky-subtracted frame that
 * frame_importation.py:119 wrote.  Here the frames are uploaded once, imported where they lie, and every stamp of one
 * size is cut in one call (DESIGN.md section 5 "Stamp cutting").
 *   lc_frames_create   K frames of h x w, row-major float32, copied to the device; the object belongs to ctx and is
 *     destroyed before it.  lc_frames_get copies planes [first, first + count) back as they are now.
 *   lc_frames_import   what lc_import_frames runs, on the resident planes, with the same arguments, outputs and error
 *     codes after `exptime`; sub may be NULL.  Afterwards the resident planes are sub, the raw planes are freed and
 *     exptime and globalrms stay recorded on the device (lc_frames_info: imported = 1).  If a frame's object table was
 *     too small (ex_status 1) the call still returns LC_OK with every output filled, but the set stays as it was
 *     (imported = 0), so that the caller can import again with a larger max_objects.  LC_ERR_INVALID for a set that is
 *     imported already.  During the call the device holds sub and four more planes of scratch beside the raw frames.
 *   lc_frames_cut_stamps   S stamps of n x n in one call: stamp s has its corner at (y0[s], x0[s]) of frame frame[s]
 *     (frames in any order, repeated at will), pixel (i, j) = frame pixel (y0 + i, x0 + j), NaN outside the frame.
 *     noisemap_out = max(sqrt((t rms)^2 + |t data|), 1e-7) / t in the float32 steps of lc_prepare_stamps, NaN where data
 *     is; exptime (t) and rms [K] per frame of the set, each may be NULL after an import (the recorded values are used).
 *     mask_out: what lc_mask_cutouts returns for data_out and noisemap_out with the same switches and settings, formed
 *     on the stamps where they lie on the device; both switches off gives a zero mask.  n_inside [S]: pixels of the stamp
 *     that lie in the frame.  kernel_ms = device time of all kernels (HIP events).
 *     Checked on the host before anything is launched, LC_ERR_INVALID: S or n < 1, a missing pointer (data_out; mask_out
 *     with a switch on; the settings of a switch that is on), a frame index outside [0, K), a stamp without one pixel
 *     in the frame, an exptime that is not finite or not > 0, no exptime or rms (given or recorded) when noisemap_out
 *     or a switch is set.  LC_ERR_UNSUPPORTED: S n n >= 2^31; with a switch on, n outside 8 .. 128 and what the two mask
 *     calls refuse.  lc_cutout_supported(n, with_masks) answers for one stamp (1 / 0) without a device. */
typedef struct lc_frames lc_frames;
int lc_frames_create(lc_ctx *ctx, int K, int h, int w, const float *data /*[K][h][w]*/, lc_frames **out);
void lc_frames_destroy(lc_frames *f);
int lc_frames_info(lc_frames *f, int *K, int *h, int *w, int *imported); /* each may be NULL */
int lc_frames_get(lc_frames *f, int first, int count, float *out /*[count][h][w]*/);
int lc_frames_import(lc_frames *f, const float *exptime /*[K]*/, const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg,
                     int mask_sources_first, const lc_extract_cfg *mcfg /*read when mask_sources_first*/, int max_objects,
                     float *sub /*nullable*/, float *mesh_back /*nullable*/, float *mesh_rms /*nullable*/, float *globalback,
                     float *globalrms, int32_t *bg_status /*nullable*/, lc_extract_object *objects, int32_t *nobj,
                     int32_t *segmap /*nullable*/, int32_t *ex_status, float *kernel_ms /*nullable*/);
/* lc_frames_import with the catalogue as lc_extract_frames_deblended (dcfg) */
int lc_frames_import_deblended(lc_frames *f, const float *exptime /*[K]*/, const lc_background_cfg *bcfg,
                               const lc_extract_cfg *ecfg, const lc_deblend_cfg *dcfg, int mask_sources_first,
                               const lc_extract_cfg *mcfg /*read when mask_sources_first*/, int max_objects,
                               float *sub /*nullable*/, float *mesh_back /*nullable*/, float *mesh_rms /*nullable*/,
                               float *globalback, float *globalrms, int32_t *bg_status /*nullable*/,
                               lc_extract_object *objects, int32_t *nobj, int32_t *segmap /*nullable*/,
                               int32_t *ex_status, float *kernel_ms /*nullable*/);
int lc_cutout_supported(int n, int with_masks);
int lc_frames_cut_stamps(lc_frames *f, int S, int n, const int32_t *frame /*[S]*/, const int32_t *y0 /*[S]*/,
                         const int32_t *x0 /*[S]*/, const float *exptime /*[K], nullable after an import*/,
                         const float *rms /*[K], nullable after an import*/, int do_bad_columns, int do_cosmics,
                         const lc_cosmics_cfg *cosmics_cfg /*nullable*/, const lc_ccdmask_cfg *ccdmask_cfg /*nullable*/,
                         float *data_out /*[S][n][n]*/, float *noisemap_out /*nullable*/, uint8_t *mask_out /*nullable*/,
                         int32_t *n_inside /*[S] nullable*/, float *kernel_ms /*nullable*/);

/* ---- exact circular-aperture sums (photutils.aperture_photometry with CircularAperture, method='exact'), batched ------
 * The reference takes the starting fluxes of the ROI's point sources from exact circular apertures on the median stack
 * (lightcurver/processes/roi_modelling.py:198-204).  Here P apertures are summed in one call, one wave each (DESIGN.md
 * section 5 "Aperture sums" is the SPEC; csrc/aperture.hip).  Aperture p lies on image image[p] (images in any order,
 * repeated at will) with its centre at xy[p] = (x, y), x along the columns, 0-based with the pixel centres at integers,
 * and has radius r[p].  The weight of a pixel is the area of its square inside the circle, in float64.  A pixel is good
 * if it is in the image, not masked (mask != 0 excludes it) and its data and its error (when there is one) are finite.
 *   sum       sum of weight * data over the good pixels
 *   sum_err   sqrt(sum of weight * error^2) over the good pixels
 *   area      sum of the weights of the good pixels
 *   bad_area  sum of the weights of the bad pixels that are not masked
 * A circle that lies outside the image gives four zeros.  An aperture's outputs depend on nothing but the aperture and its
 * image: not on P, K, its place in the list or its neighbours, bit for bit.  kernel_ms = device time of the kernel (HIP
 * events).
 *   lc_aperture_sums         images, error map and mask are uploaded with the call.
 *   lc_frames_aperture_sums  on the resident planes of a frame set (raw, or sub after an import); only the list is
 *     uploaded.  with_error: the error of a pixel is the noise lc_frames_cut_stamps gives it, formed on the fly in the
 *     same float32 steps from exptime and rms [K], each of which may be NULL after an import (the recorded values are
 *     used).
 * Checked on the host before anything is launched, the outputs untouched.  LC_ERR_INVALID: K, h, w or P < 1, a missing
 * data, image, xy, r or sum, sum_err without an error source (error; with_error), an image index outside [0, K), a
 * coordinate or radius that is not finite, r <= 0, with_error without exptime and rms (given or recorded), an exptime
 * that is not finite or not > 0.  LC_ERR_UNSUPPORTED: lc_aperture_sums with K h w >= 2^31. */
int lc_aperture_sums(lc_ctx *ctx, int K, int h, int w, const float *data /*[K][h][w]*/, const float *error /*nullable*/,
                     const uint8_t *mask /*nullable*/, int P, const int32_t *image /*[P]*/, const double *xy /*[P][2]*/,
                     const double *r /*[P]*/, double *sum /*[P]*/, double *sum_err /*[P] nullable*/,
                     double *area /*[P] nullable*/, double *bad_area /*[P] nullable*/, float *kernel_ms /*nullable*/);
int lc_frames_aperture_sums(lc_frames *f, int P, const int32_t *frame /*[P]*/, const double *xy, const double *r,
                            const float *exptime /*[K], nullable after an import*/, const float *rms /*likewise*/,
                            int with_error, double *sum, double *sum_err /*nullable*/, double *area /*nullable*/,
                            double *bad_area /*nullable*/, float *kernel_ms /*nullable*/);

/* ---- co-addition of the registered frames of a set: the deep image of the field -------------------------------------
 * DESIGN.md section 5 "Co-addition of frames" is the SPEC; csrc/coadd.hip.  n frames of the set (frame[k], in any order,
 * repeated at will) are resampled onto a grid of H x W reference pixels whose pixel (i, j) is the reference pixel
 * (x0 + j, y0 + i), and combined per pixel.  affine[k] = a, b, c, d, e, f maps reference pixels to the pixels of frame k:
 * x' = (a x + b y) + c, y' = (d x + e y) + f, in double (the rows of lc_register_sources' transform, and of
 * SimilarityTransform.params[:2]).  order 1: bilinear; order 3: Keys' cubic convolution with a = -1/2, no prefilter.  A
 * sample is missing (NaN) unless every tap lies inside the frame; NaN taps propagate.  A sample is multiplied by
 * float32(flux_scale[k] |det affine[k]|), which keeps flux per reference pixel.  combine, over the finite samples of a
 * pixel in the order of the list, with the per-frame weight[k] where lc_align_stack has 1 / noise:
 *   LC_COADD_MEAN        sum w v / sum w
 *   LC_COADD_MEDIAN      the middle order statistic, 0.5 (lo + hi) for an even count; weights enter weight_out only
 *   LC_COADD_SIGMA_CLIP  median, population deviation, keep |v - median| <= n_sigma deviation, weighted mean of the kept
 * Outputs [H][W]: image; weight_out = sum of weight[k] over the kept samples; count = the kept samples; n_rejected.  A
 * pixel without a sample gives NaN, 0, 0, 0.  The results do not depend on scratch_rows, and a frame's samples do not
 * depend on what else is in the list, bit for bit.  Works on a raw or an imported set and leaves the planes unchanged.
 * Device memory beyond the set: the four outputs and n scratch_rows W samples.  kernel_ms = device time of all kernels.
 *   Checked on the host before anything is launched, the outputs untouched, LC_ERR_INVALID: n < 1, a missing frame,
 *   affine, cfg or image, a frame index outside [0, K), an affine entry that is not finite or det = 0, a flux scale that
 *   is not finite, a weight that is negative or not finite, H or W < 1, H W >= 2^31, an order other than 1 or 3, an
 *   unknown combine, n_sigma <= 0 or not finite, scratch_rows < 0. */
#define LC_COADD_MEAN 0
#define LC_COADD_MEDIAN 1
#define LC_COADD_SIGMA_CLIP 2
typedef struct {
  int32_t order;        /* 1 or 3 */
  int32_t combine;      /* LC_COADD_* */
  float n_sigma;        /* read by every combine: > 0 and finite */
  int32_t scratch_rows; /* output rows resampled per strip; 0: as many as fit a budget of 128 MiB */
} lc_coadd_cfg;
int lc_frames_coadd(lc_frames *f, int n, const int32_t *frame /*[n]*/, const double *affine /*[n][6]*/,
                    const float *flux_scale /*[n], nullable: 1*/, const float *weight /*[n], nullable: 1*/, int H, int W,
                    int x0, int y0, const lc_coadd_cfg *cfg, float *image /*[H][W]*/, float *weight_out /*nullable*/,
                    int32_t *count /*nullable*/, int32_t *n_rejected /*nullable*/, float *kernel_ms /*nullable*/);

/* ---- difference imaging: a reference image PSF-matched to each frame and subtracted ---------------------------------
 * DESIGN.md section 5 "Difference imaging" is the SPEC; csrc/diffim.hip.  Per frame k and region g of a gy x gx grid
 * (rows [i H / gy, (i + 1) H / gy), columns likewise) the (2r + 1)^2 free pixel values of a convolution kernel and a
 * polynomial background of degree bg_degree (terms 1, X, Y, X^2, XY, Y^2 of the region's coordinates in [-1, 1]) are
 * fitted by least squares so that M = reference (*) kernel + background matches the frame (a true convolution, indexed
 * as scipy.signal.convolve2d(reference, kernel, mode='same')), with clip_iters further rounds that leave out the pixels
 * with |D| > n_sigma sigma.  sigma: sqrt(var) where variances are given, else sigma[k], else the previous round's
 * residual rms.  The normal equations are summed in float64 on the device in a fixed order, solved by Cholesky in
 * float64 on the host, and D = frame - M is evaluated in float32.  Nothing depends on K, on what else shares the call,
 * on scratch_frames or on the run, bit for bit.
 *   lc_diffim_frames: host pointers.  target [K][h][w]; reference [h][w]; var [K][h][w], mask [K][h][w] (nonzero: out
 *   of the fit, D still computed) and sigma [K] nullable.
 *   lc_frames_subtract_reference: the same on the resident planes of a set.  Slot k is plane frame[k] resampled onto the
 *   grid of H x W reference pixels at (x0, y0) exactly as lc_frames_coadd resamples it with flux scale 1 (affine, order:
 *   as there; a missing sample is NaN and falls out of the fit).  mask [n][H][W], sigma [n]: by slot, nullable.  Frames
 *   are processed in chunks of scratch_frames (0: as many as fit a budget of 128 MiB, at least one).  The planes stay
 *   as they are.
 * Outputs (lc_diffim_out, each nullable, G = gy gx, P = (2r + 1)^2 + 1, 3 or 6): diff [K][h][w] (NaN within r pixels
 * of the border and wherever the frame or a reference pixel of the footprint is not finite); kernel [K][G][(2r + 1)^2];
 * bg [K][G][6] (unused entries 0); scale [K][G] = the sum of the kernel; n_used [K][G] = the pixels of the last round's
 * fit set; chi2 [K][G] = sum over them of D^2 / sigma^2, over n_used - P (with neither var nor sigma, sigma is the last
 * round's own rms); status [K][G]: 0 ok, 1 n_used < 2 P, 2 a pivot that is not positive (then kernel, bg, scale, chi2
 * and the region's diff are NaN; the call still returns LC_OK); gram [K][G][P][P] and rhs [K][G][P]: the normal
 * equations of the last round the region went through.  Beside them split_ms [3], a diagnostic that does not count
 * as an output: device time of the Gram sums, host time of the solves, device time of the subtraction.  kernel_ms: device time of all kernels.
 *   Checked on the host before anything is launched, the outputs untouched, LC_ERR_INVALID: K or n < 1; a missing
 *   target, reference, cfg, out or frame list; no output at all; a frame index outside [0, K); an affine entry that is
 *   not finite or det = 0; r outside [1, 7], bg_degree outside [0, 2], gy or gx < 1 or gy gx > 64, clip_iters < 0,
 *   n_sigma not finite or <= 0, an order other than 1 or 3; a sigma that is not finite or not > 0; scratch_frames < 0.
 *   LC_ERR_UNSUPPORTED: what lc_diffim_supported (no device needed) refuses: h or w < 2 r + 1, h w >= 2^31, a region
 *   without a pixel, and the ranges above. */
typedef struct {
  int32_t r, bg_degree, gy, gx, clip_iters;
  float n_sigma;
} lc_diffim_cfg;
typedef struct {
  float *diff;
  double *kernel, *bg, *scale;
  int32_t *n_used;
  double *chi2;
  int32_t *status;
  double *gram, *rhs;
  float *split_ms;
} lc_diffim_out;
int lc_diffim_supported(int h, int w, int r, int bg_degree, int gy, int gx);
int lc_diffim_frames(lc_ctx *ctx, int K, int h, int w, const float *target, const float *reference,
                     const float *var /*nullable*/, const uint8_t *mask /*nullable*/, const float *sigma /*nullable*/,
                     const lc_diffim_cfg *cfg, const lc_diffim_out *out, float *kernel_ms /*nullable*/);
int lc_frames_subtract_reference(lc_frames *f, int n, const int32_t *frame /*[n]*/, const double *affine /*[n][6]*/, int H,
                                 int W, int x0, int y0, int order, const float *reference /*[H][W]*/,
                                 const float *sigma /*[n] nullable*/, const uint8_t *mask /*[n][H][W] nullable*/,
                                 const lc_diffim_cfg *cfg, int scratch_frames, const lc_diffim_out *out,
                                 float *kernel_ms /*nullable*/);

/* ---- cosmic rays of whole frames: astroscrappy.detect_cosmics as upstream applies it, to an image of any size ----------
 * DESIGN.md section 5 "Cosmic rays of whole frames"; csrc/cosmics_frames.hip.  The SPEC of lc_detect_cosmics with "the
 * stamp" read as the frame of h x w pixels: the border rule of every median pass, the dilations, the 5 x 5 window of the
 * cleaning and the outermost ring of the 2x grid are the FRAME's, whatever the tiling.  One call over K frames gives the
 * bits of the SPEC's float32 restatement on each whole frame; the result depends neither on K nor on scratch_frames.
 *   lc_detect_cosmics_frames: host pointers, the frame twin of lc_detect_cosmics.  data, invar (nullable), inmask
 *   (nullable) [K][h][w] as there.  crmask [K][h][w]; clean [K][h][w] = the cleaned counts / gain; iters [K]; n_flagged
 *   [K] = the pixels of crmask; kernel_ms = device time of all launches (HIP events).
 *   lc_frames_detect_cosmics: the same on the resident planes of a set, slot k of the n slots being plane frame[k].
 *   noise_from_rms = 1: invar is formed on the device as the square, in float32, of the noise map lc_frames_cut_stamps
 *   and lc_frames_aperture_sums form from exptime and rms ([K], by plane; after an import both default to the recorded
 *   values, LC_ERR_INVALID when neither is there).  noise_from_rms = 0: the SPEC's noise model from the data and
 *   readnoise.  inmask, crmask, clean [n][h][w], iters, n_flagged [n]: by slot, each nullable.  apply: 0 leaves the
 *   planes as they are; LC_COSMICS_SET_NAN sets the flagged pixels of the planes to NaN (what lc_frames_coadd and the
 *   NaN rule of lc_frames_cut_stamps treat as missing); LC_COSMICS_SET_CLEAN replaces them by clean.
 * Frames are processed in chunks of scratch_frames frames (0: as many as fit a budget of 128 MiB, at least one): 6 bytes
 * of scratch per pixel, 10 with a variance.  Any h, w >= 8 with h w < 2^31 (lc_cosmics_frames_supported, no device
 * needed; LC_ERR_UNSUPPORTED otherwise).  Only sepmed = 1 is built for frames: sepmed = 0, and cleantype / fsmode other
 * than 0, return LC_ERR_UNSUPPORTED.
 *   Checked on the host before anything is launched, the outputs untouched, LC_ERR_INVALID: K or n < 1, a missing data,
 *   cfg, crmask (host-pointer form) or frame list; in the frames form no output at all with apply = 0, a frame index
 *   outside [0, K), a frame listed twice with apply != 0, an unknown apply, an exptime that is not finite or not > 0;
 *   the settings lc_detect_cosmics refuses; scratch_frames < 0. */
#define LC_COSMICS_SET_NAN 1
#define LC_COSMICS_SET_CLEAN 2
int lc_cosmics_frames_supported(int h, int w);
int lc_detect_cosmics_frames(lc_ctx *ctx, int K, int h, int w, const float *data, const float *invar /*nullable*/,
                             const uint8_t *inmask /*nullable*/, const lc_cosmics_cfg *cfg, int scratch_frames,
                             uint8_t *crmask /*[K][h][w]*/, float *clean /*nullable*/, int32_t *iters /*nullable*/,
                             int32_t *n_flagged /*nullable, [K]*/, float *kernel_ms /*nullable*/);
int lc_frames_detect_cosmics(lc_frames *f, int n, const int32_t *frame /*[n]*/, const float *exptime /*[K] nullable*/,
                             const float *rms /*[K] nullable*/, int noise_from_rms, const uint8_t *inmask /*[n][h][w] nullable*/,
                             const lc_cosmics_cfg *cfg, int apply, int scratch_frames, uint8_t *crmask /*nullable*/,
                             float *clean /*nullable*/, int32_t *iters /*nullable*/, int32_t *n_flagged /*nullable*/,
                             float *kernel_ms /*nullable*/);

/* ---- registration of source lists by star triangles (astroalign.find_transform), batched ----------------------------------
 * The reference gives a frame its WCS from another frame's, or from Gaia positions, with one astroalign.find_transform per
 * frame (lightcurver/processes/alternate_plate_solving_adapt_existing_wcs.py:24, alternate_plate_solving_with_gaia.py:66).
 * lc_register_sources solves K such problems in one call, one workgroup each (DESIGN.md section 5 "Frame registration" is
 * the SPEC; csrc/register.hip).  Problem k: the first nsrc[k] rows of src[k] against the first ntgt[k] rows of tgt[k],
 * (x, y) float64, brightest first, already cut to the control points.  Outputs per problem:
 *   transform  a, -b, tx, b, a, ty: target = [[a, -b], [b, a]] source + (tx, ty); NaN unless status is 0
 *   pairs      the matched (source row, target row), by source row; -1 past npairs[k]
 *   diag       source triangles, target triangles, matching triangle pairs, the winning hypothesis (-1: none), the inlier
 *              matches of the final fit
 *   status     0 solved; 1 no consensus (astroalign's MaxIterError), or a degenerate fit; 2 more than max_matches
 *              matching triangle pairs; 3 fewer than three points on a side (astroalign's ValueError)
 * A problem's status never affects another problem of the call, and its outputs do not depend on K or on its neighbours.
 * kernel_ms spans both kernels and the one wait between them that sizes the table of matches.
 * Checked on the host before anything is launched.  LC_ERR_INVALID: K < 1, a count outside [0, P], a coordinate inside a
 * count that is not finite, a missing pointer, max_matches < 1, a tolerance or fraction that is not finite or not > 0.
 * LC_ERR_UNSUPPORTED: P outside 3 .. 128 (lc_register_supported, no device needed). */
typedef struct {
  int32_t max_matches;         /* 65536 */
  double pixel_tol;            /* 2.0: astroalign's PIXEL_TOL */
  double invariant_radius;     /* 0.1: the radius of astroalign's query_ball_tree */
  double min_matches_fraction; /* 0.8: astroalign's MIN_MATCHES_FRACTION */
} lc_register_cfg;
int lc_register_supported(int max_points);
int lc_register_sources(lc_ctx *ctx, int K, int P, const double *src /*[K][P][2]*/, const int32_t *nsrc /*[K]*/,
                        const double *tgt /*[K][P][2]*/, const int32_t *ntgt /*[K]*/, const lc_register_cfg *cfg,
                        double *transform /*[K][6]*/, int32_t *pairs /*[K][P][2] nullable*/, int32_t *npairs /*[K]*/,
                        int32_t *diag /*[K][5] nullable*/, int32_t *status /*[K]*/, float *kernel_ms /*nullable*/);

/* ---- optimiser settings shared by both fits ----------------------------------------------- */
/* optax.adabelief as driven by STARRED's Optimizer(method='adabelief'):
 * lightcurver/processes/star_photometry.py:113-122, roi_modelling.py:326-334. */
typedef struct {
  float init_learning_rate;
  int32_t schedule_learning_rate; /* 0/1: lr_t = lr0 * decay_rate^(t / transition_steps) */
  float decay_rate;               /* default 0.99 */
  int32_t transition_steps;       /* default 10 */
  float b1, b2, eps, eps_root;    /* defaults 0.9, 0.999, 1e-16, 1e-16 */
} lc_adabelief_cfg;
void lc_adabelief_defaults(lc_adabelief_cfg *cfg);

/* ---- PSF fit: replaces starred.procedures.psf_routines.build_psf ----------------------------
 * Reference call site: lightcurver/processes/psf_modelling.py:164-171 (one call per frame inside
 * the serial loop at :92).  Here a whole batch of F frames is fitted at once, one workgroup per
 * frame.  S_max stars per frame; frames with fewer usable stars (the 40 % mask filter at
 * psf_modelling.py:144-153) pass weight == 0 for the padding stamps.
 *
 *   data    [F][S_max][n][n]  stamps, already divided by the caller's normalisation
 *   weight  [F][S_max][n][n]  mask / sigma^2 (0 where masked, NaN or padding)
 *   model per star i of a frame:  a_i * D_ss[ G(x0_i, y0_i) (*) (Moffat + B) ] + sky_i
 */
int lc_psf_supported(int n, int ss); /* 1 if a kernel is instantiated for this stamp size */
int lc_psf_batch_create(lc_ctx *ctx, int F, int S_max, int n, int ss, const float *data,
                        const float *weight, lc_psf_batch **out);
void lc_psf_batch_destroy(lc_psf_batch *b);
/* Moffat parameters [F][4] = fwhm_x, fwhm_y (data px), phi (rad), beta; rasterises the unit-sum
 * Moffat of every frame on the N x N grid (N = ss * n). */
int lc_psf_batch_set_moffat(lc_psf_batch *b, const float *moffat);
int lc_psf_batch_get_moffat(lc_psf_batch *b, float *moffat);
/* per-star parameters [F][S_max][4] = a, x0, y0, sky */
int lc_psf_batch_set_stars(lc_psf_batch *b, const float *stars);
int lc_psf_batch_get_stars(lc_psf_batch *b, float *stars);
/* pixel grid B [F][N*N]; NULL resets it (and the optimiser moments) to zero */
int lc_psf_batch_set_grid(lc_psf_batch *b, const float *grid);
int lc_psf_batch_get_grid(lc_psf_batch *b, float *grid);
/* starlet weights W [F][J][N][N] (J = floor(log2 N) detail scales) and strengths.  W == NULL keeps the weights the
 * batch already holds: the starlet scale norms of a new batch ("lambda is not normalized" case of STARRED), or the
 * maps left by lc_psf_batch_propagate_noise / an earlier call with W != NULL. */
int lc_psf_batch_set_regularization(lc_psf_batch *b, const float *W, float lam_scales, float lam_hf);
/* noise propagation of the chi2 gradient into the starlet domain of B (replaces the
 * propagate_noise call inside build_psf), using the current a, x0, y0.  Writes device W.  A star further than N/4
 * high-resolution pixels from the stamp centre enters pinned there, as in the fit itself (device and host path). */
int lc_psf_batch_propagate_noise(lc_psf_batch *b);
int lc_psf_batch_get_weights(lc_psf_batch *b, float *W);
/* One evaluation at the current parameters.  Any output may be NULL.
 *   loss [F] (0.5 chi2 + l1), chi2 [F], grad_moffat [F][4], grad_stars [F][S_max][4] (a,x0,y0,sky),
 *   grad_grid [F][N*N] (d loss / d B, regularisation included), model [F][S_max][n][n]. */
/* (after lc_psf_batch_set_moffat_q, grad_moffat is d loss / d (q11, q12, q22, beta)) */
int lc_psf_batch_eval(lc_psf_batch *b, float *loss, float *chi2, float *grad_moffat,
                      float *grad_stars, float *grad_grid, float *model);
/* Stage A of build_psf: Moffat + a, x0, y0 by bounded L-BFGS with B = 0 (n_iter_analytic).  One independent problem per
 * frame, optimiser state and two-loop recursion on the device (csrc/psf_lbfgs.h); replaces STARRED's
 * Optimizer(method='l-bfgs-b') inside build_psf (reference call site lightcurver/processes/psf_modelling.py:164-171). */
int lc_psf_batch_fit_moffat(lc_psf_batch *b, int n_iter, float *final_loss /* [F] or NULL */);
/* Stage B: n_iter AdaBelief steps on B, a, x0, y0, state and loop on device (the hot loop).
 * Asynchronous on the context stream.  loss history accumulates across calls. */
int lc_psf_batch_run_adabelief(lc_psf_batch *b, int n_iter, const lc_adabelief_cfg *cfg);
int lc_psf_batch_iterations_done(lc_psf_batch *b);
/* Small batches run the loop with two workgroups per frame that hand their halves of the gradient to each other inside
 * the launch; a launch whose partner workgroups cannot all be resident gives up and is redone by the library itself in
 * the one-workgroup form from the pre-launch state (same bits).  count = how often that happened for this batch. */
int lc_psf_batch_split_fallbacks(lc_psf_batch *b, int *count);
/* loss at theta_0 .. theta_T (T + 1 values per frame; history[f][t] is the loss BEFORE update t,
 * the last entry the loss of the final parameters) */
int lc_psf_batch_get_loss_history(lc_psf_batch *b, float *history, int stride);
/* narrow_psf, full_psf [F][N][N] (unit sum), residuals = data - model [F][S_max][n][n],
 * reduced chi2 [F] over unmasked pixels. */
int lc_psf_batch_get_results(lc_psf_batch *b, float *narrow_psf, float *full_psf, float *residuals,
                             float *chi2);

/* ---- build_psf(field_distortion=True): lightcurver/processes/psf_modelling.py:164-171 with field_distortion and
 * stamp_coordinates.  Star i of a frame sees T_i = Moffat_i + W_i[B] (csrc/psf_distort.h).  Two
 * batches work together: `frames` (F frames; holds B, the starlet term and the AdaBelief state of B) and `stars` (F * S
 * single-star frames, frame-major; holds the stamps, each star's Moffat by its quadratic form, and the AdaBelief state of
 * a, x0, y0).  One iteration = forward (resample B for every star) -> step of `stars` with export_grad -> backward
 * (adjoint resampling summed over the stars) -> step of `frames` with use_ext_grad; everything asynchronous. */
int lc_psf_batch_set_moffat_q(lc_psf_batch *b, const float *q /* [F][4] = q11, q12, q22, beta */);
/* Refused (LC_ERR_INVALID, nothing copied, the batch keeps the distortion it had), checked on the host for every (frame,
 * star): a coefficient that is not finite or outside +-0.25; a coordinate that is not finite; an entry of the star's matrix
 * A further than 0.5 from the identity (the range the adjoint resampling gathers without loss, csrc/psf_distort.h: with
 * |x|, |y| <= 0.5 the coefficient bound keeps the entries inside it, pixel coordinates passed by mistake do not);
 * det A <= 1e-3 (coefficients inside +-0.25 can make A singular).  The message names the frame and the star. */
int lc_psf_batch_set_distortion(lc_psf_batch *frames, int S_stars, const float *coeffs /* [F][9] */,
                                const float *xy /* [F][S_stars][2] rescaled frame coordinates */);
int lc_psf_distortion_forward(lc_psf_batch *frames, lc_psf_batch *stars);
int lc_psf_distortion_backward(lc_psf_batch *frames, lc_psf_batch *stars);
int lc_psf_batch_get_ext_grad(lc_psf_batch *b, float *grad /* [F][N*N] */);
int lc_psf_batch_step_adabelief(lc_psf_batch *b, const lc_adabelief_cfg *cfg, int use_ext_grad, int export_grad);
/* the whole pixel-grid stage in one call: n_iter times { forward; step(stars, export_grad); backward; step(frames,
 * use_ext_grad) } and a final forward, enqueued from C++ */
int lc_psf_distortion_run(lc_psf_batch *frames, lc_psf_batch *stars, int n_iter, const lc_adabelief_cfg *cfg);
/* The batched bounded L-BFGS of the analytic stage with a caller-supplied evaluation (the distortion fit adds nine
 * coefficients per frame to the variables): x, lo, hi [nb][D]; eval fills F [nb] and G [nb][D] for the trial points X. */
int lc_batched_lbfgs(int nb, int D, double *x, const double *lo, const double *hi, int maxiter,
                     int (*eval)(void *user, const double *X, double *F, double *G), void *user,
                     double *f_final /* [nb] or NULL */, int *evaluations /* or NULL */);

/* ---- field distortion of the narrow PSF: replaces starred.psf.psf.apply_distortion ------------
 * Reference call sites: lightcurver/processes/star_photometry.py:291-304, roi_file_preparation.py:169-180
 * (narrow_psf, kwargs_distortion read back from the regions file, rescaled star position).
 *   narrow_psf [N][N]; coeffs [9] = dilation_x (c0, c1, c2), dilation_y (c0, c1, c2), shear (c0, c1, c2), each evaluated
 *   as c0 + c1 x + c2 y; xy [K][2] rescaled frame coordinates of the K positions; out [K][N][N], unit sum each.
 * Host buffers, copied at call time; synchronous.
 * Refused (LC_ERR_INVALID) before anything is copied or launched, `out` untouched: N <= 0, K <= 0, a coefficient or a
 * position that is not finite, det A <= 1e-3 at any position (singular or inverting matrix; the message names it). */
int lc_apply_distortion(lc_ctx *ctx, int N, int K, const float *narrow_psf, const float *coeffs,
                        const float *xy, float *out);

/* ---- joint multi-epoch forward model: replaces starred Deconv / Loss / Optimizer ------------
 * Reference call sites: lightcurver/processes/star_photometry.py:66-137 (one star, all epochs)
 * and lightcurver/processes/roi_modelling.py:213-334 (ROI, M point sources + background).
 *   data, sigma2 [E][n][n];  psf [E][N][N] narrow PSF per epoch;  N = ss * n
 * Parameter blocks follow STARRED's kwargs: a [E*M] epoch-major (roi_modelling.py:462),
 * c_x, c_y [M], dx, dy, alpha [E] (alpha in degrees, never free), h [N*N], mean [E].
 */
enum { LC_P_A = 0, LC_P_CX = 1, LC_P_CY = 2, LC_P_DX = 3, LC_P_DY = 4, LC_P_ALPHA = 5, LC_P_H = 6,
       LC_P_MEAN = 7, LC_P_COUNT = 8 };

typedef struct {
  float lam_scales, lam_hf;  /* regularization_strength_scales / _hf (l1_starlet on h) */
  float lam_positivity;      /* regularization_strength_positivity (h) */
  float lam_positivity_ps;   /* regularization_strength_positivity_ps (a) */
  float lam_pts_source;      /* regularization_strength_pts_source */
  float lam_flux_uniformity; /* regularization_strength_flux_uniformity */
  int32_t n_prior;           /* Gaussian prior terms on c_x / c_y: arrays below, length M each */
  const float *prior_cx_mean, *prior_cx_sigma, *prior_cy_mean, *prior_cy_sigma; /* may be NULL */
} lc_joint_loss_cfg;

int lc_joint_supported(int n, int ss);
/* Diagnostic: when on, objects created afterwards for n = 16 or 32 (ss = 2) use the large-grid kernels
   (spectrum scratch in HBM, multi-block starlet / update) that n = 128 always uses, so that those kernels
   can be checked against the oracle at sizes the oracle finishes in seconds. Not for production use. */
int lc_joint_set_debug_global(int on);
int lc_joint_create(lc_ctx *ctx, int E, int M, int n, int ss, const float *data, const float *sigma2,
                    const float *psf, lc_joint **out);
/* ... with PSF stamps of their own side: psf [E][psf_side][psf_side], any psf_side >= 1 (the reference fits its narrow
 * PSFs at stamp_size_stars and cuts the ROI at stamp_size_ROI, two independent settings: 24 and 32 by default, so
 * 48 x 48 stamps beside a 64 x 64 grid).  A stamp is placed on the N x N grid, N = n * ss, with the zero lags of the
 * 'same' convolution coinciding: tap (a, b) goes to (a + c_N - c_P, b + c_N - c_P), c_S = (S - 1) / 2; taps outside
 * [0, N) are dropped and nothing is renormalised.  For psf_side <= N that is the same linear operator as convolving with
 * the stamp; for psf_side > N the N x N window is all the fit carries (the dropped wings are a declared approximation,
 * DESIGN.md section 7).  lc_joint_create is this call with psf_side = n * ss, bit for bit.  LC_ERR_INVALID for
 * psf_side < 1, LC_ERR_UNSUPPORTED for E * psf_side^2 >= 2^31 or, with psf_side != n * ss, E > 65535; refused before
 * anything is allocated, *out untouched.  The grouped creators below keep psf [sum E_g][N][N]: in the reference a star's
 * PSF and its stamp are both stamp_size_stars. */
int lc_joint_create_psf(lc_ctx *ctx, int E, int M, int n, int ss, int psf_side, const float *data, const float *sigma2,
                        const float *psf /* [E][psf_side][psf_side] */, lc_joint **out);
void lc_joint_destroy(lc_joint *j);
int lc_joint_set_param(lc_joint *j, int which, const float *values, int count);
int lc_joint_get_param(lc_joint *j, int which, float *values, int count);
/* free_mask[LC_P_COUNT]: 1 = optimised, 0 = fixed (ParametersDeconv kwargs_fixed) */
int lc_joint_set_free(lc_joint *j, const int32_t *free_mask);
int lc_joint_set_loss(lc_joint *j, const lc_joint_loss_cfg *cfg, const float *W /* [J][N][N] or NULL */);
/* propagate_noise(method='SLIT', likelihood_type='chi2')[0]  ->  W [J+1][N][N] */
int lc_joint_propagate_noise(lc_joint *j, float *W_out /* may be NULL: keep on device only */);
/* loss and gradient at the current parameters; grads[which] may be NULL.  For L-BFGS drivers. */
int lc_joint_loss_grad(lc_joint *j, float *loss, float *const grads[LC_P_COUNT]);
/* Deconv.model(kwargs) -> [E][n][n];  chi2_per_epoch [E] = sum res^2/sigma2 (not normalised) */
int lc_joint_model(lc_joint *j, float *model, float *chi2_per_epoch);
/* Deconv.getDeconvolved(kwargs, epoch) -> high-res scene and background, [N][N] each */
int lc_joint_deconvolved(lc_joint *j, int epoch, float *scene, float *background);
int lc_joint_run_adabelief(lc_joint *j, int n_iter, const lc_adabelief_cfg *cfg);
/* Optimizer(method='l-bfgs-b').minimize(maxiter=...) (roi_modelling.py:278-280, starred_utilities.py:33-34): bounded
 * L-BFGS on the free blocks with parameters, gradients, direction and (s, y) history on the device; the host reads a few
 * scalars per trial point.  lower / upper: per block, length of the block, or NULL (unbounded); may be NULL altogether.
 * loss_history[i] = loss after accepted iteration i (up to history_capacity entries). */
int lc_joint_run_lbfgs(lc_joint *j, int maxiter, const float *const lower[LC_P_COUNT],
                       const float *const upper[LC_P_COUNT], float *loss_history, int history_capacity,
                       int *n_iterations, int *n_evaluations);
int lc_joint_get_loss_history(lc_joint *j, float *history, int count);
int lc_joint_iterations_done(lc_joint *j);
/* Few epochs per GPU (a rank's share of a sharded fit; the reference keeps all epochs on one device,
 * lightcurver/processes/roi_modelling.py:154-160,213, and has no counterpart): inside lc_joint_run_adabelief /
 * lc_joint_run_sharded the epoch kernel of a 64 x 64 fit runs as a CLUSTER launch - several workgroups per epoch in one
 * launch, phases separated by arrival counters in device memory - when all of them are resident together.  Every wait is
 * bounded; a run in which one gave up is redone by the library with one workgroup per epoch (lc_joint_run_adabelief) or
 * reported (lc_joint_run_sharded), and the object keeps the one-workgroup kernel afterwards.  parts_last: workgroups per epoch
 * of the most recent epoch launch (0 = one-workgroup kernel); fallbacks: runs in which a wait gave up.  LCMI_CLUSTER=0
 * switches the form off, LCMI_CLUSTER=<P> forces the count. */
int lc_joint_cluster_info(lc_joint *j, int *parts_last, int *fallbacks);
/* Optimizer.minimize(..., return_param_history=True) - what the reference's own call sites pass
 * (lightcurver/processes/star_photometry.py:115-122, roi_modelling.py:326-334).  begin: from now on every AdaBelief update
 * also stores the free parameter blocks (in block order a, c_x, c_y, dx, dy, h, mean; *n_params = their total length) into
 * a device-resident history of `capacity` rows, so the loop of lc_joint_run_adabelief stays on the device; updates past
 * the capacity are not recorded.  get: rows [first, first + count) -> out [count][n_params] (one D2H copy, whenever the
 * caller first looks at the history).  end: releases the buffer (also done by begin, set_free and destroy). */
int lc_joint_param_history_begin(lc_joint *j, int capacity, int *n_params);
int lc_joint_param_history_rows(lc_joint *j);
int lc_joint_param_history_get(lc_joint *j, int first, int count, float *out);
int lc_joint_param_history_end(lc_joint *j);
/* Batched star photometry.  The reference fits its reference stars one after the other (the loop at
 * lightcurver/processes/star_photometry.py:257 over do_one_star_forward_modelling, :23-151): G independent joint fits
 * without a background, each over its own epochs.  Here they are ONE object: star g owns epochs_per_group[g] consecutive
 * epochs of data / sigma2 / psf ([sum E_g][..]), M point sources with its own c_x, c_y (parameter blocks c_x, c_y have
 * G * M entries, star-major; a, dx, dy, mean follow the epochs), and every AdaBelief iteration is one kernel pair for all
 * stars (grid over (star, epoch), then one block per star for its reduction and update).  Each star's trajectory is bit
 * for bit that of lc_joint_create + lc_joint_run_adabelief on that star alone.  h and alpha stay fixed; no weight cube,
 * prior or point-source starlet term.  set/get_param, set_free, set_loss, run_adabelief, model, fisher_flux_sigma,
 * deconvolved (epoch counted over the epochs of all stars; the positions of its star) and iterations_done work as on a
 * plain object; the loss history is per star. */
int lc_joint_create_groups(lc_ctx *ctx, int G, const int32_t *epochs_per_group, int M, int n, int ss, const float *data,
                           const float *sigma2, const float *psf, lc_joint **out);
int lc_joint_get_group_loss_history(lc_joint *j, float *history /* [G][count_per_group] */, int count_per_group);
/* ... with a background grid per star (the reference's do_one_star_forward_modelling with starlet_global_background=True,
 * its own default: star_photometry.py:23-24, and the pipeline's switch for crowded fields).  Same arguments and the same
 * object as lc_joint_create_groups, plus every star's own background: block h has G * N * N entries, star-major
 * (set/get_param, set_free); lc_joint_set_loss takes W as [G][J][N][N]; lc_joint_propagate_noise writes [G][J + 1][N][N]
 * (each star's levels from its own epochs); model, fisher_flux_sigma and deconvolved use each epoch's own star's h.
 * lc_joint_run_adabelief needs h free with the starlet / positivity regulariser on (LC_ERR_UNSUPPORTED otherwise).  Each
 * star's trajectory is bit for bit that of lc_joint_create + lc_joint_run_adabelief on that star alone with h free.  No
 * point-source starlet term or prior; loss_grad, the step / sharded entry points, L-BFGS and the parameter history return
 * LC_ERR_UNSUPPORTED.  Stamp sizes with a single-workgroup update only (n = 16, 24, 32 at ss = 2, n = 16 at ss = 1);
 * LC_ERR_UNSUPPORTED at create otherwise; lc_joint_groups_background_supported(n, ss) answers (1 / 0) without a device. */
int lc_joint_groups_background_supported(int n, int ss);
int lc_joint_create_groups_background(lc_ctx *ctx, int G, const int32_t *epochs_per_group, int M, int n, int ss,
                                      const float *data, const float *sigma2, const float *psf, lc_joint **out);
/* FisherCovariance(diagonal_only=True) with only `a` free -> sigma(a) [E*M]
 * (lightcurver/utilities/starred_utilities.py:36-38). */
int lc_joint_fisher_flux_sigma(lc_joint *j, float *sigma_a);
/* FisherCovariance(diagonal_only=False) with only `a` free: the full Fisher information of the fluxes.  The model is linear
 * in a, so it is the exact Hessian of 1/2 chi2 (no regulariser: the flux-uniformity term would couple the epochs), independent
 * of a and block diagonal over the epochs: F_e[i][j] = sum_pix w T_{e,i} T_{e,j} with T_{e,i} the unit-flux model of source i
 * in epoch e.  Writes fisher = F and cov = F^-1 [E][M][M] and the marginal sigma = sqrt(diag cov) [E][M], epoch-major like a;
 * each pointer may be null.  A source with F_ii = 0 (outside the stamp, or masked) has sigma = +inf and a zero row and column
 * of cov, the rest of its epoch's block is solved without it; an epoch whose block is numerically singular (a Cholesky pivot
 * not above 1e-6 times its diagonal entry) has NaN cov and sigma, the call still succeeds.  Same scope as
 * lc_joint_fisher_flux_sigma (batched star photometry: every epoch with its own star), whose 1 / sqrt(F_ii) it matches. */
int lc_joint_fisher_flux_cov(lc_joint *j, float *fisher, float *cov, float *sigma);
/* Fisher information with the source positions free: theta = (a [E * M], c_x [M], c_y [M], optionally mean [E]), everything
 * else (dx, dy, alpha, h) fixed at its current value - the result is conditional on the registration and the background.
 * F = J^T diag(1 / sigma^2) J (Gauss-Newton, independent of the data) is an arrowhead: per-epoch local blocks F_local
 * (a_e, then mean_e), one shared block F_shared (c_x, then c_y; summed over the epochs in epoch order) and the couplings
 * F_cross.  The C outputs are the blocks of F^-1 (Schur complement in float64): marginal covariances.  LC_FISHER_PRIOR adds
 * 1 / sigma_p^2 of the Gaussian prior last given to lc_joint_set_loss to the diagonal of F_shared; no other regulariser
 * enters.  A parameter whose diagonal entry is zero (prior included) is left out: sigma = +inf, zero rows and columns of C.
 * A Cholesky pivot of any local block or of the Schur complement that is not above 1e-6 times its diagonal entry makes every
 * C and sigma output NaN (F stays as computed, the call returns LC_OK).  Without LC_FISHER_POSITIONS the call is the flux
 * (+ mean) covariance and the shared outputs must be NULL; sigma_mean must be NULL without LC_FISHER_MEAN; LC_FISHER_PRIOR
 * needs LC_FISHER_POSITIONS (LC_ERR_INVALID).  LC_ERR_UNSUPPORTED: a batched star-photometry object; LC_FISHER_PRIOR when
 * the loss has no prior.  Every refusal happens before a launch, outputs untouched. */
#define LC_FISHER_POSITIONS 1   /* c_x, c_y free (both or neither) */
#define LC_FISHER_MEAN      2   /* mean_e free */
#define LC_FISHER_PRIOR     4   /* add the loss's Gaussian prior on c_x, c_y to F_shared */
typedef struct {                /* every pointer may be NULL; Lp = M + (flags & LC_FISHER_MEAN ? 1 : 0) */
  float *F_local, *F_cross, *F_shared;   /* [E][Lp][Lp], [E][Lp][2M], [2M][2M] */
  float *C_local, *C_cross, *C_shared;   /* same shapes: marginal covariances */
  float *sigma_a, *sigma_mean, *sigma_c; /* [E*M], [E], [2M] */
} lc_fisher_positions_out;
int lc_joint_fisher_positions(lc_joint *j, int flags, const lc_fisher_positions_out *out);
/* Fisher information with the epochs' translations free: theta = (a [E * M], dx [E], dy [E], optionally mean [E] and c_x,
 * c_y [M each]); alpha and h stay fixed.  The same arrowhead as lc_joint_fisher_positions with two more local parameters per
 * epoch: the local block is ordered a_e (M), mean_e (0 / 1), dx_e, dy_e.  The columns of dx_e, dy_e hold the point sources
 * (ss sum_i df/dX_i, df/dY_i) and the resampled background (the derivative of the bilinear resampling in the cell floor
 * selects, clamped at the edge, as in the gradient of the loss), convolved with the epoch's PSF; the background pass runs
 * whenever the object holds a background, whatever its values.  The flags are those of lc_joint_fisher_positions, the shifts
 * are always free; the prior, the zero-diagonal rule, the 1e-6 pivot rule and the NaN outcome carry over.  Refusals as there
 * (LC_ERR_INVALID: unknown flags, shared outputs without LC_FISHER_POSITIONS, sigma_mean without LC_FISHER_MEAN,
 * LC_FISHER_PRIOR without LC_FISHER_POSITIONS; LC_ERR_UNSUPPORTED: a batched star-photometry object, LC_FISHER_PRIOR when
 * the loss has no prior), and LC_ERR_UNSUPPORTED for LC_FISHER_POSITIONS without LC_FISHER_PRIOR: a common translation of
 * all sources is a translation of every epoch, a gauge of the shifts, so with both free the information is exactly singular
 * unless a background or a prior pins the frame - the call asks for the prior instead of leaving that to a pivot test on a
 * float32 matrix.  Every refusal happens before a launch, outputs untouched. */
typedef struct {  /* every pointer may be NULL; Lp = M + (flags & LC_FISHER_MEAN ? 1 : 0) + 2; local order a_e, mean_e, dx_e, dy_e */
  float *F_local, *F_cross, *F_shared, *C_local, *C_cross, *C_shared;  /* [E][Lp][Lp], [E][Lp][2M], [2M][2M], twice */
  float *sigma_a, *sigma_mean, *sigma_c, *sigma_dx, *sigma_dy;        /* [E*M], [E], [2M], [E], [E] */
} lc_fisher_shifts_out;
int lc_joint_fisher_shifts(lc_joint *j, int flags, const lc_fisher_shifts_out *out);
/* ... of a batched star-photometry object (lc_joint_create_groups, lc_joint_create_groups_background), every star in one
 * call: theta = (a [sum E_g * M], dx, dy [sum E_g], optionally mean [sum E_g]); every star's c_x, c_y stay fixed (the gauge of
 * that star's shifts), alpha and h too.  With the positions fixed the information is block diagonal over the epochs: the
 * local block of an epoch is that of lc_joint_fisher_shifts (a_e, mean_e, dx_e, dy_e; Lp = M + mean + 2), computed with its
 * own star's positions and, in a batch with backgrounds, its own star's h - bit for bit what lc_joint_fisher_shifts gives
 * for a plain object over that star's epochs and parameters (for a batch without a background: one holding h = 0).  Outputs
 * in the order the batch concatenates its stars, every pointer may be NULL; the shared outputs (F_cross, F_shared, C_cross,
 * C_shared, sigma_c) must be NULL and sigma_mean needs LC_FISHER_MEAN (LC_ERR_INVALID, as unknown flags).  LC_FISHER_MEAN
 * is the only flag: LC_FISHER_POSITIONS and LC_FISHER_PRIOR are LC_ERR_UNSUPPORTED (a batched object holds no prior, and
 * without one the positions beside the shifts are singular), as is an object that is not batched (use
 * lc_joint_fisher_shifts).  Every refusal happens before a launch, outputs untouched.  The zero-diagonal rule is per
 * parameter as before; the pivot rule is per STAR: a pivot not above 1e-6 times its diagonal entry in any epoch of star g
 * makes the C and sigma outputs of all of star g's epochs NaN and star_ok[g] = 0 (else 1; star_ok [G] may be NULL), and
 * touches no other star; F stays as computed and the call returns LC_OK. */
int lc_joint_groups_fisher_shifts(lc_joint *j, int flags, const lc_fisher_shifts_out *out, int32_t *star_ok);
/* Multi-GPU epoch sharding: split one optimiser step around the caller's all-reduce of the shared block
 * [dL/dh (N*N) | dL/dc_x (M) | dL/dc_y (M) | sum_e (a - ref) (M) | sum_e (a - ref)^2 (M) | chi2 | n_epochs]
 * living in device memory.  The flux moments (flux-uniformity term, jnp.std over epochs in the reference:
 * roi_modelling.py:273-276) are centred on one reference flux per source so that the variance does not cancel in
 * fp32; lc_joint_set_param(LC_P_A) sets it to the mean of the local fluxes, a sharded fit must give every rank the
 * same reference (lightcurver_amd/distributed.py does) with lc_joint_set_flux_reference. */
int lc_joint_set_flux_reference(lc_joint *j, const float *ref, int count /* = M */);
int lc_joint_get_flux_reference(lc_joint *j, float *ref, int count /* = M */);
int lc_joint_step_local(lc_joint *j);                      /* forward/backward of local epochs */
int lc_joint_shared_buffer_dev(lc_joint *j, void **dev_ptr, int *count);
int lc_joint_step_update(lc_joint *j, const lc_adabelief_cfg *cfg); /* regularise + AdaBelief */
/* The gradient-only counterpart of lc_joint_step_update (the sharded L-BFGS stage: roi_modelling.py:278-280 with the epochs
 * spread over ranks): behind lc_joint_step_local and the all-reduce of the shared block it returns the loss of the WHOLE fit
 * and the gradients - those of the shared parameters complete, those of the per-epoch parameters for the local epochs -
 * without stepping anything.  grads as in lc_joint_loss_grad. */
int lc_joint_step_grad(lc_joint *j, float *loss, float *const grads[LC_P_COUNT]);
/* host-staged access to the shared block (gloo / CPU collectives: D2H, all-reduce, H2D) */
int lc_joint_shared_get(lc_joint *j, float *host, int count);
int lc_joint_shared_set(lc_joint *j, const float *host, int count);
/* The sharded loop without the host language in it: n_iter times { lc_joint_step_local; allreduce(user, block, count,
 * stream); lc_joint_step_update }, enqueued from C++.  `allreduce` must sum-all-reduce the `count` floats at `dev_buf`
 * over the ranks in place, ordered on `hip_stream` (= lc_ctx_stream: e.g. ncclAllReduce enqueued there, or
 * lc_peer_allreduce below with user = the peer group), and return 0.  Every rank must have agreed on the flux reference
 * (lc_joint_set_flux_reference) beforehand. */
typedef int (*lc_allreduce_fn)(void *user, void *dev_buf, int count, void *hip_stream);
int lc_joint_run_sharded(lc_joint *j, int n_iter, const lc_adabelief_cfg *cfg, lc_allreduce_fn allreduce, void *user);

/* ---- peer group: one-shot all-reduce of the shared block through peer memory (xGMI, one hop) -------------------------------
 * The block is 64 - 256 KiB and latency bound: every rank publishes it in an exchange buffer that the others map with HIP
 * IPC, reads the N - 1 peers directly and adds in rank order (the same bits on every rank).  csrc/peer.hip.
 *   create   count = lc_joint_shared_buffer_dev's count; rank / world of this process
 *   export   this rank's IPC handle (64 bytes used of handle_bytes) - the caller carries the handles between the processes
 *            (e.g. torch.distributed.all_gather_object)
 *   connect  handles [world][handle_bytes], own entry ignored
 *   lc_peer_allreduce   has the signature of lc_allreduce_fn with user = the group; all ranks must call it equally often
 *   status   LC_ERR_DEVICE if a rank did not show up within ~2 s in some call (the kernels never wait longer) */
typedef struct lc_peer_group lc_peer_group;
int lc_peer_group_create(lc_ctx *ctx, int count, int rank, int world, lc_peer_group **out);
int lc_peer_group_export(lc_peer_group *g, void *handle_out, int handle_bytes);
int lc_peer_group_connect(lc_peer_group *g, const void *handles, int handle_bytes);
int lc_peer_allreduce(void *group, void *dev_buf, int count, void *hip_stream);
int lc_peer_group_status(lc_peer_group *g);
void lc_peer_group_destroy(lc_peer_group *g);

/* RCCL group: the same all-reduce by RCCL, from the library's own loop ("RCCL all-reduce over xGMI only for the
 * shared-background gradient in the joint fit", BASELINE.json north_star; the reference keeps all epochs on one device,
 * lightcurver/processes/roi_modelling.py:154-160,213, and has no counterpart).  The library loads librccl at run time (it
 * does not link against it; a copy the process already carries - torch's - is shared) and owns the communicator:
 *   lc_rccl_available   1 when librccl could be loaded
 *   lc_rccl_unique_id   rank 0: a fresh ncclUniqueId (id_bytes >= 128), which the caller hands to every rank over any
 *                       channel it has (a torch.distributed broadcast, MPI, a file)
 *   lc_rccl_group_create  every rank, collectively: ncclCommInitRank on the context's device
 *   lc_rccl_allreduce   has the signature of lc_allreduce_fn with user = the group: ncclAllReduce (float32, sum) in place
 *                       on the given stream, enqueued, never synchronised - pass it to lc_joint_run_sharded and no host
 *                       code runs inside the loop
 *   lc_rccl_group_info  rank, size, all-reduces enqueued so far (each may be NULL) */
typedef struct lc_rccl_group lc_rccl_group;
int lc_rccl_available(void);
int lc_rccl_unique_id(void *id_out, int id_bytes);
int lc_rccl_group_create(lc_ctx *ctx, const void *unique_id, int id_bytes, int rank, int world, lc_rccl_group **out);
int lc_rccl_allreduce(void *group, void *dev_buf, int count, void *hip_stream);
int lc_rccl_group_info(lc_rccl_group *g, int *rank, int *world, long long *calls);
void lc_rccl_group_destroy(lc_rccl_group *g);

#ifdef __cplusplus
}
#endif
#endif /* LCMI_H */
