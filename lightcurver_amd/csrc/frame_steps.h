// The whole-frame steps as launches on device pointers: what lc_background_frames (background.hip) and lc_extract_frames
// (extract.hip) run between their uploads and downloads, so that lc_import_frames can chain them on one uploaded frame.
// Every function enqueues on ctx->stream and returns without synchronising; the buffers belong to the caller.
#pragma once
#include <vector>

#include "device_call.h"
#include "lc_common.h"

namespace lc {

// ---- sky background (background.hip) -----------------------------------------------------------------------------

struct BackgroundBuffers {
  const float *data = nullptr;      // [K][h][w]
  const uint8_t *mask = nullptr;    // [K][h][w], nullable
  const double *cfac = nullptr;     // background_pivots()
  float *sub = nullptr, *back = nullptr;            // [K][h][w], nullable
  float *mesh_back = nullptr, *mesh_rms = nullptr;  // [K][ny][nx]
  float *globalback = nullptr, *globalrms = nullptr;  // [K]
  int32_t *status = nullptr;                          // [K], nullable
  float *raw_back = nullptr, *raw_rms = nullptr, *zy = nullptr;  // [K][ny][nx] scratch
};

// the pivots of the splines' Thomas sweep, the same for every call
std::vector<double> background_pivots();
// meshes of one frame, 0 if (h, w, bw, bh) is no grid
size_t background_meshes(int h, int w, int bw, int bh);
// K frames go into one grid (lc_background_supported answers for the frame alone)
bool background_batch_fits(int K, int h, int w, int bw, int bh);
// the three launches of lc_background_frames; the arguments have been checked
hipError_t background_launch(lc_ctx *ctx, int K, int h, int w, const lc_background_cfg *cfg, const BackgroundBuffers &B);

// ---- source extraction (extract.hip) -----------------------------------------------------------------------------

struct ExtractBuffers {
  const float *data = nullptr;        // [K][h][w]
  const float *var = nullptr;         // [K][h][w], or null:
  const float *var_scalar = nullptr;  // [K]
  lc_extract_object *objects = nullptr;  // [K][max_objects], nullable
  int32_t *nobj = nullptr;               // [K]
  int32_t *segmap = nullptr;             // [K][h][w], nullable
  uint8_t *mask = nullptr;               // [K][h][w], nullable
  int32_t *status = nullptr;             // [K]
  // scratch: extract_scratch() fills these
  float *snr = nullptr;                          // [K][h][w]
  int32_t *label = nullptr, *count = nullptr;    // [K][h][w]
  int32_t *block = nullptr;                      // [K][blocks of 256 pixels]
  int32_t *aux = nullptr;                        // [K][max_objects][6]: first, npix, xmin, xmax, ymin, ymax
};

// K frames of h x w go into the grids of the extraction
bool extract_batch_fits(int K, int h, int w);
// allocates the scratch buffers of one extraction from the call's pool (aux only with objects)
hipError_t extract_scratch(DeviceCall &call, int K, int h, int w, int max_objects, bool with_objects, ExtractBuffers *B);
// every launch of lc_extract_frames; the arguments have been checked
hipError_t extract_launch(lc_ctx *ctx, int K, int h, int w, const lc_extract_cfg *cfg, int max_objects,
                          const ExtractBuffers &B);
// Its launches in three parts, which the de-blended extraction (deblend.hip) runs more than once on planes it rewrote:
//   label: count and status zeroed, then snr, the label plane of roots and count[root] = pixels of the component;
//   count: nobj [K] = the roots with count >= minarea (status 1 where nobj > max_objects);
//   table: count[root] becomes the object number, aux (where not null), segmap, mask, and objects (where not null).
hipError_t extract_label_launch(lc_ctx *ctx, int K, int h, int w, const lc_extract_cfg *cfg, const ExtractBuffers &B);
hipError_t extract_count_launch(lc_ctx *ctx, int K, int h, int w, int minarea, int max_objects, const ExtractBuffers &B);
hipError_t extract_table_launch(lc_ctx *ctx, int K, int h, int w, int minarea, int max_objects, const ExtractBuffers &B);
// what is wrong with the settings, or null
const char *extract_cfg_error(const lc_extract_cfg *cfg);

// ---- de-blending and cleaning of frame objects (deblend.hip) --------------------------------------------------------

// what is wrong with the settings (*code: the error code), or null
const char *deblend_cfg_error(const lc_deblend_cfg *dcfg, int *code);
// Every launch of lc_extract_frames_deblended; the arguments have been checked.  Unlike extract_launch it waits for the
// stream twice, to size the tables of the parents and of the final objects from their counts, and takes those tables
// from the call's pool.
hipError_t deblend_launch(lc_ctx *ctx, DeviceCall &call, int K, int h, int w, const lc_extract_cfg *cfg,
                          const lc_deblend_cfg *dcfg, int max_objects, const ExtractBuffers &B);

// ---- the import of frames (extract.hip): what lc_import_frames and lc_frames_import (cutout.hip) both run ------------

struct ImportBuffers {
  BackgroundBuffers G;  // data: the frames; sub, mesh_back, mesh_rms, globalback, globalrms are outputs of the import
  ExtractBuffers B;     // objects, nobj, segmap (nullable), status are outputs; data and var are set by the launch
  const float *exptime = nullptr;  // [K]
  float *var = nullptr;            // [K][h][w] scratch
  // scratch of mask_sources_first
  uint8_t *mask = nullptr;                        // [K][h][w]
  float *v0 = nullptr;                            // [K]
  int32_t *mstatus = nullptr, *mnobj = nullptr;   // [K]
  // the catalogue de-blended and cleaned (null: not), with the call that owns its tables
  const lc_deblend_cfg *dcfg = nullptr;
  DeviceCall *call = nullptr;
};

// The arguments of an import that both entries share: LC_OK, or the error code with ctx->err set ("<who>: ...").
// pointers_ok: the entry's own test of the pointers it needs, reported with the other invalid arguments.
int import_check(lc_ctx *ctx, const char *who, bool pointers_ok, int K, int h, int w, const float *exptime,
                 const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg, int mask_sources_first,
                 const lc_extract_cfg *mcfg, int max_objects);
// every launch of lc_import_frames; the arguments have been checked
hipError_t import_launch(lc_ctx *ctx, int K, int h, int w, const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg,
                         int mask_sources_first, const lc_extract_cfg *mcfg, int max_objects, ImportBuffers &I);

}  // namespace lc
