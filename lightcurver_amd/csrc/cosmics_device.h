// The cosmic-ray kernel with device pointers: what lc_detect_cosmics (cosmics.hip) runs between its copies, and what
// lc_mask_cutouts (ccdmask.hip) runs on the stack it has already uploaded.
#pragma once
#include "lc_common.h"

namespace lc {

// stamp size and settings of a call: LC_OK, or the error code with ctx->err set ("<who>: ...")
int cosmics_check(lc_ctx *ctx, const char *who, int n, const lc_cosmics_cfg *cfg);

// bytes of global planes the launch needs (n above the LDS limit), 0 when the planes live in LDS
size_t cosmics_scratch_bytes(const lc_ctx *ctx, int K, int n);

// one launch on ctx->stream over K stamps; every pointer is a device pointer, invar / inmask / clean / iters may be
// null, scratch holds cosmics_scratch_bytes (null when that is 0)
hipError_t cosmics_launch(lc_ctx *ctx, int K, int n, const float *data, const float *invar, const uint8_t *inmask,
                          const lc_cosmics_cfg *cfg, uint8_t *crmask, float *clean, int32_t *iters, float *scratch);

}  // namespace lc
