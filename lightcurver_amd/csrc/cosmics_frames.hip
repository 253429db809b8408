// Cosmic-ray detection on whole frames: the L.A.Cosmic SPEC of DESIGN.md §5 "Cosmic-ray detection" with "the stamp" read
// as the frame of h x w pixels (DESIGN.md §5 "Cosmic rays of whole frames").  Separable medians only (sepmed = 1).  Every
// float32 operation is the SPEC's, in its order, so the result is bit for bit that of tests/_lacosmic.py on the whole
// frame, whatever the tiling and the chunking.
//
// The planes of a chunk of frames (C, N with a variance, M, CR) live in global scratch between the launches:
//   prep     per tile: counts, noise and mask of step 0, the saturation mask of step 1 (needs C within 5 pixels)
//   detect   per iteration and tile: steps 2a - 2g on a 48 x 48 tile with its 8-pixel halo, 64 x 64 pixels in LDS (six
//            float and three byte planes, 108 KiB); ORs g2 into CR and reports per frame whether a tile found a pixel
//   clean    step 2h in place: a pixel of CR is written, only pixels outside CR are read, so no second buffer is
//            needed; a pixel without a good neighbour is marked 2 in CR and the frame's need word is set
//   select   for the frames that need it: the lower median of the frame's good pixels by a four-pass byte radix select
//            on the order-preserving integer image of the floats (integer histograms: exact and deterministic)
//   fixup    writes that value to the marked pixels
//   step     per frame: iters, the early exit, the control words of the next iteration
//   finish   crmask, clean = C / gain, the count of flagged pixels, and what `apply` asks for on the resident planes
// Every kernel of an iteration reads the frame's control words and leaves at once for a frame that has stopped, so
// the host reads back one word per iteration: the number of frames still running.
#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "cosmics_device.h"
#include "cosmics_frames_device.h"
#include "device_call.h"
#include "frames_state.h"
#include "lacosmic_steps.h"
#include "lc_common.h"
#include "noise_pixel.h"
#include "order_stats.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kCfThreads = 1024;               // the tile kernels: 4 pixels of the region per lane and pass
constexpr int kCfTile = 48, kCfHalo = 8;       // detection needs C, M, N within 8 pixels of the tile
constexpr int kCfR = kCfTile + 2 * kCfHalo;    // 64: the region's side
constexpr int kCfNp = kCfR * kCfR;
constexpr int kCfFloatPlanes = 6, kCfBytePlanes = 3;
constexpr size_t kCfLdsBytes = (size_t)kCfNp * (4 * kCfFloatPlanes + kCfBytePlanes);  // 110592
constexpr int kCfPixThreads = 256;             // the per-pixel kernels
constexpr int kCfPixBlocks = 2048;             // of a frame at the most; a larger frame strides
constexpr int kCfMinSide = 8;
constexpr size_t kCfScratchBytes = (size_t)128 << 20;
constexpr int kCfMaxChunk = 65535;             // gridDim.y

// control words of a frame
enum { kStFound = 0, kStNeed, kStRunning, kStIters, kStPrefix, kStRank, kStFallback, kStWords };

struct CfArgs {
  int h, w, ntx, it;
  int have_var;  // a variance is given: invar, or exptime and rms
  size_t hw;
  const float *data;
  const int32_t *frame;
  const float *invar, *exptime, *rms;
  const uint8_t *inmask;
  float *C, *N;
  uint8_t *M, *CR;
  int32_t *state;
  uint32_t *hist;
  int32_t *running;
  uint8_t *crmask;
  float *clean;
  int32_t *iters, *n_flagged;
  float *planes;
  int apply, pass;
  float gain, gain2;    // gain, gain * gain
  float rn2, vhole;     // readnoise^2, 1e-5 + readnoise^2 (the variance the NaN rule gives a hole)
  float satg, satg10;   // gain * satlevel, (gain * satlevel) / 10
  float sigclip, sigcliplow, objlim;  // sigcliplow = sigfrac * sigclip
};

// the region of a workgroup (lacosmic_steps.h): LDS pixel (ly, lx) is frame pixel (oy + ly, ox + lx)
using CfTile = LaRegion;

// Y = the separable K median of X over the region (T1 is the row pass's output)
template <int K>
__device__ __forceinline__ void cf_median(const float *X, float *T1, float *Y, const CfTile &T) {
  la_sep_median<K, kCfThreads>(X, T1, Y, kCfR, T);
}

__device__ __forceinline__ CfTile cf_tile(const CfArgs &A) {
  const int ty = blockIdx.x / A.ntx, tx = blockIdx.x - ty * A.ntx;
  return CfTile{ty * kCfTile - kCfHalo, tx * kCfTile - kCfHalo, A.h, A.w};
}

// step 0 at pixel q of slot k: counts, noise (with a variance) and mask
__device__ __forceinline__ void cf_input(const CfArgs &A, int k, size_t q, float *c_out, float *n_out, bool *m_out) {
  const int plane = A.frame ? A.frame[k] : k;
  const float d = A.data[(size_t)plane * A.hw + q];
  float iv = 0.f;
  if (A.invar) {
    iv = A.invar[(size_t)k * A.hw + q];
  } else if (A.have_var) {
    const float t = A.exptime[plane];
    const float e = noise_from_rms(d, t, noise_trms2(t, A.rms[plane]));
    iv = e * e;
  }
  la_input(d, A.have_var, iv, A.inmask && A.inmask[(size_t)k * A.hw + q] != 0, A.gain, A.gain2, A.vhole, c_out, n_out,
           m_out);
}

// steps 0 and 1 of a tile; grid (tiles, frames of the chunk)
__global__ __launch_bounds__(kCfThreads) void cf_prep_kernel(CfArgs A) {
  extern __shared__ __align__(16) float cf_lds[];
  const int k = blockIdx.y, tid = threadIdx.x;
  const CfTile T = cf_tile(A);
  float *C = cf_lds, *Np = C + kCfNp, *T1 = Np + kCfNp, *T2 = T1 + kCfNp;
  uint8_t *M = (uint8_t *)(cf_lds + kCfFloatPlanes * kCfNp), *B1 = M + kCfNp, *B2 = B1 + kCfNp;
  for (int p = tid; p < kCfNp; p += kCfThreads) {
    const int ly = p / kCfR, lx = p - ly * kCfR;
    float c = 0.f, nz = 1.f;
    bool m = true;
    if (T.inside(ly, lx)) cf_input(A, k, (size_t)(T.oy + ly) * A.w + (T.ox + lx), &c, &nz, &m);
    C[p] = c;
    Np[p] = nz;
    M[p] = m ? 1 : 0;
  }
  __syncthreads();
  cf_median<7>(C, T1, T2, T);
  for (int p = tid; p < kCfNp; p += kCfThreads) {
    const int ly = p / kCfR, lx = p - ly * kCfR;
    B1[p] = (T.inside(ly, lx) && C[p] >= A.satg && T2[p] > A.satg10) ? 1 : 0;
  }
  __syncthreads();
  for (int p = tid; p < kCfNp; p += kCfThreads) {
    const int ly = p / kCfR, lx = p - ly * kCfR;
    B2[p] = (T.inside(ly, lx) && la_dil3(B1, ly, lx, kCfR)) ? 1 : 0;
  }
  __syncthreads();
  const size_t base = (size_t)k * A.hw;
  for (int p = tid; p < kCfTile * kCfTile; p += kCfThreads) {
    const int ly = kCfHalo + p / kCfTile, lx = kCfHalo + p % kCfTile;
    if (!T.inside(ly, lx)) continue;
    const int r = ly * kCfR + lx;
    const size_t q = base + (size_t)(T.oy + ly) * A.w + (T.ox + lx);
    A.C[q] = C[r];
    if (A.have_var) A.N[q] = Np[r];
    A.M[q] = (M[r] || la_dil3(B2, ly, lx, kCfR)) ? 1 : 0;
    A.CR[q] = 0;
  }
}

// steps 2a - 2g of a tile; grid (tiles, frames of the chunk)
__global__ __launch_bounds__(kCfThreads) void cf_detect_kernel(CfArgs A) {
  extern __shared__ __align__(16) float cf_lds[];
  const int k = blockIdx.y, tid = threadIdx.x;
  int32_t *st = A.state + (size_t)k * kStWords;
  if (!st[kStRunning]) return;
  const CfTile T = cf_tile(A);
  float *C = cf_lds, *Np = C + kCfNp, *S = Np + kCfNp, *T1 = S + kCfNp, *T2 = T1 + kCfNp, *Fp = T2 + kCfNp;
  uint8_t *M = (uint8_t *)(cf_lds + kCfFloatPlanes * kCfNp), *B1 = M + kCfNp, *B2 = B1 + kCfNp;
  const size_t base = (size_t)k * A.hw;
  for (int p = tid; p < kCfNp; p += kCfThreads) {
    const int ly = p / kCfR, lx = p - ly * kCfR;
    float c = 0.f, nz = 1.f;
    uint8_t m = 1;
    if (T.inside(ly, lx)) {
      const size_t q = base + (size_t)(T.oy + ly) * A.w + (T.ox + lx);
      c = A.C[q];
      m = A.M[q];
      if (A.have_var) nz = A.N[q];
    }
    C[p] = c;
    Np[p] = nz;
    M[p] = m;
  }
  __syncthreads();
  // b: noise model without a variance
  if (!A.have_var) {
    cf_median<7>(C, T1, T2, T);
    for (int p = tid; p < kCfNp; p += kCfThreads) Np[p] = sqrtf(fmaxf(T2[p], 1e-5f) + A.rn2);
    __syncthreads();
  }
  // a, c: S = L / (2 N), SP = S - m5(S)
  for (int p = tid; p < kCfNp; p += kCfThreads) {
    const int ly = p / kCfR, lx = p - ly * kCfR;
    S[p] = la_laplace(C, ly, lx, kCfR, T) / (2.0f * Np[p]);
  }
  __syncthreads();
  cf_median<7>(S, T1, T2, T);
  for (int p = tid; p < kCfNp; p += kCfThreads) S[p] = S[p] - T2[p];
  // d: fine structure F = max((m3 - m7(m3)) / N, 0.01)
  cf_median<5>(C, T1, Fp, T);
  cf_median<9>(Fp, T1, T2, T);
  for (int p = tid; p < kCfNp; p += kCfThreads) Fp[p] = fmaxf((Fp[p] - T2[p]) / Np[p], 0.01f);
  __syncthreads();
  // e, f: candidates and their growth (M is 1 outside the frame, so B1 and B2 are 0 there)
  for (int p = tid; p < kCfNp; p += kCfThreads) {
    const float sp = S[p];
    B1[p] = (sp > A.sigclip && !M[p] && sp / Fp[p] > A.objlim) ? 1 : 0;
  }
  __syncthreads();
  for (int p = tid; p < kCfNp; p += kCfThreads) {
    const int ly = p / kCfR, lx = p - ly * kCfR;
    B2[p] = (la_dil3(B1, ly, lx, kCfR) && S[p] > A.sigclip && !M[p]) ? 1 : 0;
  }
  __syncthreads();
  // g: CR |= g2 on the tile
  int any = 0;
  for (int p = tid; p < kCfTile * kCfTile; p += kCfThreads) {
    const int ly = kCfHalo + p / kCfTile, lx = kCfHalo + p % kCfTile;
    if (!T.inside(ly, lx)) continue;
    const int r = ly * kCfR + lx;
    if (la_dil3(B2, ly, lx, kCfR) && S[r] > A.sigcliplow && !M[r]) {
      A.CR[base + (size_t)(T.oy + ly) * A.w + (T.ox + lx)] = 1;
      any = 1;
    }
  }
  if (__syncthreads_or(any) && tid == 0) atomicAdd(&st[kStFound], 1);
}

__device__ __forceinline__ bool cf_cleaning(const int32_t *st) { return st[kStRunning] && st[kStFound]; }

// step 2h in place; grid (blocks, frames of the chunk)
__global__ __launch_bounds__(kCfPixThreads) void cf_clean_kernel(CfArgs A) {
  const int k = blockIdx.y;
  int32_t *st = A.state + (size_t)k * kStWords;
  if (!cf_cleaning(st)) return;
  const size_t base = (size_t)k * A.hw;
  float *C = A.C + base;
  uint8_t *CR = A.CR + base;
  const uint8_t *M = A.M + base;
  const int h = A.h, w = A.w;
  int need = 0;
  for (size_t p = (size_t)blockIdx.x * kCfPixThreads + threadIdx.x; p < A.hw; p += (size_t)gridDim.x * kCfPixThreads) {
    if (!CR[p]) continue;
    const int i = (int)(p / w), j = (int)(p - (size_t)i * w);
    float acc = 0.f;
    int cnt = 0;
    for (int y = max(i - 2, 0); y <= min(i + 2, h - 1); ++y)
      for (int x = max(j - 2, 0); x <= min(j + 2, w - 1); ++x) {
        const size_t q = (size_t)y * w + x;
        if (!CR[q] && !M[q]) {
          acc = acc + C[q];
          ++cnt;
        }
      }
    if (cnt) {
      C[p] = acc / (float)cnt;
    } else {
      CR[p] = 2;
      need = 1;
    }
  }
  if (__syncthreads_or(need) && threadIdx.x == 0) atomicOr(&st[kStNeed], 1);
}

__device__ __forceinline__ bool cf_selecting(const int32_t *st) { return cf_cleaning(st) && st[kStNeed]; }

// pass A.pass of the radix select: the histogram of byte 3 - pass of the keys of the good pixels whose higher bytes
// equal the prefix found so far; grid (blocks, frames of the chunk)
__global__ __launch_bounds__(kCfPixThreads) void cf_hist_kernel(CfArgs A) {
  __shared__ unsigned s_hist[256];
  const int k = blockIdx.y;
  const int32_t *st = A.state + (size_t)k * kStWords;
  if (!cf_selecting(st)) return;
  const size_t base = (size_t)k * A.hw;
  const unsigned prefix = (unsigned)st[kStPrefix];
  const int shift = 24 - 8 * A.pass;
  s_hist[threadIdx.x] = 0;  // kCfPixThreads == 256
  __syncthreads();
  for (size_t p = (size_t)blockIdx.x * kCfPixThreads + threadIdx.x; p < A.hw; p += (size_t)gridDim.x * kCfPixThreads) {
    if (A.CR[base + p] || A.M[base + p]) continue;
    const unsigned key = float_key(A.C[base + p]);
    if (A.pass > 0 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
    atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  const unsigned c = s_hist[threadIdx.x];
  if (c) atomicAdd(&A.hist[(size_t)k * 256 + threadIdx.x], c);
}
static_assert(kCfPixThreads == 256, "cf_hist_kernel: one lane per bin");

// after pass A.pass: the bin that holds the rank, one lane per frame; grid (ceil(frames / 64))
__global__ __launch_bounds__(64) void cf_pick_kernel(CfArgs A, int frames) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= frames) return;
  int32_t *st = A.state + (size_t)k * kStWords;
  if (!cf_selecting(st)) return;
  uint32_t *hist = A.hist + (size_t)k * 256;
  if (A.pass == 0) {
    unsigned m = 0;
    for (int b = 0; b < 256; ++b) m += hist[b];
    st[kStRank] = m ? (int)((m - 1) / 2) : -1;  // -1: no good pixel, the value is 0
    st[kStPrefix] = 0;
    st[kStFallback] = 0;
  }
  const int rank = st[kStRank];
  if (rank >= 0) {
    unsigned cum = 0;
    int b = 0;
    for (; b < 255; ++b) {
      if ((unsigned)rank < cum + hist[b]) break;
      cum += hist[b];
    }
    const unsigned prefix = (unsigned)st[kStPrefix] | ((unsigned)b << (24 - 8 * A.pass));
    st[kStPrefix] = (int)prefix;
    st[kStRank] = rank - (int)cum;
    if (A.pass == 3) st[kStFallback] = (int)__float_as_uint(float_unkey(prefix));
  }
  for (int b = 0; b < 256; ++b) hist[b] = 0;
}

// the fall-back value to the pixels marked 2; grid (blocks, frames of the chunk)
__global__ __launch_bounds__(kCfPixThreads) void cf_fixup_kernel(CfArgs A) {
  const int k = blockIdx.y;
  const int32_t *st = A.state + (size_t)k * kStWords;
  if (!cf_selecting(st)) return;
  const size_t base = (size_t)k * A.hw;
  const float value = __uint_as_float((unsigned)st[kStFallback]);
  for (size_t p = (size_t)blockIdx.x * kCfPixThreads + threadIdx.x; p < A.hw; p += (size_t)gridDim.x * kCfPixThreads) {
    if (A.CR[base + p] == 2) {
      A.C[base + p] = value;
      A.CR[base + p] = 1;
    }
  }
}

// the frames' control words: before the first iteration (A.it < 0), and after iteration A.it
__global__ __launch_bounds__(64) void cf_step_kernel(CfArgs A, int frames, int niter) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= frames) return;
  int32_t *st = A.state + (size_t)k * kStWords;
  if (A.it < 0) {
    for (int i = 0; i < kStWords; ++i) st[i] = 0;
    st[kStRunning] = niter > 0 ? 1 : 0;
    return;
  }
  if (st[kStRunning]) {
    st[kStIters] = A.it + 1;
    if (st[kStFound])
      atomicAdd(A.running, 1);
    else
      st[kStRunning] = 0;
  }
  st[kStFound] = 0;
  st[kStNeed] = 0;
}

// the outputs of the chunk; grid (blocks, frames of the chunk)
__global__ __launch_bounds__(kCfPixThreads) void cf_finish_kernel(CfArgs A) {
  const int k = blockIdx.y;
  const size_t base = (size_t)k * A.hw;
  float *plane = A.apply ? A.planes + (size_t)A.frame[k] * A.hw : nullptr;
  int flagged = 0;
  for (size_t p = (size_t)blockIdx.x * kCfPixThreads + threadIdx.x; p < A.hw; p += (size_t)gridDim.x * kCfPixThreads) {
    const uint8_t cr = A.CR[base + p] ? 1 : 0;
    const float clean = A.C[base + p] / A.gain;
    if (A.crmask) A.crmask[base + p] = cr;
    if (A.clean) A.clean[base + p] = clean;
    if (cr && A.apply) plane[p] = A.apply == LC_COSMICS_SET_NAN ? __builtin_nanf("") : clean;
    flagged += cr;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) flagged += __shfl_down(flagged, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && flagged && A.n_flagged) atomicAdd(&A.n_flagged[k], flagged);
  if (blockIdx.x == 0 && threadIdx.x == 0 && A.iters) A.iters[k] = A.state[(size_t)k * kStWords + kStIters];
}

static bool cosmics_frames_shape_ok(int h, int w) {
  return h >= kCfMinSide && w >= kCfMinSide && (int64_t)h * w < ((int64_t)1 << 31);
}

int cosmics_frames_check(lc_ctx *ctx, const char *who, int h, int w, const lc_cosmics_cfg *cfg, int scratch_frames) {
  const std::string s(who);
  if (scratch_frames < 0) LC_FAIL(ctx, LC_ERR_INVALID, s + ": scratch_frames must be >= 0");
  // (the settings the stamp kernel refuses, at a stamp size it takes)
  if (int rc = cosmics_check(ctx, who, kCfMinSide, cfg)) return rc;
  if (!cosmics_frames_shape_ok(h, w)) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, s + ": frames of h, w >= 8 with h w < 2^31 only");
  if (cfg->sepmed == 0) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, s + ": only the separable medians (sepmed = 1) are built for frames");
  return LC_OK;
}

int cosmics_frames_chunk(int K, int h, int w, bool with_variance, int scratch_frames) {
  const size_t per_frame = (size_t)h * w * (with_variance ? 10 : 6);
  const size_t fit = scratch_frames > 0 ? (size_t)scratch_frames : std::max<size_t>(1, kCfScratchBytes / per_frame);
  return (int)std::min<size_t>(std::min<size_t>(fit, (size_t)K), (size_t)kCfMaxChunk);
}

hipError_t cosmics_frames_scratch(DeviceCall &call, int K, int h, int w, bool with_variance, int scratch_frames,
                                  CosmicsFramesScratch *S) {
  S->chunk = cosmics_frames_chunk(K, h, w, with_variance, scratch_frames);
  const size_t tot = (size_t)S->chunk * h * w;
  hipError_t e = call.alloc(tot, &S->C);
  if (e == hipSuccess && with_variance) e = call.alloc(tot, &S->N);
  if (e == hipSuccess) e = call.alloc(tot, &S->M);
  if (e == hipSuccess) e = call.alloc(tot, &S->CR);
  if (e == hipSuccess) e = call.alloc((size_t)S->chunk * kStWords, &S->state);
  if (e == hipSuccess) e = call.alloc((size_t)S->chunk * 256, &S->hist);
  if (e == hipSuccess) e = call.alloc((size_t)1, &S->running);
  return e;
}

#define CF_TRY(call)                   \
  do {                                 \
    hipError_t e_ = (call);            \
    if (e_ != hipSuccess) return e_;   \
  } while (0)

hipError_t cosmics_frames_launch(lc_ctx *ctx, int K, int h, int w, const CosmicsFramesIO &io, const lc_cosmics_cfg *cfg,
                                 const CosmicsFramesScratch &S) {
  const size_t hw = (size_t)h * w;
  CfArgs A;
  std::memset(&A, 0, sizeof(A));
  A.h = h;
  A.w = w;
  A.hw = hw;
  A.ntx = (w + kCfTile - 1) / kCfTile;
  A.have_var = (io.invar || (io.exptime && io.rms)) ? 1 : 0;
  A.exptime = io.exptime;
  A.rms = io.rms;
  A.C = S.C;
  A.N = S.N;
  A.M = S.M;
  A.CR = S.CR;
  A.state = S.state;
  A.hist = S.hist;
  A.running = S.running;
  A.planes = io.planes;
  A.apply = io.apply;
  A.gain = cfg->gain;
  A.gain2 = cfg->gain * cfg->gain;
  A.rn2 = cfg->readnoise * cfg->readnoise;
  A.vhole = 1e-5f + A.rn2;
  A.satg = cfg->gain * cfg->satlevel;
  A.satg10 = A.satg / 10.0f;
  A.sigclip = cfg->sigclip;
  A.sigcliplow = cfg->sigfrac * cfg->sigclip;
  A.objlim = cfg->objlim;
  const unsigned tiles = (unsigned)A.ntx * (unsigned)((h + kCfTile - 1) / kCfTile);
  const unsigned pix_blocks = (unsigned)std::min<size_t>((hw + kCfPixThreads - 1) / kCfPixThreads, (size_t)kCfPixBlocks);
  CF_TRY(hipFuncSetAttribute((const void *)cf_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCfLdsBytes));
  CF_TRY(hipFuncSetAttribute((const void *)cf_detect_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCfLdsBytes));
  if (io.n_flagged) CF_TRY(hipMemsetAsync(io.n_flagged, 0, (size_t)K * sizeof(int32_t), ctx->stream));
  for (int c0 = 0; c0 < K; c0 += S.chunk) {
    const int kc = std::min(S.chunk, K - c0);
    const size_t off = (size_t)c0 * hw;
    A.data = io.frame ? io.data : io.data + off;
    A.frame = io.frame ? io.frame + c0 : nullptr;
    A.invar = io.invar ? io.invar + off : nullptr;
    A.inmask = io.inmask ? io.inmask + off : nullptr;
    A.crmask = io.crmask ? io.crmask + off : nullptr;
    A.clean = io.clean ? io.clean + off : nullptr;
    A.iters = io.iters ? io.iters + c0 : nullptr;
    A.n_flagged = io.n_flagged ? io.n_flagged + c0 : nullptr;
    const dim3 tile_grid(tiles, (unsigned)kc), pix_grid(pix_blocks, (unsigned)kc), frame_grid((unsigned)(kc + 63) / 64);
    CF_TRY(hipMemsetAsync(S.hist, 0, (size_t)kc * 256 * sizeof(uint32_t), ctx->stream));
    A.it = -1;
    hipLaunchKernelGGL(cf_step_kernel, frame_grid, dim3(64), 0, ctx->stream, A, kc, cfg->niter);
    hipLaunchKernelGGL(cf_prep_kernel, tile_grid, dim3(kCfThreads), kCfLdsBytes, ctx->stream, A);
    CF_TRY(hipGetLastError());
    for (int it = 0; it < cfg->niter; ++it) {
      A.it = it;
      hipLaunchKernelGGL(cf_detect_kernel, tile_grid, dim3(kCfThreads), kCfLdsBytes, ctx->stream, A);
      hipLaunchKernelGGL(cf_clean_kernel, pix_grid, dim3(kCfPixThreads), 0, ctx->stream, A);
      for (int pass = 0; pass < 4; ++pass) {
        A.pass = pass;
        hipLaunchKernelGGL(cf_hist_kernel, pix_grid, dim3(kCfPixThreads), 0, ctx->stream, A);
        hipLaunchKernelGGL(cf_pick_kernel, frame_grid, dim3(64), 0, ctx->stream, A, kc);
      }
      hipLaunchKernelGGL(cf_fixup_kernel, pix_grid, dim3(kCfPixThreads), 0, ctx->stream, A);
      CF_TRY(hipMemsetAsync(S.running, 0, sizeof(int32_t), ctx->stream));
      hipLaunchKernelGGL(cf_step_kernel, frame_grid, dim3(64), 0, ctx->stream, A, kc, cfg->niter);
      CF_TRY(hipGetLastError());
      if (it + 1 == cfg->niter) break;
      int32_t running = 0;
      CF_TRY(hipMemcpyAsync(&running, S.running, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      CF_TRY(hipStreamSynchronize(ctx->stream));
      if (!running) break;
    }
    hipLaunchKernelGGL(cf_finish_kernel, pix_grid, dim3(kCfPixThreads), 0, ctx->stream, A);
    CF_TRY(hipGetLastError());
  }
  return hipSuccess;
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_cosmics_frames_supported(int h, int w) { return cosmics_frames_shape_ok(h, w) ? 1 : 0; }

int lc_detect_cosmics_frames(lc_ctx *ctx, int K, int h, int w, const float *data, const float *invar, const uint8_t *inmask,
                             const lc_cosmics_cfg *cfg, int scratch_frames, uint8_t *crmask, float *clean, int32_t *iters,
                             int32_t *n_flagged, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K < 1 || !data || !cfg || !crmask) LC_FAIL(ctx, LC_ERR_INVALID, "lc_detect_cosmics_frames: invalid argument");
  if (int rc = cosmics_frames_check(ctx, "lc_detect_cosmics_frames", h, w, cfg, scratch_frames)) return rc;
  LC_ENTER(ctx);
  const size_t tot = (size_t)K * h * w;
  DeviceCall call(ctx);
  CosmicsFramesIO io;
  CosmicsFramesScratch S;
  LC_HIP(ctx, call.upload(data, tot, &io.data));
  LC_HIP(ctx, call.upload(invar, tot, &io.invar));
  LC_HIP(ctx, call.upload(inmask, tot, &io.inmask));
  LC_HIP(ctx, call.result(crmask, tot, &io.crmask));
  LC_HIP(ctx, call.result(clean, tot, &io.clean));
  LC_HIP(ctx, call.result(iters, (size_t)K, &io.iters));
  LC_HIP(ctx, call.result(n_flagged, (size_t)K, &io.n_flagged));
  LC_HIP(ctx, cosmics_frames_scratch(call, K, h, w, invar != nullptr, scratch_frames, &S));
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, cosmics_frames_launch(ctx, K, h, w, io, cfg, S));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

int lc_frames_detect_cosmics(lc_frames *f, int n, const int32_t *frame, const float *exptime, const float *rms,
                             int noise_from_rms, const uint8_t *inmask, const lc_cosmics_cfg *cfg, int apply,
                             int scratch_frames, uint8_t *crmask, float *clean, int32_t *iters, int32_t *n_flagged,
                             float *kernel_ms) {
  if (!f) return LC_ERR_INVALID;
  lc_ctx *ctx = f->ctx;
  const int K = f->K, h = f->h, w = f->w;
  if (n < 1 || !frame || !cfg) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_detect_cosmics: invalid argument");
  if (apply != 0 && apply != LC_COSMICS_SET_NAN && apply != LC_COSMICS_SET_CLEAN)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_detect_cosmics: unknown apply");
  if (!apply && !crmask && !clean && !iters && !n_flagged)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_detect_cosmics: neither an output nor apply");
  std::vector<char> seen((size_t)K, 0);
  for (int k = 0; k < n; ++k) {
    if (frame[k] < 0 || frame[k] >= K) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_detect_cosmics: a frame index outside the set");
    if (apply && seen[frame[k]]) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_detect_cosmics: a frame listed twice with apply");
    seen[frame[k]] = 1;
  }
  if (noise_from_rms) {
    if ((!exptime || !rms) && !f->imported)
      LC_FAIL(ctx, LC_ERR_INVALID,
              "lc_frames_detect_cosmics: the noise from rms needs exptime and rms, or a frame set that has been imported");
    if (exptime)
      for (int k = 0; k < K; ++k)
        if (!std::isfinite(exptime[k]) || !(exptime[k] > 0.0f))
          LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_detect_cosmics: an exposure time that is not finite or not > 0");
  }
  if (int rc = cosmics_frames_check(ctx, "lc_frames_detect_cosmics", h, w, cfg, scratch_frames)) return rc;
  LC_ENTER(ctx);
  const size_t tot = (size_t)n * h * w;
  DeviceCall call(ctx);
  CosmicsFramesIO io;
  CosmicsFramesScratch S;
  io.data = f->planes;
  io.planes = f->planes;
  io.apply = apply;
  LC_HIP(ctx, call.upload(frame, (size_t)n, &io.frame));
  if (noise_from_rms) {
    io.exptime = f->exptime;
    io.rms = f->rms;
    if (exptime) LC_HIP(ctx, call.upload(exptime, (size_t)K, &io.exptime));
    if (rms) LC_HIP(ctx, call.upload(rms, (size_t)K, &io.rms));
  }
  LC_HIP(ctx, call.upload(inmask, tot, &io.inmask));
  LC_HIP(ctx, call.result(crmask, tot, &io.crmask));
  LC_HIP(ctx, call.result(clean, tot, &io.clean));
  LC_HIP(ctx, call.result(iters, (size_t)n, &io.iters));
  LC_HIP(ctx, call.result(n_flagged, (size_t)n, &io.n_flagged));
  LC_HIP(ctx, cosmics_frames_scratch(call, n, h, w, noise_from_rms != 0, scratch_frames, &S));
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, cosmics_frames_launch(ctx, n, h, w, io, cfg, S));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
