// Source extraction of whole frames: detection, 8-connected labelling and measurement, what sep.extract does without
// de-blending and cleaning (lightcurver/processes/star_extraction.py:23, background_estimation.py:32), frozen as the SPEC
// of DESIGN.md §5 "Source extraction of frames" and restated in NumPy by tests/_extract.py.  K frames of one shape per
// call, the phases as separate launches; no workgroup waits for another within a launch (no flags, no spin loops):
//   ex_tile_kernel     one workgroup per 64 x 16 tile: w and dw of the tile and its rim into LDS, snr, detection, a
//                      union-find over the tile in LDS; writes snr and, per detected pixel, the raster index of the first
//                      pixel of its component within the tile (-1 elsewhere);
//   ex_merge_kernel    one workgroup per tile: the links of its first row and outer columns that cross a tile border,
//                      as atomicMin unions on the label plane;
//   ex_flatten_kernel  every pixel takes its root; every horizontal run adds its length to the root's count;
//   ex_count_kernel, ex_scan_kernel, ex_number_kernel
//                      the roots with at least minarea pixels, counted per block of 256 pixels, scanned per frame and
//                      numbered in raster order: the root's count becomes its object number;
//   ex_box_kernel      segmap and mask, and the bounding boxes by integer atomicMin / atomicMax per run of one object;
//   ex_measure_kernel  one workgroup per object over its box: integer moments, peaks and the flux in a fixed order.
// Labels only ever decrease (a pixel points at a pixel before it in raster order), so every find terminates; the loops
// carry a bound all the same, and reaching it sets the frame's status to 2.  Offsets into the planes are 64-bit.
#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "block_reduce.h"
#include "device_call.h"
#include "frame_steps.h"
#include "lc_common.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kExThreads = 256;
constexpr int kExWaves = kExThreads / kWave;
constexpr int kExTW = 64, kExTH = 16;  // the tile of the LDS union-find
constexpr int kExTile = kExTW * kExTH;
constexpr int kExPerLane = kExTile / kExThreads;
constexpr int kExHW = kExTW + 2, kExHH = kExTH + 2;  // with the rim of the 3 x 3 filter
constexpr int kExBorder = kExTW + 2 * (kExTH - 1);   // pixels of a tile with a link across its border
constexpr int kExMergeThreads = 128;
constexpr int kExLargeBox = 512;
constexpr float kExSnrLimit = 65536.0f;
constexpr double kExFix = 1024.0;  // 2^10: the fixed point of the moments' weights
constexpr int kExAux = 6;          // first, npix, xmin, xmax, ymin, ymax
constexpr int kExMeasureBlocks = 4096;

typedef unsigned long long u64;

struct ExGeom {
  int h, w, tx, ty;  // pixels, tiles
  int hw;            // pixels of a frame, < 2^31
  unsigned nblk;     // blocks of 256 pixels of a frame
};

__device__ __forceinline__ void ex_guard(int32_t *status) { atomicMax(status, 2); }

// Which of the neighbours W, NW, N, NE (bits 0 - 3) a detected pixel links itself to.  N joins NW and NE through their
// own links to N; W joins NW through W's link to its N.  Over all pixels these links connect every 8-connected pair.
__device__ __forceinline__ unsigned ex_links(bool w_, bool nw, bool n, bool ne) {
  unsigned m = w_ ? 1u : 0u;
  if (n) return m | 4u;
  if (nw && !w_) m |= 2u;
  if (ne) m |= 8u;
  return m;
}

// ---- tile: snr, detection, union-find in LDS -------------------------------------------------------------------------

__device__ __forceinline__ int ex_find_lds(volatile int *lab, int p, bool &guard) {
  for (int i = 0; i <= kExTile; ++i) {
    const int q = lab[p];
    if (q == p) return p;
    p = q;
  }
  guard = true;
  return p;
}

__device__ __forceinline__ void ex_union_lds(int *lab, int a, int b, bool &guard) {
  for (int i = 0; i <= 2 * kExTile; ++i) {  // a + b falls in every round
    a = ex_find_lds(lab, a, guard);
    b = ex_find_lds(lab, b, guard);
    if (a == b || guard) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
  guard = true;
}

struct ExTileArgs {
  ExGeom g;
  const float *data, *var, *var_scalar;
  float thresh;
  int filter;
  float *snr;
  int32_t *label, *status;
};

__global__ __launch_bounds__(kExThreads) void ex_tile_kernel(ExTileArgs A) {
  __shared__ float s_w[kExHH][kExHW], s_dw[kExHH][kExHW];
  __shared__ int s_lab[kExTile];
  const ExGeom g = A.g;
  const int tid = threadIdx.x;
  const unsigned tiles = (unsigned)(g.tx * g.ty);
  const unsigned frame = blockIdx.x / tiles, t = blockIdx.x - frame * tiles;
  const int tyi = (int)(t / (unsigned)g.tx), txi = (int)t - tyi * g.tx;
  const int x0 = txi * kExTW, y0 = tyi * kExTH;
  const size_t base = (size_t)frame * (size_t)g.hw;
  const float v0 = A.var ? 0.0f : A.var_scalar[frame];

  for (int i = tid; i < kExHH * kExHW; i += kExThreads) {
    const int ly = i / kExHW, lx = i - ly * kExHW;
    const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
    float w = 0.0f, dw = 0.0f;
    if (gy >= 0 && gy < g.h && gx >= 0 && gx < g.w) {
      const size_t off = base + (size_t)gy * g.w + gx;
      const float d = A.data[off], v = A.var ? A.var[off] : v0;
      if (__builtin_isfinite(d) && __builtin_isfinite(v) && v > 0.0f) {
        w = 1.0f / v;
        dw = d * w;
      }
    }
    s_w[ly][lx] = w;
    s_dw[ly][lx] = dw;
  }
  __syncthreads();

  bool det[kExPerLane];
#pragma unroll
  for (int j = 0; j < kExPerLane; ++j) {
    const int p = tid + j * kExThreads, ly = p / kExTW, lx = p - ly * kExTW;
    const int gy = y0 + ly, gx = x0 + lx;
    det[j] = false;
    if (gy < g.h && gx < g.w) {
      float num = 0.0f, den2 = 0.0f;
      if (A.filter) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float kf = (float)((2 - (dy == 1 ? 0 : 1)) * (2 - (dx == 1 ? 0 : 1)));
            num = num + kf * s_dw[ly + dy][lx + dx];
            den2 = den2 + (kf * kf) * s_w[ly + dy][lx + dx];
          }
      } else {
        num = num + 1.0f * s_dw[ly + 1][lx + 1];
        den2 = den2 + (1.0f * 1.0f) * s_w[ly + 1][lx + 1];
      }
      const float r = den2 > 0.0f ? num / sqrtf(den2) : 0.0f;
      A.snr[base + (size_t)gy * g.w + gx] = r;
      det[j] = r > A.thresh;
    }
    s_lab[p] = det[j] ? p : -1;
  }
  __syncthreads();

  bool guard = false;
#pragma unroll
  for (int j = 0; j < kExPerLane; ++j) {
    if (!det[j]) continue;
    const int p = tid + j * kExThreads, ly = p / kExTW, lx = p - ly * kExTW;
    const bool up = ly > 0, lf = lx > 0, rt = lx < kExTW - 1;
    const unsigned m = ex_links(lf && s_lab[p - 1] >= 0, up && lf && s_lab[p - kExTW - 1] >= 0, up && s_lab[p - kExTW] >= 0,
                                up && rt && s_lab[p - kExTW + 1] >= 0);
    if (m & 1u) ex_union_lds(s_lab, p, p - 1, guard);
    if (m & 2u) ex_union_lds(s_lab, p, p - kExTW - 1, guard);
    if (m & 4u) ex_union_lds(s_lab, p, p - kExTW, guard);
    if (m & 8u) ex_union_lds(s_lab, p, p - kExTW + 1, guard);
  }
  __syncthreads();

#pragma unroll
  for (int j = 0; j < kExPerLane; ++j) {
    const int p = tid + j * kExThreads, ly = p / kExTW, lx = p - ly * kExTW;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy < g.h && gx < g.w) {
      int32_t l = -1;
      if (det[j]) {
        const int r = ex_find_lds(s_lab, p, guard);
        l = (y0 + r / kExTW) * g.w + x0 + (r % kExTW);
      }
      A.label[base + (size_t)gy * g.w + gx] = l;
    }
  }
  if (guard) ex_guard(A.status + frame);
}

// ---- the label plane of one frame in device memory --------------------------------------------------------------------

// the root of p: labels fall along the way, so at most hw steps
__device__ __forceinline__ int ex_find(int32_t *L, int p, int hw, bool &guard) {
  for (int i = 0; i < hw; ++i) {
    const int q = __hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == p) return p;
    if (q < 0 || q > p) break;  // no label of a detected pixel: never written by these kernels
    p = q;
  }
  guard = true;
  return p;
}

__device__ __forceinline__ void ex_union(int32_t *L, int a, int b, int hw, bool &guard) {
  for (long long i = 0; i < 2ll * hw; ++i) {  // a + b falls in every round, and both are below hw
    a = ex_find(L, a, hw, guard);
    b = ex_find(L, b, hw, guard);
    if (a == b || guard) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
  guard = true;
}

struct ExMergeArgs {
  ExGeom g;
  int32_t *label, *status;
};

__global__ __launch_bounds__(kExMergeThreads) void ex_merge_kernel(ExMergeArgs A) {
  const ExGeom g = A.g;
  const int tid = threadIdx.x;
  if (tid >= kExBorder) return;
  const unsigned tiles = (unsigned)(g.tx * g.ty);
  const unsigned frame = blockIdx.x / tiles, t = blockIdx.x - frame * tiles;
  const int tyi = (int)(t / (unsigned)g.tx), txi = (int)t - tyi * g.tx;
  // the first row, then the first and the last column below it
  int lx, ly;
  if (tid < kExTW) {
    lx = tid;
    ly = 0;
  } else if (tid < kExTW + kExTH - 1) {
    lx = 0;
    ly = tid - kExTW + 1;
  } else {
    lx = kExTW - 1;
    ly = tid - (kExTW + kExTH - 1) + 1;
  }
  const int gx = txi * kExTW + lx, gy = tyi * kExTH + ly;
  if (gx >= g.w || gy >= g.h) return;
  int32_t *L = A.label + (size_t)frame * (size_t)g.hw;
  const int p = gy * g.w + gx;
  if (L[p] < 0) return;
  const bool up = gy > 0, lf = gx > 0, rt = gx < g.w - 1;
  const unsigned m = ex_links(lf && L[p - 1] >= 0, up && lf && L[p - g.w - 1] >= 0, up && L[p - g.w] >= 0,
                              up && rt && L[p - g.w + 1] >= 0);
  // the links that leave the tile; the others were made in LDS
  const bool xl = lx == 0, xr = lx == kExTW - 1, yu = ly == 0;
  bool guard = false;
  if ((m & 1u) && xl) ex_union(L, p, p - 1, g.hw, guard);
  if ((m & 2u) && (xl || yu)) ex_union(L, p, p - g.w - 1, g.hw, guard);
  if ((m & 4u) && yu) ex_union(L, p, p - g.w, g.hw, guard);
  if ((m & 8u) && (xr || yu)) ex_union(L, p, p - g.w + 1, g.hw, guard);
  if (guard) ex_guard(A.status + frame);
}

// Horizontal runs inside a block of 256 consecutive pixels: lane tid heads a run if its pixel is set and the pixel
// before it is not, or lies in another block or line; the run's length from the flags in LDS.
__device__ __forceinline__ int ex_run(const uint8_t *s_set, int tid, int x, int w, int left_in_block) {
  if (!s_set[tid] || (tid > 0 && x > 0 && s_set[tid - 1])) return 0;
  const int room = min(left_in_block, w - x);
  int len = 1;
  while (len < room && s_set[tid + len]) ++len;
  return len;
}

struct ExFlattenArgs {
  ExGeom g;
  int32_t *label, *count, *status;
};

__global__ __launch_bounds__(kExThreads) void ex_flatten_kernel(ExFlattenArgs A) {
  __shared__ uint8_t s_set[kExThreads];
  const ExGeom g = A.g;
  const int tid = threadIdx.x;
  const unsigned frame = blockIdx.x / g.nblk, b = blockIdx.x - frame * g.nblk;
  const size_t base = (size_t)frame * (size_t)g.hw;
  int32_t *L = A.label + base;
  const long long p64 = (long long)b * kExThreads + tid;
  const bool in = p64 < (long long)g.hw;
  const int p = in ? (int)p64 : 0;
  int root = -1;
  bool guard = false;
  if (in) {
    const int l = L[p];
    if (l >= 0) {
      root = ex_find(L, l, g.hw, guard);
      if (root != l) __hip_atomic_store(L + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  s_set[tid] = root >= 0;
  __syncthreads();
  if (root >= 0) {
    const int x = p % g.w;
    const int left = (int)min((long long)(kExThreads - tid), (long long)g.hw - p64);
    const int len = ex_run(s_set, tid, x, g.w, left);
    if (len > 0) atomicAdd(A.count + base + root, len);
  }
  if (guard) ex_guard(A.status + frame);
}

// ---- numbering the objects in raster order ---------------------------------------------------------------------------

struct ExNumberArgs {
  ExGeom g;
  int minarea, max_objects;
  const int32_t *label;
  int32_t *count, *block, *status, *nobj, *aux;
};

__device__ __forceinline__ bool ex_is_object(const ExNumberArgs &A, size_t base, long long p64, int &npix, bool &root) {
  npix = 0;
  root = false;
  if (p64 >= (long long)A.g.hw) return false;
  root = A.label[base + p64] == (int32_t)p64;
  if (!root) return false;
  npix = A.count[base + p64];
  return npix >= A.minarea;
}

__global__ __launch_bounds__(kExThreads) void ex_count_kernel(ExNumberArgs A) {
  const unsigned frame = blockIdx.x / A.g.nblk, b = blockIdx.x - frame * A.g.nblk;
  const size_t base = (size_t)frame * (size_t)A.g.hw;
  int npix;
  bool root;
  const bool ok = A.status[frame] != 2 && ex_is_object(A, base, (long long)b * kExThreads + threadIdx.x, npix, root);
  const int n = __syncthreads_count(ok ? 1 : 0);
  if (threadIdx.x == 0) A.block[(size_t)frame * A.g.nblk + b] = n;
}

// exclusive scan of the frame's block counts in place, one workgroup per frame; nobj and status 1
__global__ __launch_bounds__(kExThreads) void ex_scan_kernel(ExNumberArgs A) {
  __shared__ int s_wave[kExWaves];
  const unsigned frame = blockIdx.x;
  int32_t *blk = A.block + (size_t)frame * A.g.nblk;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  int carry = 0;
  for (unsigned c0 = 0; c0 < A.g.nblk; c0 += kExThreads) {
    const unsigned i = c0 + tid;
    const int v = i < A.g.nblk ? blk[i] : 0;
    const int incl = wave_inclusive_scan(v);
    if (lane == kWave - 1) s_wave[wv] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kExWaves; ++k) {
      if (k < wv) before += s_wave[k];
      total += s_wave[k];
    }
    if (i < A.g.nblk) blk[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) {
    A.nobj[frame] = carry;  // 0 for a frame with status 2: ex_count_kernel counted nothing
    if (carry > A.max_objects && A.status[frame] == 0) A.status[frame] = 1;
  }
}

// the root's count becomes its object number (0 for a component below minarea); the first columns of the table
__global__ __launch_bounds__(kExThreads) void ex_number_kernel(ExNumberArgs A) {
  __shared__ int s_wave[kExWaves];
  const unsigned frame = blockIdx.x / A.g.nblk, b = blockIdx.x - frame * A.g.nblk;
  const size_t base = (size_t)frame * (size_t)A.g.hw;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const long long p64 = (long long)b * kExThreads + tid;
  int npix;
  bool root;
  const bool ok = A.status[frame] != 2 && ex_is_object(A, base, p64, npix, root);
  const u64 bal = __ballot(ok);
  const int below = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) s_wave[wv] = __popcll(bal);
  __syncthreads();
  int before = 0;
  for (int k = 0; k < wv; ++k) before += s_wave[k];
  if (!root) return;
  const int i = A.block[(size_t)frame * A.g.nblk + b] + before + below;  // 0-based, in raster order of the roots
  A.count[base + p64] = ok ? i + 1 : 0;
  if (ok && A.aux && i < A.max_objects) {
    int32_t *a = A.aux + ((size_t)frame * A.max_objects + i) * kExAux;
    a[0] = (int32_t)p64;
    a[1] = npix;
    a[2] = INT_MAX;
    a[3] = -1;
    a[4] = INT_MAX;
    a[5] = -1;
  }
}

struct ExBoxArgs {
  ExGeom g;
  int max_objects;
  const int32_t *label, *count;
  int32_t *aux, *segmap;
  uint8_t *mask;
};

// The same for runs of one object number: after de-blending (deblend.hip) two objects can touch within a line.  Without
// it a detected pixel and its detected neighbour belong to one component, and these runs are those of ex_run.
__device__ __forceinline__ int ex_run_of(const int *s_num, int tid, int x, int w, int left_in_block) {
  const int num = s_num[tid];
  if (num <= 0 || (tid > 0 && x > 0 && s_num[tid - 1] == num)) return 0;
  const int room = min(left_in_block, w - x);
  int len = 1;
  while (len < room && s_num[tid + len] == num) ++len;
  return len;
}

__global__ __launch_bounds__(kExThreads) void ex_box_kernel(ExBoxArgs A) {
  __shared__ int s_num[kExThreads];
  const ExGeom g = A.g;
  const int tid = threadIdx.x;
  const unsigned frame = blockIdx.x / g.nblk, b = blockIdx.x - frame * g.nblk;
  const size_t base = (size_t)frame * (size_t)g.hw;
  const long long p64 = (long long)b * kExThreads + tid;
  const bool in = p64 < (long long)g.hw;
  int num = 0;
  if (in) {
    const int l = A.label[base + p64];
    if (l >= 0) num = A.count[base + l];
    if (A.segmap) A.segmap[base + p64] = num;
    if (A.mask) A.mask[base + p64] = num > 0;
  }
  s_num[tid] = num;
  __syncthreads();
  if (num > 0 && num <= A.max_objects && A.aux) {
    const int p = (int)p64, y = p / g.w, x = p - y * g.w;
    const int left = (int)min((long long)(kExThreads - tid), (long long)g.hw - p64);
    const int len = ex_run_of(s_num, tid, x, g.w, left);
    if (len > 0) {
      int32_t *a = A.aux + ((size_t)frame * A.max_objects + (num - 1)) * kExAux;
      atomicMin(a + 2, x);
      atomicMax(a + 3, x + len - 1);
      atomicMin(a + 4, y);
      atomicMax(a + 5, y);
    }
  }
}

// ---- measurement ---------------------------------------------------------------------------------------------------------

struct ExMeasureArgs {
  ExGeom g;
  int K, max_objects;
  const float *data, *snr;
  const int32_t *label, *aux, *nobj;
  lc_extract_object *objects;
};

__global__ __launch_bounds__(kExThreads) void ex_measure_kernel(ExMeasureArgs A) {
  __shared__ u64 s_u[kExWaves];
  __shared__ double s_d[kExWaves];
  __shared__ float s_f[kExWaves], s_c[kExWaves];
  __shared__ int s_i[kExWaves], s_r[kExWaves];
  const ExGeom g = A.g;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const long long slots = (long long)A.K * A.max_objects;
  for (long long s = blockIdx.x; s < slots; s += gridDim.x) {
    const int frame = (int)(s / A.max_objects), i = (int)(s - (long long)frame * A.max_objects);
    if (i >= min(A.nobj[frame], A.max_objects)) continue;  // the same for every lane
    const int32_t *a = A.aux + (size_t)s * kExAux;
    const int first = a[0], npix = a[1], xmin = a[2], xmax = a[3], ymin = a[4], ymax = a[5];
    if (xmin < 0 || ymin < 0 || xmax >= g.w || ymax >= g.h || xmin > xmax || ymin > ymax) continue;  // no box was made
    const size_t base = (size_t)frame * (size_t)g.hw;
    const unsigned bw = (unsigned)(xmax - xmin + 1), bh = (unsigned)(ymax - ymin + 1);
    const u64 count = (u64)bw * bh;
    // lane t takes the pixels t, t + 256, ... of the box in raster order: a stride is step_r rows and step_c columns
    unsigned r = (unsigned)tid / bw, c = (unsigned)tid - r * bw;
    const unsigned step_r = kExThreads / bw, step_c = kExThreads - step_r * bw;
    u64 s0 = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    double flux = 0.0;
    float pk = -__builtin_inff(), cpk = -__builtin_inff();
    int cidx = INT_MAX, range = 0;
    for (u64 j = tid; j < count; j += kExThreads) {
      const int y = ymin + (int)r, x = xmin + (int)c;
      const int p = y * g.w + x;
      if (A.label[base + p] == first) {
        const float v = A.snr[base + p], d = A.data[base + p];
        if (!(v < kExSnrLimit)) {
          range = 1;
        } else {
          const u64 q = (u64)(long long)rint((double)v * kExFix);
          const u64 dx = c, dy = r;
          s0 += q;
          sx += q * dx;
          sy += q * dy;
          sxx += q * dx * dx;
          syy += q * dy * dy;
          sxy += q * dx * dy;
        }
        if (v > cpk) {  // the lane meets its pixels in raster order: the first of equals stays
          cpk = v;
          cidx = p;
        }
        if (__builtin_isfinite(d)) {
          pk = fmaxf(pk, d);
          flux += (double)d;
        }
      }
      r += step_r;
      c += step_c;
      if (c >= bw) {
        c -= bw;
        ++r;
      }
    }
    s0 = block_sum<kExWaves>(s0, s_u);
    sx = block_sum<kExWaves>(sx, s_u);
    sy = block_sum<kExWaves>(sy, s_u);
    sxx = block_sum<kExWaves>(sxx, s_u);
    syy = block_sum<kExWaves>(syy, s_u);
    sxy = block_sum<kExWaves>(sxy, s_u);
    flux = block_sum<kExWaves>(flux, s_d);
    // the maxima: the larger snr, of equals the earlier pixel
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const float ov = __shfl_down(cpk, o, kWave), op = __shfl_down(pk, o, kWave);
      const int oi = __shfl_down(cidx, o, kWave);
      range |= __shfl_down(range, o, kWave);
      if (ov > cpk || (ov == cpk && oi < cidx)) {
        cpk = ov;
        cidx = oi;
      }
      pk = fmaxf(pk, op);
    }
    if (lane == 0) {
      s_c[wv] = cpk;
      s_i[wv] = cidx;
      s_f[wv] = pk;
      s_r[wv] = range;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < kExWaves; ++k) {
        if (s_c[k] > cpk || (s_c[k] == cpk && s_i[k] < cidx)) {
          cpk = s_c[k];
          cidx = s_i[k];
        }
        pk = fmaxf(pk, s_f[k]);
        range |= s_r[k];
      }
      int flag = 0;
      if (bw > (unsigned)kExLargeBox || bh > (unsigned)kExLargeBox) flag |= 1;
      if (range) flag |= 2;
      if (xmin == 0 || ymin == 0 || xmax == g.w - 1 || ymax == g.h - 1) flag |= 4;
      lc_extract_object o;
      o.first = first;
      o.npix = npix;
      o.xmin = xmin;
      o.xmax = xmax;
      o.ymin = ymin;
      o.ymax = ymax;
      o.ypeak = cidx / g.w;
      o.xpeak = cidx - o.ypeak * g.w;
      o.flag = flag;
      o.pad = 0;
      o.peak = pk;
      o.cpeak = cpk;
      o.flux = flux;
      const double nan_ = __builtin_nan("");
      o.x = o.y = o.a = o.b = o.theta = nan_;
      if (!(flag & 3) && s0 > 0) {
        const double t = (double)s0, twelfth = 1.0 / 12.0;
        const double mx = (double)sx / t, my = (double)sy / t;
        const double x2 = fmax((double)sxx / t - mx * mx, twelfth), y2 = fmax((double)syy / t - my * my, twelfth);
        const double xy = (double)sxy / t - mx * my;
        const double half = 0.5 * (x2 + y2), dif = x2 - y2;
        const double root = sqrt(fmax(0.25 * (dif * dif) + xy * xy, 0.0));
        o.a = sqrt(half + root);
        o.b = sqrt(fmax(half - root, twelfth));
        o.theta = 0.5 * atan2(2.0 * xy, dif);
        o.x = (double)xmin + mx;
        o.y = (double)ymin + my;
      }
      A.objects[s] = o;
    }
    __syncthreads();
  }
}

// ---- the steps between the two extractions of lc_import_frames -----------------------------------------------------------

struct ExVarArgs {
  int K;
  size_t hw;
  const float *sub, *globalrms, *exptime;
  float *var;
};

// the reference's variance map, frame_importation.py:127-131, in float32
__global__ __launch_bounds__(kExThreads) void ex_variance_kernel(ExVarArgs A) {
  for (size_t frame = blockIdx.y; frame < (size_t)A.K; frame += gridDim.y) {
    const float t = A.exptime[frame], rt = A.globalrms[frame] * t, tt = t * t;
    for (size_t p = (size_t)blockIdx.x * kExThreads + threadIdx.x; p < A.hw; p += (size_t)gridDim.x * kExThreads) {
      const size_t off = frame * A.hw + p;
      A.var[off] = (rt * rt + fabsf(A.sub[off] * t)) / tt;
    }
  }
}

__global__ void ex_square_kernel(int K, const float *rms, float *var) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < K) var[k] = rms[k] * rms[k];
}

static bool ex_geom(int h, int w, ExGeom *g) {
  if (h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return false;
  g->h = h;
  g->w = w;
  g->tx = (w + kExTW - 1) / kExTW;
  g->ty = (h + kExTH - 1) / kExTH;
  g->hw = h * w;
  g->nblk = (unsigned)(((int64_t)h * w + kExThreads - 1) / kExThreads);
  return true;
}

bool extract_batch_fits(int K, int h, int w) {
  ExGeom g;
  const int64_t lim = (int64_t)1 << 31;
  return ex_geom(h, w, &g) && K >= 1 && (int64_t)K * g.tx * g.ty < lim && (int64_t)K * g.nblk < lim;
}

hipError_t extract_scratch(DeviceCall &call, int K, int h, int w, int max_objects, bool with_objects, ExtractBuffers *B) {
  ExGeom g;
  if (!ex_geom(h, w, &g)) return hipErrorInvalidValue;
  const size_t tot = (size_t)K * g.hw;
  hipError_t e = call.alloc(tot, &B->snr);
  if (e == hipSuccess) e = call.alloc(tot, &B->label);
  if (e == hipSuccess) e = call.alloc(tot, &B->count);
  if (e == hipSuccess) e = call.alloc((size_t)K * g.nblk, &B->block);
  if (e == hipSuccess && with_objects) e = call.alloc((size_t)K * max_objects * kExAux, &B->aux);
  return e;
}

hipError_t extract_label_launch(lc_ctx *ctx, int K, int h, int w, const lc_extract_cfg *cfg, const ExtractBuffers &B) {
  ExGeom g;
  if (!ex_geom(h, w, &g)) return hipErrorInvalidValue;
  const size_t tot = (size_t)K * g.hw;
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemsetAsync(B.count, 0, tot * sizeof(int32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(B.status, 0, (size_t)K * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  const unsigned tiles = (unsigned)K * (unsigned)(g.tx * g.ty), blocks = (unsigned)K * g.nblk;

  ExTileArgs T;
  T.g = g;
  T.data = B.data;
  T.var = B.var;
  T.var_scalar = B.var_scalar;
  T.thresh = cfg->thresh;
  T.filter = cfg->filter;
  T.snr = B.snr;
  T.label = B.label;
  T.status = B.status;
  hipLaunchKernelGGL(ex_tile_kernel, dim3(tiles), dim3(kExThreads), 0, st, T);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  ExMergeArgs M;
  M.g = g;
  M.label = B.label;
  M.status = B.status;
  hipLaunchKernelGGL(ex_merge_kernel, dim3(tiles), dim3(kExMergeThreads), 0, st, M);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  ExFlattenArgs F;
  F.g = g;
  F.label = B.label;
  F.count = B.count;
  F.status = B.status;
  hipLaunchKernelGGL(ex_flatten_kernel, dim3(blocks), dim3(kExThreads), 0, st, F);
  return hipGetLastError();
}

static ExNumberArgs ex_number_args(const ExGeom &g, int minarea, int max_objects, const ExtractBuffers &B) {
  ExNumberArgs N;
  N.g = g;
  N.minarea = minarea;
  N.max_objects = max_objects;
  N.label = B.label;
  N.count = B.count;
  N.block = B.block;
  N.status = B.status;
  N.nobj = B.nobj;
  N.aux = B.aux;
  return N;
}

hipError_t extract_count_launch(lc_ctx *ctx, int K, int h, int w, int minarea, int max_objects, const ExtractBuffers &B) {
  ExGeom g;
  if (!ex_geom(h, w, &g)) return hipErrorInvalidValue;
  const ExNumberArgs N = ex_number_args(g, minarea, max_objects, B);
  hipError_t e;
  hipLaunchKernelGGL(ex_count_kernel, dim3((unsigned)K * g.nblk), dim3(kExThreads), 0, ctx->stream, N);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(ex_scan_kernel, dim3((unsigned)K), dim3(kExThreads), 0, ctx->stream, N);
  return hipGetLastError();
}

hipError_t extract_table_launch(lc_ctx *ctx, int K, int h, int w, int minarea, int max_objects, const ExtractBuffers &B) {
  ExGeom g;
  if (!ex_geom(h, w, &g)) return hipErrorInvalidValue;
  hipStream_t st = ctx->stream;
  const unsigned blocks = (unsigned)K * g.nblk;
  const ExNumberArgs N = ex_number_args(g, minarea, max_objects, B);
  hipError_t e;
  hipLaunchKernelGGL(ex_number_kernel, dim3(blocks), dim3(kExThreads), 0, st, N);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  if (B.aux || B.segmap || B.mask) {
    ExBoxArgs X;
    X.g = g;
    X.max_objects = max_objects;
    X.label = B.label;
    X.count = B.count;
    X.aux = B.aux;
    X.segmap = B.segmap;
    X.mask = B.mask;
    hipLaunchKernelGGL(ex_box_kernel, dim3(blocks), dim3(kExThreads), 0, st, X);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (B.objects) {
    ExMeasureArgs Q;
    Q.g = g;
    Q.K = K;
    Q.max_objects = max_objects;
    Q.data = B.data;
    Q.snr = B.snr;
    Q.label = B.label;
    Q.aux = B.aux;
    Q.nobj = B.nobj;
    Q.objects = B.objects;
    const long long slots = (long long)K * max_objects;
    hipLaunchKernelGGL(ex_measure_kernel, dim3((unsigned)std::min<long long>(slots, kExMeasureBlocks)), dim3(kExThreads), 0,
                       st, Q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t extract_launch(lc_ctx *ctx, int K, int h, int w, const lc_extract_cfg *cfg, int max_objects,
                          const ExtractBuffers &B0) {
  ExtractBuffers B = B0;
  if (!B.objects) B.aux = nullptr;  // the boxes are made for the table alone
  hipError_t e = hipSuccess;
  if (B.objects) e = hipMemsetAsync(B.objects, 0, (size_t)K * max_objects * sizeof(lc_extract_object), ctx->stream);
  if (e == hipSuccess) e = extract_label_launch(ctx, K, h, w, cfg, B);
  if (e == hipSuccess) e = extract_count_launch(ctx, K, h, w, cfg->minarea, max_objects, B);
  if (e == hipSuccess) e = extract_table_launch(ctx, K, h, w, cfg->minarea, max_objects, B);
  return e;
}

const char *extract_cfg_error(const lc_extract_cfg *c) {
  if (!c) return "a missing configuration";
  if (!std::isfinite(c->thresh) || !(c->thresh > 0.0f)) return "thresh must be finite and > 0";
  if (c->minarea < 1) return "minarea < 1";
  if (c->filter != 0 && c->filter != 1) return "filter must be 0 or 1";
  return nullptr;
}

int import_check(lc_ctx *ctx, const char *who, bool pointers_ok, int K, int h, int w, const float *exptime,
                 const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg, int mask_sources_first,
                 const lc_extract_cfg *mcfg, int max_objects) {
  const std::string me(who);
  if (!pointers_ok || K < 1 || h < 1 || w < 1 || !exptime || !bcfg || max_objects < 1 || bcfg->bw < 1 || bcfg->bh < 1 ||
      !std::isfinite(bcfg->fthresh))
    LC_FAIL(ctx, LC_ERR_INVALID, me + ": invalid argument");
  for (int k = 0; k < K; ++k)
    if (!std::isfinite(exptime[k]) || !(exptime[k] > 0.0f))
      LC_FAIL(ctx, LC_ERR_INVALID, me + ": an exposure time that is not finite or not > 0");
  if (const char *why = extract_cfg_error(ecfg)) LC_FAIL(ctx, LC_ERR_INVALID, me + ": catalogue: " + why);
  if (mask_sources_first)
    if (const char *why = extract_cfg_error(mcfg)) LC_FAIL(ctx, LC_ERR_INVALID, me + ": source mask: " + why);
  if (bcfg->fthresh != 0.0f) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, me + ": fthresh other than 0 is not built");
  if (!lc_background_supported(h, w, bcfg->bw, bcfg->bh, bcfg->fw, bcfg->fh) ||
      !background_batch_fits(K, h, w, bcfg->bw, bcfg->bh))
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED,
            me + ": only the 1 x 1 and 3 x 3 filters, at most 256 meshes along an axis and 2048 in all");
  if (!lc_extract_supported(h, w) || !extract_batch_fits(K, h, w) ||
      (int64_t)K * max_objects >= ((int64_t)1 << 31) / kExAux)
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, me + ": frames of 2^31 pixels or more, or more of them than one grid takes");
  return LC_OK;
}

hipError_t import_launch(lc_ctx *ctx, int K, int h, int w, const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg,
                         int mask_sources_first, const lc_extract_cfg *mcfg, int max_objects, ImportBuffers &I) {
  const size_t hw = (size_t)h * w;
  BackgroundBuffers &G = I.G;
  ExtractBuffers &B = I.B;
  hipError_t e = background_launch(ctx, K, h, w, bcfg, G);
  if (e != hipSuccess) return e;
  if (mask_sources_first) {
    hipLaunchKernelGGL(ex_square_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, ctx->stream, K, G.globalrms, I.v0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ExtractBuffers Mk = B;  // the same scratch; no table, no segmap
    Mk.data = G.sub;
    Mk.var = nullptr;
    Mk.var_scalar = I.v0;
    Mk.objects = nullptr;
    Mk.segmap = nullptr;
    Mk.mask = I.mask;
    Mk.nobj = I.mnobj;
    Mk.status = I.mstatus;
    if ((e = extract_launch(ctx, K, h, w, mcfg, max_objects, Mk)) != hipSuccess) return e;
    G.mask = I.mask;
    if ((e = background_launch(ctx, K, h, w, bcfg, G)) != hipSuccess) return e;
  }
  ExVarArgs V;
  V.K = K;
  V.hw = hw;
  V.sub = G.sub;
  V.globalrms = G.globalrms;
  V.exptime = I.exptime;
  V.var = I.var;
  hipLaunchKernelGGL(ex_variance_kernel, dim3((unsigned)std::min<size_t>((hw + kExThreads - 1) / kExThreads, 4096), (unsigned)std::min(K, 65535)),
                     dim3(kExThreads), 0, ctx->stream, V);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  B.data = G.sub;
  B.var = I.var;
  if (I.dcfg) return deblend_launch(ctx, *I.call, K, h, w, ecfg, I.dcfg, max_objects, B);
  return extract_launch(ctx, K, h, w, ecfg, max_objects, B);
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_extract_supported(int h, int w) {
  ExGeom g;
  return ex_geom(h, w, &g) ? 1 : 0;
}

int lc_extract_frames(lc_ctx *ctx, int K, int h, int w, const float *data, const float *var, const float *var_scalar,
                      const lc_extract_cfg *cfg, int max_objects, lc_extract_object *objects, int32_t *nobj, int32_t *segmap,
                      uint8_t *mask, int32_t *status, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K < 1 || h < 1 || w < 1 || !data || (!var && !var_scalar) || !nobj || !status || max_objects < 1)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_extract_frames: invalid argument");
  if (const char *why = extract_cfg_error(cfg)) LC_FAIL(ctx, LC_ERR_INVALID, std::string("lc_extract_frames: ") + why);
  if (!lc_extract_supported(h, w) || !extract_batch_fits(K, h, w) ||
      (int64_t)K * max_objects >= ((int64_t)1 << 31) / kExAux)
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_extract_frames: frames of 2^31 pixels or more, or more of them than one grid takes");
  LC_ENTER(ctx);
  const size_t tot = (size_t)K * h * w;
  DeviceCall call(ctx);
  ExtractBuffers B;
  LC_HIP(ctx, call.upload(data, tot, &B.data));
  LC_HIP(ctx, call.upload(var, tot, &B.var));
  if (!var) LC_HIP(ctx, call.upload(var_scalar, (size_t)K, &B.var_scalar));
  LC_HIP(ctx, call.result(objects, (size_t)K * max_objects, &B.objects));
  LC_HIP(ctx, call.result(nobj, (size_t)K, &B.nobj));
  LC_HIP(ctx, call.result(segmap, tot, &B.segmap));
  LC_HIP(ctx, call.result(mask, tot, &B.mask));
  LC_HIP(ctx, call.result(status, (size_t)K, &B.status));
  LC_HIP(ctx, extract_scratch(call, K, h, w, max_objects, objects != nullptr, &B));
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, extract_launch(ctx, K, h, w, cfg, max_objects, B));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"

// lc_import_frames (dcfg null) and lc_import_frames_deblended
static int import_frames(const char *who, bool deblended, lc_ctx *ctx, int K, int h, int w, const float *data,
                         const float *exptime, const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg,
                         const lc_deblend_cfg *dcfg, int mask_sources_first, const lc_extract_cfg *mcfg, int max_objects,
                         float *sub, float *mesh_back, float *mesh_rms, float *globalback, float *globalrms,
                         int32_t *bg_status, lc_extract_object *objects, int32_t *nobj, int32_t *segmap, int32_t *ex_status,
                         float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  const bool pointers_ok = data && sub && globalback && globalrms && objects && nobj && ex_status;
  if (int rc = import_check(ctx, who, pointers_ok, K, h, w, exptime, bcfg, ecfg, mask_sources_first, mcfg, max_objects))
    return rc;
  if (deblended) {
    int code = 0;
    if (const char *why = deblend_cfg_error(dcfg, &code)) LC_FAIL(ctx, code, std::string(who) + ": " + why);
  }
  LC_ENTER(ctx);
  const size_t hw = (size_t)h * w, tot = (size_t)K * hw, meshes = (size_t)K * background_meshes(h, w, bcfg->bw, bcfg->bh);
  const std::vector<double> pivots = background_pivots();
  DeviceCall call(ctx);
  ImportBuffers I;
  BackgroundBuffers &G = I.G;
  ExtractBuffers &B = I.B;
  LC_HIP(ctx, call.upload(data, tot, &G.data));
  LC_HIP(ctx, call.upload(exptime, (size_t)K, &I.exptime));
  LC_HIP(ctx, call.upload(pivots.data(), pivots.size(), &G.cfac));
  LC_HIP(ctx, call.result(sub, tot, &G.sub));
  LC_HIP(ctx, mesh_back ? call.result(mesh_back, meshes, &G.mesh_back) : call.alloc(meshes, &G.mesh_back));
  LC_HIP(ctx, mesh_rms ? call.result(mesh_rms, meshes, &G.mesh_rms) : call.alloc(meshes, &G.mesh_rms));
  LC_HIP(ctx, call.result(globalback, (size_t)K, &G.globalback));
  LC_HIP(ctx, call.result(globalrms, (size_t)K, &G.globalrms));
  LC_HIP(ctx, call.result(bg_status, (size_t)K, &G.status));
  LC_HIP(ctx, call.alloc(meshes, &G.raw_back));
  LC_HIP(ctx, call.alloc(meshes, &G.raw_rms));
  LC_HIP(ctx, call.alloc(meshes, &G.zy));
  LC_HIP(ctx, call.result(objects, (size_t)K * max_objects, &B.objects));
  LC_HIP(ctx, call.result(nobj, (size_t)K, &B.nobj));
  LC_HIP(ctx, call.result(segmap, tot, &B.segmap));
  LC_HIP(ctx, call.result(ex_status, (size_t)K, &B.status));
  LC_HIP(ctx, extract_scratch(call, K, h, w, max_objects, true, &B));
  LC_HIP(ctx, call.alloc(tot, &I.var));
  if (mask_sources_first) {
    LC_HIP(ctx, call.alloc(tot, &I.mask));
    LC_HIP(ctx, call.alloc((size_t)K, &I.v0));
    LC_HIP(ctx, call.alloc((size_t)K, &I.mstatus));
    LC_HIP(ctx, call.alloc((size_t)K, &I.mnobj));
  }
  I.dcfg = deblended ? dcfg : nullptr;
  I.call = &call;
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, import_launch(ctx, K, h, w, bcfg, ecfg, mask_sources_first, mcfg, max_objects, I));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

extern "C" {

int lc_import_frames(lc_ctx *ctx, int K, int h, int w, const float *data, const float *exptime,
                     const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg, int mask_sources_first,
                     const lc_extract_cfg *mcfg, int max_objects, float *sub, float *mesh_back, float *mesh_rms,
                     float *globalback, float *globalrms, int32_t *bg_status, lc_extract_object *objects, int32_t *nobj,
                     int32_t *segmap, int32_t *ex_status, float *kernel_ms) {
  return import_frames("lc_import_frames", false, ctx, K, h, w, data, exptime, bcfg, ecfg, nullptr, mask_sources_first, mcfg,
                       max_objects, sub, mesh_back, mesh_rms, globalback, globalrms, bg_status, objects, nobj, segmap,
                       ex_status, kernel_ms);
}

int lc_import_frames_deblended(lc_ctx *ctx, int K, int h, int w, const float *data, const float *exptime,
                               const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg, const lc_deblend_cfg *dcfg,
                               int mask_sources_first, const lc_extract_cfg *mcfg, int max_objects, float *sub,
                               float *mesh_back, float *mesh_rms, float *globalback, float *globalrms, int32_t *bg_status,
                               lc_extract_object *objects, int32_t *nobj, int32_t *segmap, int32_t *ex_status,
                               float *kernel_ms) {
  return import_frames("lc_import_frames_deblended", true, ctx, K, h, w, data, exptime, bcfg, ecfg, dcfg, mask_sources_first,
                       mcfg, max_objects, sub, mesh_back, mesh_rms, globalback, globalrms, bg_status, objects, nobj, segmap,
                       ex_status, kernel_ms);
}

}  // extern "C"
