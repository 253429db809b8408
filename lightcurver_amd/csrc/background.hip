// Sky background of whole frames: SExtractor's mesh background (the algorithm behind sep.Background, which the reference's
// subtract_background calls at lightcurver/processes/background_estimation.py:25), frozen as the SPEC of DESIGN.md §5
// "Sky background" and restated in NumPy by tests/_background.py.  K frames of one shape per call, three launches:
//   bg_stats_kernel  one workgroup of 1024 per (frame, mesh): moments, clipped moments and histogram in three streaming passes,
//                    then the mode of the histogram (steps 3 - 5);
//   bg_post_kernel   one workgroup per frame: bad meshes, median filter, global values, y-direction spline (steps 6 - 9);
//   bg_map_kernel    one workgroup per (frame, block of lines): node values and x-direction spline per line, then the
//                    streaming read of the frame and write of sub and / or back (steps 9 - 10).
// Every floating sum is a reduction in a fixed order over a fixed assignment of pixels to lanes, and the histogram is
// built with integer adds, so a frame's result does not depend on K, on its place in the batch or on the run.
#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

#include <algorithm>
#include <cstring>
#include <vector>

#include "block_reduce.h"
#include "device_call.h"
#include "frame_steps.h"
#include "lc_common.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kBgThreads = 256;
constexpr int kBgMaxLevels = 4096;  // SExtractor's QUANTIF_NMAXLEVELS: 16 KiB of LDS as u32
constexpr int kBgStatThreads = 1024;  // bg_stats_kernel: a mesh is walked three times, by as many lanes as a workgroup has
constexpr int kBgStatWaves = kBgStatThreads / kWave;
constexpr int kBgBinsPerLane = kBgMaxLevels / kBgStatThreads;
constexpr int kBgMaxMeshes = 2048;  // what bg_post_kernel holds in LDS
constexpr int kBgMaxAxis = 256;     // nodes per line in the LDS of bg_map_kernel
constexpr int kBgLines = 4;         // image lines per workgroup of bg_map_kernel

struct BgGrid {
  int h, w, bw, bh, nx, ny;
};

typedef unsigned long long u64;

struct BgStatArgs {
  BgGrid g;
  const float *data;
  const uint8_t *mask;
  float *raw_back, *raw_rms;  // [K][ny][nx], NaN = bad mesh
};

__global__ __launch_bounds__(kBgStatThreads) void bg_stats_kernel(BgStatArgs A) {
  __shared__ unsigned s_hist[kBgMaxLevels], s_scan[kBgMaxLevels];
  __shared__ unsigned s_lane[kBgStatThreads];
  __shared__ double s_pd[kBgStatWaves];
  __shared__ u64 s_pu[kBgStatWaves];
  const BgGrid g = A.g;
  const int tid = threadIdx.x;
  const unsigned meshes = (unsigned)(g.nx * g.ny);
  const unsigned frame = blockIdx.x / meshes, m = blockIdx.x - frame * meshes;
  const int my = (int)(m / (unsigned)g.nx), mx = (int)m - my * g.nx;
  const int x0 = mx * g.bw, y0 = my * g.bh;
  const unsigned mw = (unsigned)min(g.bw, g.w - x0), mh = (unsigned)min(g.bh, g.h - y0);
  const unsigned count = mw * mh;  // < 2^31: checked on the host
  const size_t base = ((size_t)frame * g.h + y0) * g.w + x0;
  const size_t out = (size_t)frame * meshes + m;
  const float nanf_ = __builtin_nanf("");

  // Lane t takes the pixels t, t + 1024, ... of the mesh in raster order.  Their rows and columns follow from one
  // division per lane: a stride of kBgStatThreads pixels is step_r rows and step_c columns, with at most one carry.
  const unsigned row0 = (unsigned)tid / mw, col0 = (unsigned)tid - row0 * mw;
  const unsigned step_r = kBgStatThreads / mw, step_c = kBgStatThreads - step_r * mw;
  // all pixels of this lane in that order: fn(value, good), good as step 2 defines it
  const auto each_pixel = [&](auto &&fn) {
    unsigned r = row0, c = col0;
    for (unsigned p = tid; p < count; p += kBgStatThreads) {
      const size_t off = base + (size_t)r * g.w + c;
      const float v = A.data[off];
      fn(v, __builtin_isfinite(v) && !(A.mask && A.mask[off]));
      r += step_r;
      c += step_c;
      if (c >= mw) {
        c -= mw;
        ++r;
      }
    }
  };

  // step 3, first pass: moments of the good pixels
  double sum = 0.0, sq = 0.0;
  u64 n = 0;
  each_pixel([&](float v, bool good) {
    if (good) {
      sum += (double)v;
      sq += (double)v * (double)v;
      ++n;
    }
  });
  sum = block_sum<kBgStatWaves>(sum, s_pd);
  sq = block_sum<kBgStatWaves>(sq, s_pd);
  n = block_sum<kBgStatWaves>(n, s_pu);
  if (2 * n < (u64)count) {  // fewer good pixels than half of the mesh: bad
    if (tid == 0) A.raw_back[out] = A.raw_rms[out] = nanf_;
    return;
  }
  double mean = sum / (double)n, var = sq / (double)n - mean * mean;
  double sigma = var > 0.0 ? sqrt(var) : 0.0;
  const float lcut = (float)(mean - 2.0 * sigma), hcut = (float)(mean + 2.0 * sigma);

  // second pass: moments inside [lcut, hcut]
  sum = sq = 0.0;
  n = 0;
  each_pixel([&](float v, bool good) {
    if (good && v >= lcut && v <= hcut) {
      sum += (double)v;
      sq += (double)v * (double)v;
      ++n;
    }
  });
  sum = block_sum<kBgStatWaves>(sum, s_pd);
  sq = block_sum<kBgStatWaves>(sq, s_pd);
  n = block_sum<kBgStatWaves>(n, s_pu);
  if (n == 0) {  // nothing inside the cuts (this project's rule): bad
    if (tid == 0) A.raw_back[out] = A.raw_rms[out] = nanf_;
    return;
  }
  mean = sum / (double)n;
  var = sq / (double)n - mean * mean;
  sigma = var > 0.0 ? sqrt(var) : 0.0;
  const double step = 0.79788456080286541 * 5.0 / 4.0;  // sqrt(2 / pi) QUANTIF_NSIGMA / QUANTIF_AMIN
  const double flev = step * (double)n + 1.0;
  const int nlev = flev < (double)kBgMaxLevels ? (int)flev : kBgMaxLevels;
  const float qscale = sigma > 0.0 ? (float)(2.0 * 5.0 * sigma / (double)nlev) : 1.0f;
  const float qzero = (float)(mean - 5.0 * sigma);

  // step 4: histogram of all good pixels, integer adds in LDS
  for (int i = tid; i < kBgMaxLevels; i += kBgStatThreads) s_hist[i] = 0;
  __syncthreads();
  const float cste = 0.499999f - qzero / qscale, top = (float)nlev;
  each_pixel([&](float v, bool good) {
    if (good) {
      const float b = v / qscale + cste;
      if (b > -1.0f && b < top) atomicAdd(&s_hist[(int)b], 1u);  // (int) truncates: bin 0 takes -1 < b < 1
    }
  });
  __syncthreads();

  // inclusive scan of the bins: lane t holds bins 4 t .. 4 t + 3
  {
    unsigned mine = 0;
#pragma unroll
    for (int i = 0; i < kBgBinsPerLane; ++i) mine += s_hist[tid * kBgBinsPerLane + i];
    const unsigned incl = wave_inclusive_scan(mine);
    s_lane[tid] = incl;
    __syncthreads();
    unsigned before = incl - mine;
    for (int wv = 0; wv < tid / kWave; ++wv) before += s_lane[wv * kWave + kWave - 1];
#pragma unroll
    for (int i = 0; i < kBgBinsPerLane; ++i) {
      before += s_hist[tid * kBgBinsPerLane + i];
      s_scan[tid * kBgBinsPerLane + i] = before;
    }
    __syncthreads();
  }
  const auto cum = [&](int i) -> unsigned { return i < 0 ? 0u : s_scan[min(i, kBgMaxLevels - 1)]; };
  const auto bin = [&](int i) -> unsigned { return i < 0 || i >= kBgMaxLevels ? 0u : s_hist[i]; };

  // step 5: every lane carries the same state; the walk's end state comes from the merge-path search over the scan
  int lo_cut = 0, hi_cut = nlev - 1;
  double sig = 10.0 * (double)(nlev - 1), sig1 = 1.0, mea = 0.0, med = 0.0;  // mea, med: set by the first round
  bool ran = false;
  for (int round = 100; round-- && sig >= 0.1 && fabs(sig / sig1 - 1.0) > 1e-4;) {
    ran = true;
    sig1 = sig;
    const int T = max(hi_cut - lo_cut + 1, 0);
    int a = 0;
    if (T > 0) {
      // a = low-end bins among the first T of the merge of P[i] = cum from the low end and Q[j] = cum from the high
      // end, ties to Q: P[mid] precedes Q[T - 1 - mid] exactly when more than mid low-end bins are taken
      int lo = 0, hi = T;
      const unsigned c0 = cum(lo_cut - 1), c1 = cum(hi_cut);
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned P = cum(lo_cut + mid - 1) - c0, Q = c1 - cum(hi_cut - (T - 1 - mid));
        if (P < Q) lo = mid + 1;
        else hi = mid;
      }
      a = lo;
    }
    const int b = T - a, ilo = lo_cut + a, ihi = hi_cut - b;
    const unsigned lowsum = T > 0 ? cum(ilo - 1) - cum(lo_cut - 1) : 0u;
    const unsigned highsum = T > 0 ? cum(hi_cut) - cum(ihi) : 0u;
    const unsigned peak = max(bin(ilo), bin(ihi));
    med = ihi >= 0 ? (double)ihi + 0.5 + (peak > 0 ? ((double)highsum - (double)lowsum) / (2.0 * (double)peak) : 0.0) : 0.0;
    const unsigned total = T > 0 ? cum(hi_cut) - cum(lo_cut - 1) : 0u;
    u64 s1 = 0, s2 = 0;
    for (int i = lo_cut + tid; i <= hi_cut; i += kBgStatThreads) {
      const u64 c = s_hist[i], ci = c * (u64)i;
      s1 += ci;
      s2 += ci * (u64)i;
    }
    s1 = block_sum<kBgStatWaves>(s1, s_pu);
    s2 = block_sum<kBgStatWaves>(s2, s_pu);
    if (total) {
      mea = (double)s1 / (double)total;
      sig = (double)s2 / (double)total - mea * mea;
    } else {
      mea = sig = 0.0;
    }
    sig = sig > 0.0 ? sqrt(sig) : 0.0;
    double f = med - 3.0 * sig;
    lo_cut = f > 0.0 ? (int)(f + 0.5) : 0;
    f = med + 3.0 * sig;
    hi_cut = f < (double)(nlev - 1) ? (int)(f > 0.0 ? f + 0.5 : f - 0.5) : nlev - 1;
  }
  if (tid == 0) {
    const double qz = (double)qzero, qs = (double)qscale;
    double back;
    if (!ran)  // one level (one pixel inside the cuts): no round has run; the moments of step 3 are the result
      back = mean;
    else if (sig > 0.0)
      back = fabs((mea - med) / sig) < 0.3 ? qz + (2.5 * med - 1.5 * mea) * qs : qz + med * qs;
    else
      back = qz + mea * qs;
    A.raw_back[out] = (float)back;
    A.raw_rms[out] = (float)(ran ? sig * qs : sigma);
  }
}

// z = y'' / 6 of the natural cubic spline through ny nodes of unit spacing, down mesh column j: z[k-1] + 4 z[k] + z[k+1] =
// y[k-1] - 2 y[k] + y[k+1], z = 0 at both ends, by the Thomas sweep in double with the table cfac[k] = 1 / (4 - cfac[k-1]).
// y and z are [ny][nx] float, d is a scratch of [ny][nx] doubles.
__device__ __forceinline__ void bg_spline_column(const float *y, float *z, double *d, const double *cfac, int ny, int nx,
                                                 int j) {
  if (ny < 3) {
    for (int k = 0; k < ny; ++k) z[k * nx + j] = 0.0f;
    return;
  }
  d[j] = 0.0;
  for (int k = 1; k < ny - 1; ++k) {
    const double r = ((double)y[(k - 1) * nx + j] - 2.0 * (double)y[k * nx + j]) + (double)y[(k + 1) * nx + j];
    d[k * nx + j] = (r - d[(k - 1) * nx + j]) * cfac[k];
  }
  double zk = 0.0;
  z[(ny - 1) * nx + j] = 0.0f;
  for (int k = ny - 2; k >= 1; --k) {
    zk = d[k * nx + j] - cfac[k] * zk;
    z[k * nx + j] = (float)zk;
  }
  z[j] = 0.0f;
}

__device__ __forceinline__ void bg_swap_up(float &a, float &b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// Median of the (2 ax + 1)(2 ay + 1) values of v around mesh (px, py), ax and ay 0 or 1: 1, 3 or 9 of them.  Nine slots
// with fixed indices, so they stay in registers: the slots outside the window (an even number) take -inf and +inf in
// turn, which leaves the median of the nine the median of the window.
__device__ __forceinline__ float bg_window_median(const float *v, int nx, int px, int py, int ax, int ay) {
  float t[9];
  int outside = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const bool in = abs(dx) <= ax && abs(dy) <= ay;
      const float pad = (outside & 1) ? __builtin_inff() : -__builtin_inff();
      const float inside = v[in ? (py + dy) * nx + px + dx : py * nx + px];  // never an index outside the grid
      t[(dy + 1) * 3 + dx + 1] = in ? inside : pad;
      outside += !in;
    }
#pragma unroll
  for (int i = 1; i < 9; ++i)
#pragma unroll
    for (int k = i; k > 0; --k) bg_swap_up(t[k - 1], t[k]);
  return t[4];
}

// ascending bitonic sort of s[0 .. P), P a power of two
__device__ __forceinline__ void bg_sort(float *s, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += kBgThreads) {
        const int o = i ^ j;
        if (o > i) {
          const float a = s[i], b = s[o];
          if ((a > b) == ((i & k) == 0)) {
            s[i] = b;
            s[o] = a;
          }
        }
      }
      __syncthreads();
    }
}

// median of the sorted s[first .. first + count): the mean of the two middle values for an even count
__device__ __forceinline__ float bg_sorted_median(const float *s, int first, int count) {
  return count & 1 ? s[first + count / 2] : (s[first + count / 2 - 1] + s[first + count / 2]) / 2.0f;
}

struct BgPostArgs {
  BgGrid g;
  int fw, fh;
  const float *raw_back, *raw_rms;
  const double *cfac;
  float *mesh_back, *mesh_rms, *zy;  // [K][ny][nx]
  float *globalback, *globalrms;     // [K]
  int32_t *status;                   // [K], may be null
};

__global__ __launch_bounds__(kBgThreads) void bg_post_kernel(BgPostArgs A) {
  __shared__ float s_b[kBgMaxMeshes], s_r[kBgMaxMeshes], s_b2[kBgMaxMeshes], s_r2[kBgMaxMeshes], s_sort[kBgMaxMeshes];
  __shared__ double s_d[kBgMaxMeshes];
  const BgGrid g = A.g;
  const int nx = g.nx, ny = g.ny, M = nx * ny, tid = threadIdx.x;
  const size_t off = (size_t)blockIdx.x * M;
  int good = 0;
  for (int i = tid; i < M; i += kBgThreads) {
    s_b[i] = A.raw_back[off + i];
    s_r[i] = A.raw_rms[off + i];
    good |= s_b[i] == s_b[i];
  }
  if (!__syncthreads_or(good)) {  // not one good mesh: the frame reports it and the batch goes on
    const float nanf_ = __builtin_nanf("");
    for (int i = tid; i < M; i += kBgThreads) A.mesh_back[off + i] = A.mesh_rms[off + i] = A.zy[off + i] = nanf_;
    if (tid == 0) {
      A.globalback[blockIdx.x] = A.globalrms[blockIdx.x] = nanf_;
      if (A.status) A.status[blockIdx.x] = LC_ERR_NONFINITE;
    }
    return;
  }
  // step 6: a bad mesh takes the mean of the good meshes at the smallest squared distance, summed in raster order
  for (int i = tid; i < M; i += kBgThreads) {
    float vb = s_b[i], vr = s_r[i];
    if (vb != vb) {
      const int py = i / nx, px = i - py * nx;
      int best = 0x7fffffff, cnt = 0;
      for (int j = 0; j < M; ++j) {
        const float bj = s_b[j];
        if (bj != bj) continue;
        const int y = j / nx, x = j - y * nx, d2 = (x - px) * (x - px) + (y - py) * (y - py);
        if (d2 < best) {
          best = d2;
          vb = bj;
          vr = s_r[j];
          cnt = 1;
        } else if (d2 == best) {
          vb += bj;
          vr += s_r[j];
          ++cnt;
        }
      }
      vb /= (float)cnt;
      vr /= (float)cnt;
    }
    s_b2[i] = vb;
    s_r2[i] = vr;
  }
  __syncthreads();
  // step 7: median filter; at the grid edge the window shrinks on both sides, as SExtractor's does
  for (int i = tid; i < M; i += kBgThreads) {
    const int py = i / nx, px = i - py * nx;
    const int ax = min(A.fw / 2, min(px, nx - 1 - px)), ay = min(A.fh / 2, min(py, ny - 1 - py));
    s_b[i] = bg_window_median(s_b2, nx, px, py, ax, ay);
    s_r[i] = bg_window_median(s_r2, nx, px, py, ax, ay);
  }
  __syncthreads();
  // step 8: the global values
  int P = 1;
  while (P < M) P <<= 1;
  for (int i = tid; i < P; i += kBgThreads) s_sort[i] = i < M ? s_b[i] : __builtin_inff();
  __syncthreads();
  bg_sort(s_sort, P);
  const float gback = bg_sorted_median(s_sort, 0, M);
  __syncthreads();
  for (int i = tid; i < P; i += kBgThreads) s_sort[i] = i < M ? s_r[i] : __builtin_inff();
  __syncthreads();
  bg_sort(s_sort, P);
  float grms = bg_sorted_median(s_sort, 0, M);
  if (grms <= 0.0f) {
    // the positive ones are the tail of the sorted values
    int first = 0;
    while (first < M && !(s_sort[first] > 0.0f)) ++first;
    if (first < M) grms = bg_sorted_median(s_sort, first, M - first);
  }
  for (int i = tid; i < M; i += kBgThreads) {
    A.mesh_back[off + i] = s_b[i];
    A.mesh_rms[off + i] = s_r[i];
  }
  if (tid == 0) {
    A.globalback[blockIdx.x] = gback;
    A.globalrms[blockIdx.x] = grms;
    if (A.status) A.status[blockIdx.x] = LC_OK;
  }
  // step 9, along y: one lane per mesh column
  for (int j = tid; j < nx; j += kBgThreads) bg_spline_column(s_b, A.zy + off, s_d, A.cfac, ny, nx, j);
}

// the y-direction spline alone, for mesh values that come from the host (lc_background_map)
struct BgColumnArgs {
  BgGrid g;
  const float *mesh;
  const double *cfac;
  float *zy;
};

__global__ __launch_bounds__(kBgThreads) void bg_column_kernel(BgColumnArgs A) {
  __shared__ double s_d[kBgMaxMeshes];
  const size_t off = (size_t)blockIdx.x * A.g.nx * A.g.ny;
  for (int j = threadIdx.x; j < A.g.nx; j += kBgThreads)
    bg_spline_column(A.mesh + off, A.zy + off, s_d, A.cfac, A.g.ny, A.g.nx, j);
}

// the cubic piece between nodes k and k + 1 at t = k + B, continued beyond the first and the last node
__device__ __forceinline__ float bg_cubic(float y0, float y1, float z0, float z1, float B) {
  const float A = 1.0f - B;
  return A * y0 + B * y1 + (A * A * A - A) * z0 + (B * B * B - B) * z1;
}

// node coordinate of pixel p for meshes of b pixels, the piece k it lies in (of n >= 2 nodes) and its offset B in it
__device__ __forceinline__ int bg_piece(int p, int b, int n, float &B) {
  const float t = ((float)p + 0.5f) / (float)b - 0.5f;
  const int k = min(max((int)floorf(t), 0), n - 2);
  B = t - (float)k;
  return k;
}

struct BgMapArgs {
  BgGrid g;
  unsigned blocks_per_frame;
  const float *data;  // null: back alone
  const float *mesh, *zy;
  const double *cfac;
  float *sub, *back;
};

__global__ __launch_bounds__(kBgThreads) void bg_map_kernel(BgMapArgs A) {
  __shared__ __align__(16) float s_node[kBgLines][kBgMaxAxis], s_z[kBgLines][kBgMaxAxis];
  __shared__ double s_d[kBgLines][kBgMaxAxis];
  const BgGrid g = A.g;
  const int nx = g.nx, ny = g.ny, tid = threadIdx.x;
  const unsigned frame = blockIdx.x / A.blocks_per_frame, lb = blockIdx.x - frame * A.blocks_per_frame;
  const int y0 = (int)lb * kBgLines, lines = min(kBgLines, g.h - y0);
  const float *mesh = A.mesh + (size_t)frame * nx * ny, *zy = A.zy + (size_t)frame * nx * ny;

  // the node values of each line: the y-direction spline evaluated at the line, per mesh column
  for (int i = tid; i < lines * nx; i += kBgThreads) {
    const int l = i / nx, j = i - l * nx;
    float v = mesh[j];
    if (ny > 1) {
      float B;
      const int k = bg_piece(y0 + l, g.bh, ny, B);
      v = bg_cubic(mesh[k * nx + j], mesh[(k + 1) * nx + j], zy[k * nx + j], zy[(k + 1) * nx + j], B);
    }
    s_node[l][j] = v;
  }
  __syncthreads();
  // the x-direction spline through the nodes of each line
  if (tid < lines) {
    float *y = s_node[tid], *z = s_z[tid];
    double *d = s_d[tid];
    if (nx < 3) {
      for (int k = 0; k < nx; ++k) z[k] = 0.0f;
    } else {
      d[0] = 0.0;
      for (int k = 1; k < nx - 1; ++k) {
        const double r = ((double)y[k - 1] - 2.0 * (double)y[k]) + (double)y[k + 1];
        d[k] = (r - d[k - 1]) * A.cfac[k];
      }
      double zk = 0.0;
      z[nx - 1] = 0.0f;
      for (int k = nx - 2; k >= 1; --k) {
        zk = d[k] - A.cfac[k] * zk;
        z[k] = (float)zk;
      }
      z[0] = 0.0f;
    }
  }
  __syncthreads();

  for (int l = 0; l < lines; ++l) {
    const float *node = s_node[l], *z = s_z[l];
    const auto value = [&](int x) -> float {
      if (nx == 1) return node[0];
      float B;
      const int k = bg_piece(x, g.bw, nx, B);
      return bg_cubic(node[k], node[k + 1], z[k], z[k + 1], B);
    };
    const auto one = [&](size_t p, int x) {
      const float b = value(x);
      if (A.back) A.back[p] = b;
      if (A.sub) A.sub[p] = A.data[p] - b;
    };
    const size_t row = ((size_t)frame * g.h + (y0 + l)) * g.w;
    // the line as a scalar head up to the next 16-byte boundary, 128-bit accesses, and a scalar tail
    const int head = min((int)((4 - (row & 3)) & 3), g.w), quads = (g.w - head) / 4, tail = head + 4 * quads;
    for (int x = tid; x < head; x += kBgThreads) one(row + x, x);
    for (int q = tid; q < quads; q += kBgThreads) {
      const int x = head + 4 * q;
      const size_t p = row + x;
      float4 b;
      b.x = value(x);
      b.y = value(x + 1);
      b.z = value(x + 2);
      b.w = value(x + 3);
      if (A.sub) {
        const float4 d = *reinterpret_cast<const float4 *>(A.data + p);
        float4 s;
        s.x = d.x - b.x;
        s.y = d.y - b.y;
        s.z = d.z - b.z;
        s.w = d.w - b.w;
        *reinterpret_cast<float4 *>(A.sub + p) = s;
      }
      if (A.back) *reinterpret_cast<float4 *>(A.back + p) = b;
    }
    for (int x = tail + tid; x < g.w; x += kBgThreads) one(row + x, x);
  }
}

static bool bg_grid(int h, int w, int bw, int bh, BgGrid *g) {
  if (h < 1 || w < 1 || bw < 1 || bh < 1) return false;
  g->h = h;
  g->w = w;
  g->bw = bw;
  g->bh = bh;
  g->nx = (w - 1) / bw + 1;
  g->ny = (h - 1) / bh + 1;
  return true;
}

static bool bg_grid_supported(const BgGrid &g) {
  return g.nx <= kBgMaxAxis && g.ny <= kBgMaxAxis && g.nx * g.ny <= kBgMaxMeshes &&
         (int64_t)std::min(g.bw, g.w) * std::min(g.bh, g.h) < ((int64_t)1 << 31);
}

// cfac[k] = 1 / (4 - cfac[k - 1]), cfac[0] = 0: the pivots of the Thomas sweep, the same for every spline
static std::vector<double> bg_pivots() {
  std::vector<double> c(kBgMaxAxis, 0.0);
  for (int k = 1; k < kBgMaxAxis; ++k) c[k] = 1.0 / (4.0 - c[k - 1]);
  return c;
}

static unsigned bg_map_blocks(const BgGrid &g) { return (unsigned)((g.h + kBgLines - 1) / kBgLines); }

static hipError_t bg_map_launch(lc_ctx *ctx, int K, const BgGrid &g, const float *data, const float *mesh, const float *zy,
                                const double *cfac, float *sub, float *back) {
  BgMapArgs M;
  M.g = g;
  M.blocks_per_frame = bg_map_blocks(g);
  M.data = data;
  M.mesh = mesh;
  M.zy = zy;
  M.cfac = cfac;
  M.sub = sub;
  M.back = back;
  hipLaunchKernelGGL(bg_map_kernel, dim3(M.blocks_per_frame * (unsigned)K), dim3(kBgThreads), 0, ctx->stream, M);
  return hipGetLastError();
}

// K frames in one grid: both products stay below 2^31
static bool bg_batch_fits(int K, const BgGrid &g) {
  const int64_t lim = (int64_t)1 << 31;
  return (int64_t)K * g.nx * g.ny < lim && (int64_t)K * bg_map_blocks(g) < lim;
}

std::vector<double> background_pivots() { return bg_pivots(); }

size_t background_meshes(int h, int w, int bw, int bh) {
  BgGrid g;
  return bg_grid(h, w, bw, bh, &g) ? (size_t)g.nx * g.ny : 0;
}

bool background_batch_fits(int K, int h, int w, int bw, int bh) {
  BgGrid g;
  return bg_grid(h, w, bw, bh, &g) && bg_batch_fits(K, g);
}

hipError_t background_launch(lc_ctx *ctx, int K, int h, int w, const lc_background_cfg *cfg, const BackgroundBuffers &B) {
  BgGrid g;
  if (!bg_grid(h, w, cfg->bw, cfg->bh, &g)) return hipErrorInvalidValue;
  const size_t meshes = (size_t)K * g.nx * g.ny;
  BgStatArgs S;
  S.g = g;
  S.data = B.data;
  S.mask = B.mask;
  S.raw_back = B.raw_back;
  S.raw_rms = B.raw_rms;
  hipLaunchKernelGGL(bg_stats_kernel, dim3((unsigned)meshes), dim3(kBgStatThreads), 0, ctx->stream, S);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  BgPostArgs P;
  P.g = g;
  P.fw = cfg->fw;
  P.fh = cfg->fh;
  P.raw_back = B.raw_back;
  P.raw_rms = B.raw_rms;
  P.cfac = B.cfac;
  P.mesh_back = B.mesh_back;
  P.mesh_rms = B.mesh_rms;
  P.zy = B.zy;
  P.globalback = B.globalback;
  P.globalrms = B.globalrms;
  P.status = B.status;
  hipLaunchKernelGGL(bg_post_kernel, dim3((unsigned)K), dim3(kBgThreads), 0, ctx->stream, P);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (B.sub || B.back) e = bg_map_launch(ctx, K, g, B.data, B.mesh_back, B.zy, B.cfac, B.sub, B.back);
  return e;
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_background_supported(int h, int w, int bw, int bh, int fw, int fh) {
  BgGrid g;
  if (!bg_grid(h, w, bw, bh, &g)) return 0;
  return fw == fh && (fw == 1 || fw == 3) && bg_grid_supported(g) ? 1 : 0;
}

int lc_background_frames(lc_ctx *ctx, int K, int h, int w, const float *data, const uint8_t *mask,
                         const lc_background_cfg *cfg, float *sub, float *back, float *mesh_back, float *mesh_rms,
                         float *globalback, float *globalrms, int32_t *status, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  BgGrid g;
  if (K < 1 || !data || !cfg || !globalback || !globalrms || !bg_grid(h, w, cfg->bw, cfg->bh, &g) ||
      !std::isfinite(cfg->fthresh))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_background_frames: invalid argument");
  if (cfg->fthresh != 0.0f) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_background_frames: fthresh other than 0 is not built");
  if (cfg->fw != cfg->fh || (cfg->fw != 1 && cfg->fw != 3))
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_background_frames: only the 1 x 1 and 3 x 3 filters are built");
  if (!bg_grid_supported(g) || !bg_batch_fits(K, g))
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_background_frames: more meshes than 256 along an axis or 2048 in all");
  LC_ENTER(ctx);
  const size_t tot = (size_t)K * h * w, meshes = (size_t)K * g.nx * g.ny;
  const std::vector<double> pivots = bg_pivots();
  DeviceCall call(ctx);
  const float *d_data = nullptr;
  const uint8_t *d_mask = nullptr;
  const double *d_cfac = nullptr;
  float *d_sub = nullptr, *d_back = nullptr, *d_mb = nullptr, *d_mr = nullptr, *d_gb = nullptr, *d_gr = nullptr;
  float *d_rawb = nullptr, *d_rawr = nullptr, *d_zy = nullptr;
  int32_t *d_status = nullptr;
  LC_HIP(ctx, call.upload(data, tot, &d_data));
  LC_HIP(ctx, call.upload(mask, tot, &d_mask));
  LC_HIP(ctx, call.upload(pivots.data(), pivots.size(), &d_cfac));
  LC_HIP(ctx, call.result(sub, tot, &d_sub));
  LC_HIP(ctx, call.result(back, tot, &d_back));
  // the map reads the mesh values whether or not the caller takes them
  LC_HIP(ctx, mesh_back ? call.result(mesh_back, meshes, &d_mb) : call.alloc(meshes, &d_mb));
  LC_HIP(ctx, mesh_rms ? call.result(mesh_rms, meshes, &d_mr) : call.alloc(meshes, &d_mr));
  LC_HIP(ctx, call.result(globalback, (size_t)K, &d_gb));
  LC_HIP(ctx, call.result(globalrms, (size_t)K, &d_gr));
  LC_HIP(ctx, call.result(status, (size_t)K, &d_status));
  LC_HIP(ctx, call.alloc(meshes, &d_rawb));
  LC_HIP(ctx, call.alloc(meshes, &d_rawr));
  LC_HIP(ctx, call.alloc(meshes, &d_zy));
  LC_HIP(ctx, call.start());
  BackgroundBuffers B;
  B.data = d_data;
  B.mask = d_mask;
  B.cfac = d_cfac;
  B.sub = d_sub;
  B.back = d_back;
  B.mesh_back = d_mb;
  B.mesh_rms = d_mr;
  B.globalback = d_gb;
  B.globalrms = d_gr;
  B.status = d_status;
  B.raw_back = d_rawb;
  B.raw_rms = d_rawr;
  B.zy = d_zy;
  LC_HIP(ctx, background_launch(ctx, K, h, w, cfg, B));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

int lc_background_map(lc_ctx *ctx, int K, int h, int w, int bw, int bh, const float *mesh, float *map, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  BgGrid g;
  if (K < 1 || !mesh || !map || !bg_grid(h, w, bw, bh, &g)) LC_FAIL(ctx, LC_ERR_INVALID, "lc_background_map: invalid argument");
  if (!bg_grid_supported(g) || !bg_batch_fits(K, g))
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_background_map: more meshes than 256 along an axis or 2048 in all");
  LC_ENTER(ctx);
  const size_t tot = (size_t)K * h * w, meshes = (size_t)K * g.nx * g.ny;
  const std::vector<double> pivots = bg_pivots();
  DeviceCall call(ctx);
  const float *d_mesh = nullptr;
  const double *d_cfac = nullptr;
  float *d_map = nullptr, *d_zy = nullptr;
  LC_HIP(ctx, call.upload(mesh, meshes, &d_mesh));
  LC_HIP(ctx, call.upload(pivots.data(), pivots.size(), &d_cfac));
  LC_HIP(ctx, call.result(map, tot, &d_map));
  LC_HIP(ctx, call.alloc(meshes, &d_zy));
  LC_HIP(ctx, call.start());
  BgColumnArgs C;
  C.g = g;
  C.mesh = d_mesh;
  C.cfac = d_cfac;
  C.zy = d_zy;
  hipLaunchKernelGGL(bg_column_kernel, dim3((unsigned)K), dim3(kBgThreads), 0, ctx->stream, C);
  LC_HIP(ctx, hipGetLastError());
  LC_HIP(ctx, bg_map_launch(ctx, K, g, nullptr, d_mesh, d_zy, d_cfac, nullptr, d_map));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
