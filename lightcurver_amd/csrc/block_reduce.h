// Workgroup reductions whose order is fixed, for the kernels whose results are compared bit for bit, and the wave scan
// (device only).
#pragma once
#include "lc_common.h"

namespace lc {

// The sum over the workgroup's Waves waves, returned to every lane; part is LDS of Waves values.  The order is part of
// the contract, since callers sum float64 with it (ex_measure_kernel's flux, bg_stats_kernel's moments): within a wave a
// shuffle-down tree from kWave / 2, then part[0] + part[1] + ... in wave order.  The barrier at the end frees part for
// the next call.
template <int Waves, class T>
__device__ __forceinline__ T block_sum(T v, T *part) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = v;
  __syncthreads();
  T r = part[0];
#pragma unroll
  for (int wv = 1; wv < Waves; ++wv) r += part[wv];
  __syncthreads();
  return r;
}

// the largest unsigned value of the workgroup, returned to every lane
template <int Waves>
__device__ __forceinline__ unsigned block_max(unsigned v, unsigned *part) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_down((int)v, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = v;
  __syncthreads();
  unsigned r = part[0];
#pragma unroll
  for (int wv = 1; wv < Waves; ++wv) r = max(r, part[wv]);
  __syncthreads();
  return r;
}

// the inclusive scan of v over the lanes of a wave, returned per lane: lane l holds v of lanes 0 .. l (integers)
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const T up = __shfl_up(v, o, kWave);
    if (lane >= o) v += up;
  }
  return v;
}

}  // namespace lc
