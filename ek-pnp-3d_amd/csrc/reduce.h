// reduce.h — the wave64 / workgroup reductions of the diagnostics (diag.hip, monitor.hip; private).
// DPP/permute shuffles (__shfl_down), one LDS slot per wave, fixed trees: no atomics, deterministic run to run.
#pragma once
#include <hip/hip_runtime.h>

namespace ekpnp {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

template <bool IS_MAX>
__device__ __forceinline__ double block_reduce(double v, double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = IS_MAX ? wave_max(v) : wave_sum(v);
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double r = IS_MAX ? -1.0e300 : 0.0;
  if (wave == 0) {
    r = lane < nw ? lds[lane] : (IS_MAX ? -1.0e300 : 0.0);
    r = IS_MAX ? wave_max(r) : wave_sum(r);
  }
  return r;  // valid in thread 0
}

}  // namespace ekpnp
