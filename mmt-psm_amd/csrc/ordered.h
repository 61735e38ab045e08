// Second stage of the two-stage reductions of deterministic mode (include/mmtpsm.h: mmt_set_deterministic).  Stage one is the
// reducing kernel itself: instead of one float atomic per block it stores its block's partial sums at ws[block * nv + v].  Stage two
// (here) adds them in an order that depends on the block count alone and accumulates into the destination.  A second small launch,
// not a "last block finishes" form: device-scope fences measured slower.
#pragma once
#include "common.h"

// dst[v] += sum_b ws[b * nv + v].  One block per value: thread t adds blocks t, t + 256, ... in ascending order, the 64 lanes of a wave
// meet in the xor butterfly (the same tree on every lane, whatever the timing), the four waves are added in wave order.
static __global__ __launch_bounds__(256) void ordered_finish_kernel(const float* __restrict__ ws, int blocks, int nv,
                                                                    float* __restrict__ dst) {
  const int v = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < blocks; b += 256) s += ws[(long)b * nv + v];
  s = wave_sum(s);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) dst[v] += (red[0] + red[1]) + (red[2] + red[3]);
}

static inline int ordered_finish(const float* ws, int blocks, int nv, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(ordered_finish_kernel, dim3(nv), dim3(256), 0, s, ws, blocks, nv, dst);
  MMT_LAUNCH_CHECK();
  return 0;
}
