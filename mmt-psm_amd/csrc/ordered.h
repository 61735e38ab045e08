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

// The wide form, for many values over few partials (the stem weight gradient: ten thousand values over at most 512 partials; one
// block per value would be ten thousand blocks of which each reads at most two floats per thread).
// One thread owns four consecutive workspace values: it walks the partials in ascending order with 16-byte loads -- a wave reads
// 1 KB in a row of each partial -- and accumulates each sum into dst[map(quad, e)]; a negative index is a workspace slot that
// carries no value (padding columns of a tile).  The workspace's order of values is the stage-one kernel's to choose (the order
// in which its accumulators store whole rows); `map` undoes it.  Who uses which form follows from (blocks, nv) alone: a caller
// whose nv is in the thousands by construction uses this one.
template <class Map>
static __global__ __launch_bounds__(256) void ordered_finish_wide_kernel(const float* __restrict__ ws, int blocks, long nq,
                                                                         float* __restrict__ dst, Map map) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(ws) + q;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int b = 0;
  for (; b + 4 <= blocks; b += 4) {   // four loads in flight, added in ascending order
    const f32x4 v0 = p[(long)b * nq], v1 = p[(long)(b + 1) * nq], v2 = p[(long)(b + 2) * nq], v3 = p[(long)(b + 3) * nq];
    s += v0; s += v1; s += v2; s += v3;
  }
  for (; b < blocks; ++b) s += p[(long)b * nq];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long d = map(q, e);
    if (d >= 0) dst[d] += s[e];
  }
}

// nv values (a multiple of 4) per partial, `blocks` partials
template <class Map>
static inline int ordered_finish_wide(const float* ws, int blocks, long nv, float* dst, Map map, hipStream_t s) {
  const long nq = nv / 4;
  hipLaunchKernelGGL((ordered_finish_wide_kernel<Map>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, ws, blocks, nq, dst, map);
  MMT_LAUNCH_CHECK();
  return 0;
}
