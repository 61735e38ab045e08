// Flat-buffer optimiser and EMA kernels (HBM-bound streaming, float4 per lane, grid-stride).
//
// The host keeps every model's parameters in ONE contiguous fp32 buffer (gradients and momentum
// likewise), so the 132-tensor loops of the reference -- engine/MTtrainer.py:277-281 (EMA: 264 tiny
// launches) and torch.optim.SGD over 121 parameter groups (solver/build.py:5-23) -- become one launch
// each.  Algorithmic HBM traffic: EMA 3 x 4 B/param (read t, read s, write t); SGD 5 x 4 B/param.
#include "common.h"

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ t, const float* __restrict__ s, long n4,
                                                  long n, float alpha, float beta) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 a = ((const f32x4*)t)[i];
    const f32x4 b = ((const f32x4*)s)[i];
#pragma unroll
    for (int e = 0; e < 4; e++) a[e] = fmaf(b[e], beta, a[e] * alpha);  // mul_(alpha).add_(s, alpha=1-alpha)
    ((f32x4*)t)[i] = a;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    t[i] = fmaf(s[i], beta, t[i] * alpha);
  }
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, long n4, long n, float lr, float wd,
                                                  float mom, int first) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 w = ((f32x4*)p)[i];
    const f32x4 gr = ((const f32x4*)g)[i];
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (!first) b = ((f32x4*)buf)[i];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float d = gr[e] + wd * w[e];
      b[e] = first ? d : mom * b[e] + d;
      w[e] = w[e] - lr * b[e];
    }
    ((f32x4*)buf)[i] = b;
    ((f32x4*)p)[i] = w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    const float d = g[i] + wd * p[i];
    const float b = first ? d : mom * buf[i] + d;
    buf[i] = b;
    p[i] = p[i] - lr * b;
  }
}

static int stream_blocks(long n4) {
  long b = (n4 + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}

extern "C" int mmt_ema_update(float* teacher, const float* student, int64_t n, double alpha, void* stream) {
  if (n <= 0) return 0;
  if (((uintptr_t)teacher | (uintptr_t)student) & 15) return MMT_EINVAL;
  hipLaunchKernelGGL(ema_kernel, dim3(stream_blocks(n >> 2)), dim3(256), 0, (hipStream_t)stream, teacher, student,
                     (long)(n >> 2), (long)n, (float)alpha, (float)(1.0 - alpha));
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmt_sgd_momentum(float* p, const float* g, float* buf, int64_t n, float lr, float wd, float momentum,
                                int first, void* stream) {
  if (n <= 0) return 0;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) return MMT_EINVAL;
  hipLaunchKernelGGL(sgd_kernel, dim3(stream_blocks(n >> 2)), dim3(256), 0, (hipStream_t)stream, p, g, buf,
                     (long)(n >> 2), (long)n, lr, wd, momentum, first);
  MMT_LAUNCH_CHECK();
  return 0;
}

// ---- guarded step (include/mmtpsm.h: mmt_grad_guard).  One more read of the gradient: its sum of squares in fp64, block partials
// to ws, a second small launch that adds them in block order (csrc/ordered.h: why not a last-block finish) and settles the step's
// fate in `state` on the device; the guarded SGD kernel reads it there.  Nothing travels to the host.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the 256 lanes' values -> their sum on thread 0, in a tree of fixed shape (xor butterfly per wave, the four waves in wave order)
__device__ __forceinline__ double block_sum_f64(double s) {
  __shared__ double red[4];
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// (double) x * (double) x is exact (48 significant bits) and at most 1.2e77: the sum is non-finite only if an element is
// Streaming (non-temporal) loads: behind kernels that left the last-level cache full of their stores, a read that allocates there runs
// at 2.3 TB/s whatever its shape, this one at 5.3 (77 vs 33 us behind a 1 GB store sweep, 50 vs 29 us behind the SGD kernel:
// profiles/grad_guard.txt, tools/micro/sumsq_read.hip); the gradient is read once more only, by the SGD launches, as without the guard.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n4, long n, double* __restrict__ ws) {
  double a[4] = {0.0, 0.0, 0.0, 0.0};   // one accumulator per element slot of the float4: four independent chains per lane
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  const f32x4* g4 = (const f32x4*)g;
  for (; i + 3 * stride < n4; i += 4 * stride) {   // four loads in flight
    const f32x4 v0 = __builtin_nontemporal_load(g4 + i), v1 = __builtin_nontemporal_load(g4 + i + stride);
    const f32x4 v2 = __builtin_nontemporal_load(g4 + i + 2 * stride), v3 = __builtin_nontemporal_load(g4 + i + 3 * stride);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      a[e] = fma((double)v0[e], (double)v0[e], a[e]);
      a[e] = fma((double)v1[e], (double)v1[e], a[e]);
      a[e] = fma((double)v2[e], (double)v2[e], a[e]);
      a[e] = fma((double)v3[e], (double)v3[e], a[e]);
    }
  }
  for (; i < n4; i += stride) {
    const f32x4 v = __builtin_nontemporal_load(g4 + i);
#pragma unroll
    for (int e = 0; e < 4; e++) a[e] = fma((double)v[e], (double)v[e], a[e]);
  }
  double s = (a[0] + a[1]) + (a[2] + a[3]);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double t = (double)g[(n4 << 2) + threadIdx.x];
    s = fma(t, t, s);
  }
  s = block_sum_f64(s);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// one block: thread t adds partials t, t + 256, ... in ascending order, then the same tree; thread 0 writes the state words
__global__ __launch_bounds__(256) void grad_guard_finish_kernel(const double* __restrict__ ws, int blocks, float max_norm,
                                                                float* __restrict__ state) {
  double s = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) s += ws[b];
  s = block_sum_f64(s);
  if (threadIdx.x != 0) return;
  int* ist = (int*)state;
  const bool skip = !(s < (double)INFINITY);   // NaN or +Inf (a sum of squares has no other way to be non-finite)
  const float norm = (float)sqrt(s);
  float coef = 1.0f;
  if (skip) coef = 0.0f;
  else if (max_norm > 0.0f) coef = fminf(1.0f, max_norm / (norm + 1e-6f));   // torch.nn.utils.clip_grad_norm_
  state[0] = coef;
  state[1] = norm;
  ist[2] = skip ? 1 : 0;
  ist[3] += 1;
  if (skip) ist[4] += 1;
  if (!skip && coef < 1.0f) ist[5] += 1;
  ist[6] = skip ? ist[6] + 1 : 0;
}

// sgd_kernel on g' = round_fp32(g * coef); a skipped step returns before its first store
__global__ __launch_bounds__(256) void sgd_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ buf, long n4, long n, float lr, float wd,
                                                          float mom, int first, const float* __restrict__ state) {
  if (((const int*)state)[2]) return;
  const float coef = state[0];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 w = ((f32x4*)p)[i];
    const f32x4 gr = ((const f32x4*)g)[i];
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (!first) b = ((f32x4*)buf)[i];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float d = __fmul_rn(gr[e], coef) + wd * w[e];
      b[e] = first ? d : mom * b[e] + d;
      w[e] = w[e] - lr * b[e];
    }
    ((f32x4*)buf)[i] = b;
    ((f32x4*)p)[i] = w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    const float d = __fmul_rn(g[i], coef) + wd * p[i];
    const float b = first ? d : mom * buf[i] + d;
    buf[i] = b;
    p[i] = p[i] - lr * b;
  }
}

extern "C" int mmt_grad_guard(const float* g, int64_t n, double* ws, float* state, float max_norm, void* stream) {
  if (n < 0 || !ws || !state || (n > 0 && !g)) return MMT_EINVAL;
  if (((uintptr_t)g & 15) || ((uintptr_t)ws & 7) || ((uintptr_t)state & 3)) return MMT_EINVAL;
  const int blocks = stream_blocks(n >> 2);   // of n alone, <= MMT_GRAD_GUARD_WS
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, (long)(n >> 2), (long)n, ws);
  MMT_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, blocks, max_norm,
                     state);
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmt_sgd_momentum_guarded(float* p, const float* g, float* buf, int64_t n, float lr, float wd, float momentum,
                                        int first, const float* state, void* stream) {
  if (n <= 0) return 0;
  if (!state || ((uintptr_t)state & 3)) return MMT_EINVAL;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) return MMT_EINVAL;
  hipLaunchKernelGGL(sgd_guarded_kernel, dim3(stream_blocks(n >> 2)), dim3(256), 0, (hipStream_t)stream, p, g, buf,
                     (long)(n >> 2), (long)n, lr, wd, momentum, first, state);
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmt_version(void) { return 1; }
