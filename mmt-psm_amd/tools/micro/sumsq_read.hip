// Stage one of the gradient guard (csrc/optim.hip: grad_sumsq_kernel) in variants, on a gradient of the bench's size (43 869 880 fp32):
// grid-stride with 2 / 4 / 8 loads in flight at several grid sizes, streaming (non-temporal) loads, block-contiguous spans, and an
// fp32-accumulating kernel over the same loads (what the fp64 arithmetic costs: nothing).  Each variant 12 times behind a 1 GB store
// sweep (the last-level cache full of another kernel's dirty lines) and 12 times back to back; events around single launches.
// The numbers are in profiles/grad_guard.txt.
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o sumsq_read sumsq_read.hip ; run: ./sumsq_read
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double bsum(double s) {
  __shared__ double red[4];
  s = wsum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
template <bool NT> __device__ __forceinline__ f32x4 ld(const f32x4* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}
// grid-stride, U loads in flight
template <int U, bool NT>
__global__ __launch_bounds__(256) void sumsq_gs(const float* __restrict__ g, long n4, double* __restrict__ ws) {
  double a[4] = {0, 0, 0, 0};
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  const f32x4* g4 = (const f32x4*)g;
  for (; i + (U - 1) * stride < n4; i += U * stride) {
    f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = ld<NT>(g4 + i + u * stride);
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int e = 0; e < 4; e++) a[e] = fma((double)v[u][e], (double)v[u][e], a[e]);
  }
  for (; i < n4; i += stride) {
    const f32x4 v = ld<NT>(g4 + i);
#pragma unroll
    for (int e = 0; e < 4; e++) a[e] = fma((double)v[e], (double)v[e], a[e]);
  }
  double s = bsum((a[0] + a[1]) + (a[2] + a[3]));
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
// block-contiguous spans
template <int U>
__global__ __launch_bounds__(256) void sumsq_bc(const float* __restrict__ g, long n4, double* __restrict__ ws) {
  double a[4] = {0, 0, 0, 0};
  const long per = ((n4 + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
  const long lo = per * blockIdx.x, hi = min(lo + per, n4);
  const f32x4* g4 = (const f32x4*)g;
  long i = lo + threadIdx.x;
  for (; i + (U - 1) * 256 < hi; i += U * 256) {
    f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = g4[i + u * 256];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int e = 0; e < 4; e++) a[e] = fma((double)v[u][e], (double)v[u][e], a[e]);
  }
  for (; i < hi; i += 256) {
    const f32x4 v = g4[i];
#pragma unroll
    for (int e = 0; e < 4; e++) a[e] = fma((double)v[e], (double)v[e], a[e]);
  }
  double s = bsum((a[0] + a[1]) + (a[2] + a[3]));
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
// fp32 read-only reference: the same loads, float accumulate (how fast can a read go at all)
__global__ __launch_bounds__(256) void sum_f32(const float* __restrict__ g, long n4, double* __restrict__ ws) {
  float a[4] = {0, 0, 0, 0};
  const long stride = (long)gridDim.x * 256;
  const f32x4* g4 = (const f32x4*)g;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const f32x4 v = g4[i];
#pragma unroll
    for (int e = 0; e < 4; e++) a[e] += v[e] * v[e];
  }
  double s = bsum((double)((a[0] + a[1]) + (a[2] + a[3])));
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sweep(f32x4* p, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) p[i] = f32x4{1.f, 2.f, 3.f, 4.f};
}
__global__ void fill(float* p, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = (float)((i * 2654435761u >> 8) & 1023) * (1.f / 512) - 1.f;
}

int main() {
  const long n = 43869880, n4 = n >> 2, nsweep4 = (1L << 30) / 16;
  float* g; double* ws; f32x4* junk;
  CK(hipMalloc(&g, n * 4)); CK(hipMalloc(&ws, 8192 * 8)); CK(hipMalloc(&junk, nsweep4 * 16));
  fill<<<4096, 256>>>(g, n);
  CK(hipDeviceSynchronize());
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  struct V { const char* name; int id; int grid; };
  const V vs[] = {{"gs U4 grid4096", 0, 4096}, {"gs U8 grid4096", 1, 4096}, {"gs U4 grid2048", 0, 2048}, {"gs U8 grid2048", 1, 2048},
                  {"gs U2 grid4096", 2, 4096}, {"gs U4 nontemporal grid4096 (shipped)", 3, 4096}, {"gs U8 nontemporal grid2048", 4, 2048},
                  {"block-contiguous U4 grid4096", 5, 4096}, {"block-contiguous U8 grid2048", 6, 2048}, {"fp32 accumulate grid4096", 7, 4096},
                  {"gs U4 grid1024", 0, 1024}, {"gs U8 grid1024", 1, 1024}};
  for (int cold = 1; cold >= 0; cold--) {
    printf("%s\n", cold ? "COLD (1 GB written between calls)" : "WARM (back to back)");
    for (const V& v : vs) {
      std::vector<float> t;
      double first = 0;
      for (int r = 0; r < 13; r++) {
        if (cold) sweep<<<4096, 256>>>(junk, nsweep4);
        CK(hipEventRecord(e0));
        switch (v.id) {
          case 0: sumsq_gs<4, false><<<v.grid, 256>>>(g, n4, ws); break;
          case 1: sumsq_gs<8, false><<<v.grid, 256>>>(g, n4, ws); break;
          case 2: sumsq_gs<2, false><<<v.grid, 256>>>(g, n4, ws); break;
          case 3: sumsq_gs<4, true><<<v.grid, 256>>>(g, n4, ws); break;
          case 4: sumsq_gs<8, true><<<v.grid, 256>>>(g, n4, ws); break;
          case 5: sumsq_bc<4><<<v.grid, 256>>>(g, n4, ws); break;
          case 6: sumsq_bc<8><<<v.grid, 256>>>(g, n4, ws); break;
          case 7: sum_f32<<<v.grid, 256>>>(g, n4, ws); break;
        }
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (r) t.push_back(ms * 1e3f);
        if (r == 0) { std::vector<double> h(v.grid); CK(hipMemcpy(h.data(), ws, v.grid * 8, hipMemcpyDeviceToHost)); for (double x : h) first += x; }
      }
      std::sort(t.begin(), t.end());
      printf("  %-34s median %7.1f us  min %7.1f  max %7.1f   %.2f TB/s   total %.9g\n", v.name, t[6], t[0], t[11], n * 4 / t[6] / 1e6, first);
    }
  }
  return 0;
}
