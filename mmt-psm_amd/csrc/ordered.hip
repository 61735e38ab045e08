// Deterministic mode: the library-wide switch and the ordered column sum that stands in for the float atomics of the bias gradients
// (colsum_kernel and the dbias epilogues of csrc/conv_wgrad.hip / conv_wgpl.hip) -- the reference takes its bias gradients from
// ATen's sum over the batch and pixel dimensions.
#include "common.h"

static int g_deterministic = 0;

extern "C" int mmt_set_deterministic(int on) {
  g_deterministic = on ? 1 : 0;
  return 0;
}

extern "C" int mmt_get_deterministic(void) { return g_deterministic; }

namespace {

// rows per block and block count of stage one: functions of M alone, at most MMT_COLSUM_MAX_BLOCKS blocks
inline int colsum_rows_per_block(int M) {
  int rpb = mmt_cdiv(M, MMT_COLSUM_MAX_BLOCKS);
  rpb = (rpb + 15) / 16 * 16;
  return rpb < 64 ? 64 : rpb;
}

// stage one: ws[blockIdx.y][c] = sum of dy[r][c] over the block's rows.  Lanes run along C (coalesced, as in colsum_kernel); the four
// waves take rows r0 + sub, + 4, ..., each into four interleaved accumulators (a shorter chain of additions and four loads in flight)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ dy, int M, int C, float* __restrict__ ws,
                                                             int rows_per_block) {
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    int r = r0 + sub;
    for (; r + 12 < r1; r += 16) {
#pragma unroll
      for (int u = 0; u < 4; u++) a[u] += dy[(long)(r + 4 * u) * C + c];
    }
#pragma unroll
    for (int u = 0; u < 3; u++)   // (at most three rows are left)
      if (r + 4 * u < r1) a[u] += dy[(long)(r + 4 * u) * C + c];
  }
  __shared__ float red[4][64];
  red[sub][lane] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (sub == 0 && c < C) ws[(long)blockIdx.y * C + c] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// stage two: out[c] += the column's partials, wave `sub` adding its quarter of the blocks in ascending order, the quarters in order
__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* __restrict__ ws, int blocks, int C, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int q = (blocks + 3) / 4;
  const int b0 = sub * q, b1 = min(blocks, b0 + q);
  float s = 0.f;
  if (c < C)
    for (int b = b0; b < b1; b++) s += ws[(long)b * C + c];
  __shared__ float red[4][64];
  red[sub][lane] = s;
  __syncthreads();
  if (sub == 0 && c < C) out[c] += (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

}  // namespace

extern "C" int mmt_colsum_ordered(const float* dy, int M, int C, float* out, float* ws, void* stream) {
  if (!dy || !out || !ws || M < 0 || C < 1) return MMT_EINVAL;
  if (M == 0) return 0;
  const int rpb = colsum_rows_per_block(M);
  const int blocks = mmt_cdiv(M, rpb);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(mmt_cdiv(C, 64), blocks), dim3(256), 0, s, dy, M, C, ws, rpb);
  MMT_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(mmt_cdiv(C, 64)), dim3(256), 0, s, ws, blocks, C, out);
  MMT_LAUNCH_CHECK();
  return 0;
}
