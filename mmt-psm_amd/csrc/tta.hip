// Test-time augmentation: the two merges over views (include/mmtpsm.h: mmt_tta_merge_box, mmt_tta_merge_mask).
//
// Both kernels own every output element exactly once and add the views in ascending order: no atomics, the same bits run to
// run.  Built without FMA contraction (Makefile: EXACT), so (a + a) / 2 == a and x / 1 == x hold to the bit: one view, or two
// identical un-mirrored views, give that view's softmax / sigmoid / regression back.
#include "common.h"
#include <math.h>

namespace {

// IEEE 754-2019 `maximum`: NaN when either operand is (fmaxf returns the other one), as in the convolution epilogues
__device__ __forceinline__ float tta_max_nan(const float a, const float b) { return __builtin_elementwise_maximum(a, b); }

__device__ __forceinline__ float tta_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = tta_max_nan(v, __shfl_xor(v, o, 64));
  return v;
}

constexpr int BOX_ROWS = 4;   // one wavefront per row, four rows per block

// One wavefront per proposal row: lane c holds class c (C <= 64), so a view's logit row is ONE coalesced read and the row
// maximum / sum are butterfly reductions (every lane ends with the same value: the order of additions is fixed by the lane
// pattern, not by arrival).  The 4C regression values of the row are read 64 at a time, again along the innermost dimension.
__global__ __launch_bounds__(64 * BOX_ROWS) void tta_merge_box_kernel(const float* __restrict__ logits, const float* __restrict__ reg,
                                                                       const int V, const int R, const int C, const int flip_mask,
                                                                       float* __restrict__ prob, float* __restrict__ reg_out) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * BOX_ROWS + (threadIdx.x >> 6);
  if (r >= R) return;   // (whole wavefronts leave: the shuffles below never see a missing lane)
  const bool in = lane < C;
  float acc = 0.f;
  for (int v = 0; v < V; v++) {
    const float x = in ? logits[((long)v * R + r) * C + lane] : -INFINITY;
    const float mx = tta_wave_max(x);          // NaN if any logit of the row is NaN -> the whole row becomes NaN
    const float e = in ? expf(x - mx) : 0.f;   // (+inf - +inf = NaN as well: a row with an infinite logit is NaN, like the formulation)
    const float s = wave_sum(e);
    acc += e / s;
  }
  if (in) prob[r * C + lane] = acc / (float)V;
  const int C4 = 4 * C;
  for (int j = lane; j < C4; j += 64) {
    const bool dx = (j & 3) == 0;
    float a = 0.f;
    for (int v = 0; v < V; v++) {
      const float t = reg[((long)v * R + r) * C4 + j];
      a += (dx && ((flip_mask >> v) & 1)) ? -t : t;
    }
    reg_out[r * C4 + j] = a / (float)V;
  }
}

__device__ __forceinline__ float tta_sigmoid(const float x) {   // no overflow for either sign; NaN stays NaN
  if (x >= 0.f) return 1.f / (1.f + expf(-x));
  const float e = expf(x);
  return e / (1.f + e);
}

// One thread per output pixel, x innermost: a wavefront reads runs of whole rows of the predicted class's plane -- forward for
// a plain view, the same rows right to left for a mirrored one (the same cache lines either way) -- and writes them forward.
__global__ __launch_bounds__(256) void tta_merge_mask_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              const int V, const long D, const int C, const int M,
                                                              const int flip_mask, float* __restrict__ prob) {
  const long MM = (long)M * M;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= D * MM) return;
  const long d = i / MM;
  const int p = (int)(i - d * MM);
  const int64_t lab = labels[d];
  if (lab < 0 || lab >= C) {   // no such class plane: this detection's block says so, nothing is read
    prob[i] = __builtin_nanf("");
    return;
  }
  const int y = p / M, x = p - y * M;
  float acc = 0.f;
  for (int v = 0; v < V; v++) {
    const int xv = ((flip_mask >> v) & 1) ? M - 1 - x : x;
    acc += tta_sigmoid(logits[(((long)v * D + d) * C + lab) * MM + (long)y * M + xv]);
  }
  prob[i] = acc / (float)V;
}

inline bool tta_views_ok(const int V, const int flip_mask) { return V >= 1 && V <= 8 && flip_mask >= 0 && flip_mask < (1 << V); }

}  // namespace

extern "C" int mmt_tta_merge_box(const float* logits, const float* reg, int V, int R, int C, int flip_mask, float* prob,
                                 float* reg_out, void* stream) {
  if (!tta_views_ok(V, flip_mask) || C < 1 || C > 64 || R < 0) return MMT_EINVAL;
  if (R == 0) return 0;
  if (!logits || !reg || !prob || !reg_out) return MMT_EINVAL;
  hipLaunchKernelGGL(tta_merge_box_kernel, dim3(mmt_cdiv(R, BOX_ROWS)), dim3(64 * BOX_ROWS), 0, (hipStream_t)stream, logits, reg, V, R,
                     C, flip_mask, prob, reg_out);
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmt_tta_merge_mask(const float* logits, const int64_t* labels, int V, int D, int C, int M, int flip_mask,
                                  float* prob, void* stream) {
  if (!tta_views_ok(V, flip_mask) || C < 1 || C > 64 || M < 1 || M > 1024 || D < 0) return MMT_EINVAL;
  if (D == 0) return 0;
  if (!logits || !labels || !prob) return MMT_EINVAL;
  const long blocks = ((long)D * M * M + 255) / 256;
  if (blocks > 0x7fffffffL) return MMT_EINVAL;
  hipLaunchKernelGGL(tta_merge_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits, labels, V, (long)D, C,
                     M, flip_mask, prob);
  MMT_LAUNCH_CHECK();
  return 0;
}
