// Batched Soft-NMS (Bodla et al. 2017) for gfx950: the neighbours of a picked box keep their place with a decayed score
// instead of being removed ("Soft-NMS in the box head").
//
// The greedy NMS of nms.hip cannot be reused: its bit-mask says once and for all who suppresses whom in a FIXED order, here
// the order itself depends on scores that change with every pick.  So: one block of 512 threads per pre-sorted segment of
// n <= 2048 candidates, thread t owns the positions t, t + 512, t + 1024, t + 1536 (box and current score in registers, the
// boxes once more in LDS so that every thread can read the picked one), and per pick
//   1. every thread forms the largest 64-bit key (ordered score || inverted position) of the candidates it still owns,
//   2. a wave-wide maximum (DPP row scans + four readlanes, no LDS) and one 8-byte slot per wave in LDS,
//   3. ONE barrier (the slots are double-buffered by pick parity), after which every thread reads the eight slots: the block
//      agrees on the pick without a second exchange,
//   4. every thread decays the candidates it owns against the picked box.
// It is a chain of up to n dependent picks; what a pick costs is the barrier and the IoUs of one thread's (at most four)
// candidates, not bandwidth.  No atomics, a fixed order: the same bits on every run.  Built with -ffp-contract=off: the IoU
// is the expression of nms.hip's iou_ge, rounding for rounding.
#include <math.h>
#include "common.h"

namespace {

constexpr int SN_NT = 512, SN_KPT = 4, SN_MAX = SN_NT * SN_KPT, SN_WAVES = SN_NT / 64;

__device__ __forceinline__ unsigned f2ord(float f) {  // order-preserving float -> unsigned (as in select.hip)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// maximum of a 32-bit value over the 64 lanes (uniform result): inclusive max-scan inside each row of 16 lanes with DPP row
// shifts (lanes without a source read 0, the identity), then the four row totals
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned wave_max32(unsigned v) {
  v = umax(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));  // row_shr:1
  v = umax(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));  // row_shr:2
  v = umax(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));  // row_shr:4
  v = umax(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));  // row_shr:8
  // (v_readlane's builtin returns int: compare as unsigned, ordered scores have the top bit set)
  const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 15), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 31);
  const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 47), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 63);
  return umax(umax(r0, r1), umax(r2, r3));
}

__device__ __forceinline__ float iou_of(const f32x4 a, const f32x4 b) {
  // nms.hip's iou_ge up to the comparison: areas with +1 (nms_cpu.cpp:22)
  const float aa = (a[2] - a[0] + 1) * (a[3] - a[1] + 1);
  const float ab = (b[2] - b[0] + 1) * (b[3] - b[1] + 1);
  const float xx1 = fmaxf(a[0], b[0]), yy1 = fmaxf(a[1], b[1]);
  const float xx2 = fminf(a[2], b[2]), yy2 = fminf(a[3], b[3]);
  const float w = fmaxf(0.f, xx2 - xx1 + 1), h = fmaxf(0.f, yy2 - yy1 + 1);
  const float inter = w * h;
  return inter / (aa + ab - inter);
}

// scores / out_scores may be the same array: a block reads its segment's scores before the first pick and writes them behind
// the last one, and segments do not overlap
template <int METHOD>  // 0 linear, 1 gaussian
__global__ __launch_bounds__(SN_NT) void soft_nms_kernel(const float* __restrict__ boxes, const float* scores,
                                                         const int* __restrict__ seg_off, const int max_n, const float thr,
                                                         const float sigma, const float min_score, int* __restrict__ picked,
                                                         int* __restrict__ picked_cnt, float* out_scores) {
  __shared__ f32x4 sbox[SN_MAX];
  __shared__ unsigned long long slot[2][SN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, seg = blockIdx.x;
  const int s0 = seg_off[seg];
  const int n = min(max(seg_off[seg + 1] - s0, 0), max_n);   // (max_n <= SN_MAX: checked by the caller)
  f32x4 bx[SN_KPT];
  float sc[SN_KPT];
  unsigned alive = 0u;   // bit k: position tid + k * SN_NT is a candidate that has not been picked
#pragma unroll
  for (int k = 0; k < SN_KPT; k++) {
    const int p = tid + k * SN_NT;
    bx[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    sc[k] = 0.f;
    if (p < n) {
      bx[k] = *(const f32x4*)(boxes + (long)(s0 + p) * 4);
      sc[k] = scores[s0 + p];
      sbox[p] = bx[k];
      alive |= 1u << k;
    }
  }
  __syncthreads();
  int* const pk = picked + (long)seg * max_n;
  int cnt = 0;
  for (int it = 0; it < n; it++) {
    // largest current score of this thread's candidates; equal scores: the smaller position, i.e. the larger low word.  A
    // candidate's key is never 0 (its low word is not), 0 stands for "none"
    unsigned hi = 0u, lo = 0u;
#pragma unroll
    for (int k = 0; k < SN_KPT; k++) {
      const unsigned h = f2ord(sc[k]), l = 0xffffffffu - (unsigned)(tid + k * SN_NT);
      const bool take = ((alive >> k) & 1u) && (lo == 0u || h > hi);
      hi = take ? h : hi;
      lo = take ? l : lo;
    }
    const unsigned whi = wave_max32(hi);
    const unsigned wlo = wave_max32(hi == whi ? lo : 0u);
    if (lane == 0) slot[it & 1][wave] = wlo ? (((unsigned long long)whi << 32) | wlo) : 0ull;
    __syncthreads();   // the only barrier of a pick: the slots of pick it + 2 are written behind the barrier of pick it + 1
    unsigned long long best = 0ull;
#pragma unroll
    for (int w = 0; w < SN_WAVES; w++) {
      const unsigned long long v = slot[it & 1][w];
      best = v > best ? v : best;
    }
    if (best == 0ull) break;                                  // nobody is left
    if (ord2f((unsigned)(best >> 32)) < min_score) break;     // scores only fall: nothing behind it can qualify
    const int p = (int)(0xffffffffu - (unsigned)best);
    if (tid == 0) pk[cnt] = p;
    cnt++;
    if ((p & (SN_NT - 1)) == tid) alive &= ~(1u << (p / SN_NT));   // the owner: picked, keeps its current score
    const f32x4 pb = sbox[p];
#pragma unroll
    for (int k = 0; k < SN_KPT; k++) {
      if (!((alive >> k) & 1u)) continue;
      const float ov = iou_of(pb, bx[k]);
      if (METHOD == 0) {
        if (ov >= thr) sc[k] = sc[k] * (1.0f - ov);           // (false for a NaN overlap)
      } else {
        if (ov == ov) sc[k] = sc[k] * expf(-(ov * ov) / sigma);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < SN_KPT; k++) {
    const int p = tid + k * SN_NT;
    if (p < n) out_scores[s0 + p] = sc[k];
  }
  if (tid == 0) picked_cnt[seg] = cnt;
}

}  // namespace

extern "C" int mmt_soft_nms_batched(const float* boxes, const float* scores, const int32_t* seg_off, int B, int max_n, int method,
                                    float nms_thresh, float sigma, float min_score, int32_t* picked, int32_t* picked_cnt,
                                    float* out_scores, void* stream) {
  if (B < 0 || max_n < 0 || max_n > SN_MAX || (method != 0 && method != 1)) return MMT_EINVAL;
  if (!(sigma > 0.f) || !isfinite(sigma) || !(min_score > 0.f && min_score <= 1.f) || !(nms_thresh > 0.f && nms_thresh <= 1.f))
    return MMT_EINVAL;
  if (B == 0) return 0;
  if (!seg_off || !picked_cnt || (max_n > 0 && (!boxes || !scores || !picked || !out_scores)) || ((size_t)boxes & 15))
    return MMT_EINVAL;
  if (method == 0)
    hipLaunchKernelGGL(soft_nms_kernel<0>, dim3(B), dim3(SN_NT), 0, (hipStream_t)stream, boxes, scores, seg_off, max_n, nms_thresh,
                       sigma, min_score, picked, picked_cnt, out_scores);
  else
    hipLaunchKernelGGL(soft_nms_kernel<1>, dim3(B), dim3(SN_NT), 0, (hipStream_t)stream, boxes, scores, seg_off, max_n, nms_thresh,
                       sigma, min_score, picked, picked_cnt, out_scores);
  MMT_LAUNCH_CHECK();
  return 0;
}
