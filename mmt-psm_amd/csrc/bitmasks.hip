// Geometry on mask words (include/mmtpsm.h, "bitmap ground truth"): crop, resize and flip of a set of instance masks, and
// crop-and-resize of the matched instance into each ROI's M x M target.  A mask is what csrc/maskeval.hip defines: 64-bit words
// over the run-length codec's COLUMN-major flattening, bit k = pixel (y = k % H, x = k / H), tail bits zero.
//
// Integer arithmetic only ("Bitmap ground truth"): binary bilinear resampling meets exact ties at 1/2 all the
// time, so a float kernel would differ from any oracle by rounding luck.  For output row i of OH over a window of h rows
//   ny = max((2 i + 1) h - OH, 0), dy = 2 OH, ia = ny / dy, ry = ny % dy, ib = min(ia + 1, h - 1)
// (columns alike), S = the bilinear sum of the four source bits with the integer weights, output bit = (2 S >= dx dy).
// With H, W, OH, OW <= 16384 and H W, OH OW <= 2^26 every term fits in int32: ny < 2^29, S <= dx dy <= 2^28.
// No float atomics, no atomics at all: every result is independent of scheduling.
#include "common.h"

typedef unsigned long long u64;

#define MAX_MASKS 65535          // masks per call, as for the other mask-word entry points
#define MAX_SIDE 16384
#define MAX_AREA (1L << 26)
#define MAX_M 32

static inline bool bad_size(int H, int W) { return H <= 0 || W <= 0 || H > MAX_SIDE || W > MAX_SIDE || (long)H * (long)W > MAX_AREA; }
static inline long words_of(int H, int W) { return ((long)H * W + 63) >> 6; }

struct Tap { int a, b, r; };   // the two source indices of one output index and the weight r (of 2 * out) of the second

// floor(num / den) and the remainder for 0 <= num < 2^30, 0 < den <= 2^15, inv = 1.0 / den rounded to double (the host passes it):
// the double product is within 2^-22 of the quotient, so its truncation is at most one off and the remainder says which way.
// An integer result by construction; a 32-bit hardware division is some thirty instructions, and there are three per output bit.
__device__ __forceinline__ int div_by(int num, int den, double inv, int& rem) {
  int q = (int)((double)num * inv);
  int r = num - q * den;
  if (r < 0) { q--; r += den; }
  else if (r >= den) { q++; r -= den; }
  rem = r;
  return q;
}

__device__ __forceinline__ Tap tap_of(int i, int n, int out, double inv_den) {
  const int num = max((2 * i + 1) * n - out, 0);
  Tap t;
  t.a = div_by(num, 2 * out, inv_den, t.r);
  t.b = min(t.a + 1, n - 1);
  return t;
}

__device__ __forceinline__ int bit_at(const u64* __restrict__ wp, int H, int y, int x) {
  const int k = x * H + y;   // < 2^26
  return (int)((wp[k >> 6] >> (k & 63)) & 1ULL);
}

// the output bit at (row i of OH, column j of OW) of the window (x0, y0, w, h) of the mask at wp
__device__ __forceinline__ int resampled(const u64* __restrict__ wp, int H, int x0, int y0, int w, int h, int i, int j, int OH,
                                         int OW, double inv_dy, double inv_dx) {
  const Tap ty = tap_of(i, h, OH, inv_dy), tx = tap_of(j, w, OW, inv_dx);
  const int dy = 2 * OH, dx = 2 * OW;
  const int paa = bit_at(wp, H, y0 + ty.a, x0 + tx.a), pab = bit_at(wp, H, y0 + ty.a, x0 + tx.b);
  const int pba = bit_at(wp, H, y0 + ty.b, x0 + tx.a), pbb = bit_at(wp, H, y0 + ty.b, x0 + tx.b);
  const int S = (dy - ty.r) * ((dx - tx.r) * paa + tx.r * pab) + ty.r * ((dx - tx.r) * pba + tx.r * pbb);
  return 2 * S >= dx * dy;
}

// ------------------------------------------------------------------------------------ resample
// One output word per wave: lane l computes bit 64 * word + l, the ballot is the word.  Consecutive bits run down an output
// column, so the source rows of neighbouring lanes are neighbours too: the four source bits of a wave fall in a few words.
// grid (ceil(nwo / 4), G), 256 threads.
__global__ __launch_bounds__(256) void mask_words_resample_kernel(const u64* __restrict__ words, int H, long nwi, int x0, int y0,
                                                                  int w, int h, int flip, int OH, int OW, long nwo,
                                                                  double inv_oh, double inv_dy, double inv_dx,
                                                                  u64* __restrict__ out) {
  const long word = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (word >= nwo) return;   // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int k = (int)(word * 64 + lane);
  int bit = 0;
  if (k < OH * OW) {
    int i, j = div_by(k, OH, inv_oh, i);
    if (flip & 1) j = OW - 1 - j;
    if (flip & 2) i = OH - 1 - i;
    bit = resampled(words + (long)blockIdx.y * nwi, H, x0, y0, w, h, i, j, OH, OW, inv_dy, inv_dx);
  }
  const u64 v = __ballot(bit);
  if (lane == 0) out[(long)blockIdx.y * nwo + word] = v;
}

// ------------------------------------------------------------------------------------ targets
// One block per ROI.  Threads run along i (rows) within an output column, so that neighbouring lanes read neighbouring source
// bits; the plane is staged in LDS (row stride M + 1: the column-wise writes spread over the banks) and stored row-major in
// full lines.  A ROI without an instance (roi_inst outside [0, G)) or without a window (a non-finite box) reads no mask word.
__device__ __forceinline__ int to_int_clamped(float v) {   // rintf: half to even, then +-2^30 in float
  return (int)fminf(fmaxf(rintf(v), -1073741824.f), 1073741824.f);
}

__global__ __launch_bounds__(256) void mask_words_targets_kernel(const u64* __restrict__ words, int G, int H, int W, long nwi,
                                                                 const int* __restrict__ roi_inst, const float* __restrict__ boxes,
                                                                 int M, double inv_2m, float* __restrict__ out) {
  __shared__ float plane[MAX_M * (MAX_M + 1)];
  const int p = blockIdx.x, n = M * M;
  float* dst = out + (long)p * n;
  const int g = roi_inst[p];
  const float bx1 = boxes[4L * p], by1 = boxes[4L * p + 1], bx2 = boxes[4L * p + 2], by2 = boxes[4L * p + 3];
  const bool window = isfinite(bx1) && isfinite(by1) && isfinite(bx2) && isfinite(by2);
  if (g < 0 || g >= G || !window) {   // (block-uniform)
    for (int e = threadIdx.x; e < n; e += 256) dst[e] = 0.f;
    return;
  }
  const int xa = to_int_clamped(bx1), ya = to_int_clamped(by1), xb = to_int_clamped(bx2), yb = to_int_clamped(by2);
  const int x0 = min(max(xa, 0), W - 1), y0 = min(max(ya, 0), H - 1);
  const int xe = max(min(max(xb, 0), W), x0 + 1), ye = max(min(max(yb, 0), H), y0 + 1);
  const int w = xe - x0, h = ye - y0;
  const u64* wp = words + (long)g * nwi;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int j = e / M, i = e - j * M;
    plane[i * (M + 1) + j] = (float)resampled(wp, H, x0, y0, w, h, i, j, M, M, inv_2m, inv_2m);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += 256) {
    const int i = e / M, j = e - i * M;
    dst[e] = plane[i * (M + 1) + j];
  }
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int mmt_mask_words_resample(const uint64_t* words, int G, int H, int W, int x0, int y0, int w, int h, int flip, int OH,
                                       int OW, uint64_t* out, int32_t* rec, void* stream) {
  if (G < 0 || G > MAX_MASKS || bad_size(H, W) || bad_size(OH, OW)) return MMT_EINVAL;
  if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h || flip < 0 || flip > 3) return MMT_EINVAL;
  if (G == 0) return 0;
  if (!words || !out || !rec) return MMT_EINVAL;
  const long nwi = words_of(H, W), nwo = words_of(OH, OW);
  if (out < words + (long)G * nwi && words < out + (long)G * nwo) return MMT_EINVAL;   // the output may not overlap the input
  hipLaunchKernelGGL(mask_words_resample_kernel, dim3(mmt_cdiv(nwo, 4), G), dim3(256), 0, (hipStream_t)stream, (const u64*)words, H,
                     nwi, x0, y0, w, h, flip, OH, OW, nwo, 1.0 / OH, 1.0 / (2 * OH), 1.0 / (2 * OW), (u64*)out);
  MMT_LAUNCH_CHECK();
  return mmt_mask_records(out, G, OH, OW, rec, (hipStream_t)stream);
}

extern "C" int mmt_mask_words_targets(const uint64_t* words, int G, int H, int W, const int32_t* roi_inst, const float* boxes, int P,
                                      int M, float* out, void* stream) {
  if (G < 0 || G > MAX_MASKS || P < 0 || M < 1 || M > MAX_M || bad_size(H, W)) return MMT_EINVAL;
  if (G == 0 || P == 0) return 0;
  if (!words || !roi_inst || !boxes || !out) return MMT_EINVAL;
  hipLaunchKernelGGL(mask_words_targets_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, (const u64*)words, G, H, W,
                     words_of(H, W), roi_inst, boxes, M, 1.0 / (2 * M), out);
  MMT_LAUNCH_CHECK();
  return 0;
}
