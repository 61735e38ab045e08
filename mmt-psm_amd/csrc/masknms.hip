// Mask NMS at inference (include/mmtpsm.h: mmt_mask_nms): greedy suppression of duplicate instances by the overlap of their
// masks, on the mask words of csrc/maskeval.hip.  The reference never gets past host Python here (modeling/python_nms.py:
// cyto_nms, set_cpu_nms).
//
//   phase one (mask_nms_pair_kernel)   one wave per ordered pair of sweep positions p < q: labels, record boxes, then
//                                      popcount(words_i & words_j) over the words of the overlapping columns and the integer test
//                                      inter * 2^20 >= tq * den -> one byte rel[p][q] of the caller's workspace (one writer each)
//   phase two (mask_nms_sweep_kernel)  one block, thread q owns position q: the positions are resolved 64 at a time -- the wave
//                                      that owns a chunk settles it by itself, everybody behind it then takes the chunk's kept set
//
// Integer arithmetic only, no atomics: the same bits on every run, in deterministic mode as well.
#include "maskwords.h"

#define NMS_MAX_D 1024   // the sweep is one block with a thread per detection

// rel is [D][D] bytes over SWEEP POSITIONS (row p, column q); only p < q is written and read
__global__ __launch_bounds__(256) void mask_nms_pair_kernel(const u64* __restrict__ words, const int* __restrict__ rec,
                                                            const int* __restrict__ order, const int* __restrict__ labels, int D,
                                                            int H, long nw, int tq, int measure, int agnostic,
                                                            unsigned char* __restrict__ rel) {
  const long pair = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (pair >= (long)D * D) return;
  const int p = (int)(pair / D), q = (int)(pair - (long)p * D);
  if (q <= p) return;
  const int lane = threadIdx.x & 63;
  const int i = order[p], j = order[q];
  int verdict = 0;
  // (an index outside the rows is no permutation entry: it reads nothing and overlaps nothing)
  if ((unsigned)i < (unsigned)D && (unsigned)j < (unsigned)D && (agnostic || labels[i] == labels[j])) {
    const int* ri = rec + (long)i * REC;
    const int* rj = rec + (long)j * REC;
    int ix, iy, iw, ih, jx, jy, jw, jh;
    box_of(ri, H, ix, iy, iw, ih);
    box_of(rj, H, jx, jy, jw, jh);
    const int xlo = max(ix, jx), ow = min(ix + iw, jx + jw) - xlo;
    const int oh = min(iy + ih, jy + jh) - max(iy, jy);
    if (ow > 0 && oh > 0) {
      // columns outside [xlo, xlo + ow) are empty in at least one of the two masks, so whole words may be taken at both ends
      const long j0 = max(((long)xlo * H) >> 6, 0L), j1 = min(((long)(xlo + ow) * H + 63) >> 6, nw);
      const u64* ip = words + (long)i * nw;
      const u64* jp = words + (long)j * nw;
      int c = 0;
      long k = j0 + lane;
      for (; k + 192 < j1; k += 256)   // four independent 512-byte rows of each mask in flight
        c += __popcll(ip[k] & jp[k]) + __popcll(ip[k + 64] & jp[k + 64]) + __popcll(ip[k + 128] & jp[k + 128]) +
             __popcll(ip[k + 192] & jp[k + 192]);
      for (; k < j1; k += 64) c += __popcll(ip[k] & jp[k]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
      const long ai = ri[0], aj = rj[0];
      const long den = measure ? min(ai, aj) : ai + aj - c;
      verdict = c > 0 && ((long)c << 20) >= (long)tq * den;
    }
  }
  if (lane == 0) rel[pair] = (unsigned char)verdict;
}

__global__ __launch_bounds__(NMS_MAX_D) void mask_nms_sweep_kernel(const unsigned char* __restrict__ rel,
                                                                   const int* __restrict__ order, int D,
                                                                   unsigned char* __restrict__ keep, int* __restrict__ count) {
  __shared__ u64 keptw[NMS_MAX_D / 64];   // bit s of word k: position 64 k + s is kept
  const int t = threadIdx.x, lane = t & 63, mywave = t >> 6;
  const bool valid = t < D;
  const int chunks = (D + 63) >> 6;
  bool removed = false, kept = false;
  for (int k = 0; k < chunks; k++) {
    const int p0 = k * 64;
    // bit s: position p0 + s comes before this one and overlaps it
    const int np = valid ? min(min(64, t - p0), D - p0) : 0;
    u64 m = 0;
    const unsigned char* col = rel + (long)p0 * D + t;
#pragma unroll 8
    for (int s = 0; s < np; s++) m |= (u64)(col[(long)s * D] != 0) << s;
    if (mywave == k) {   // the chunk's own wave: m holds bits below the lane only, the earlier chunks have set `removed`
      u64 K = 0;
      for (int s = 0; s < 64; s++) {
        const u64 alive = __ballot(valid && !removed && (m & K) == 0);
        K |= alive & (1ULL << s);
      }
      kept = (K >> lane) & 1;
      if (lane == 0) keptw[k] = K;
    }
    __syncthreads();
    if (mywave > k) removed = removed || (m & keptw[k]) != 0;
  }
  if (valid) {
    const int i = order[t];
    if ((unsigned)i < (unsigned)D) keep[i] = kept ? 1 : 0;
  }
  if (t == 0) {
    int c = 0;
    for (int k = 0; k < chunks; k++) c += __popcll(keptw[k]);
    *count = c;
  }
}

static inline long nms_ws_bytes(int D) { return (long)D * D; }

extern "C" int mmt_mask_nms_workspace(int D, int64_t* bytes) {
  if (D < 0 || D > NMS_MAX_D || !bytes) return MMT_EINVAL;
  *bytes = nms_ws_bytes(D);
  return 0;
}

extern "C" int mmt_mask_nms(const uint64_t* words, const int32_t* rec, const int32_t* order, const int32_t* labels, int D, int H,
                            int W, int thresh_q20, int measure, int class_agnostic, void* ws, int64_t ws_bytes, uint8_t* keep,
                            int32_t* count, void* stream) {
  if (D < 0 || D > NMS_MAX_D || bad_size(H, W) || thresh_q20 < 1 || thresh_q20 > (1 << 20) || (measure != 0 && measure != 1) ||
      !count)
    return MMT_EINVAL;
  if (D > 0 && (!words || !rec || !order || !labels || !keep || !ws || ws_bytes < nms_ws_bytes(D))) return MMT_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (D > 0) {
    hipLaunchKernelGGL(mask_nms_pair_kernel, dim3(mmt_cdiv((long)D * D, 4)), dim3(256), 0, s, (const u64*)words, rec, order, labels,
                       D, H, words_of(H, W), thresh_q20, measure, class_agnostic != 0, (unsigned char*)ws);
    MMT_LAUNCH_CHECK();
  }
  // whole waves for the D positions (D == 0: the sweep alone, which writes count = 0 and touches nothing else)
  hipLaunchKernelGGL(mask_nms_sweep_kernel, dim3(1), dim3(max(mmt_cdiv(D, 64), 1) * 64), 0, s, (const unsigned char*)ws, order, D,
                     keep, count);
  MMT_LAUNCH_CHECK();
  return 0;
}
