// Mask work of the PAP evaluator on the device: what the reference does in its vendored pycocotools and
// this build restated on numpy in data/datasets/evaluation/pap/mask_rle.py --
//
//   pack / expand     <- pycoco/maskApi.c:21-34 (rleEncode) and pycoco/_mask.pyx:144 (encode), :160 (decode): a mask becomes
//                        64-bit words over the codec's COLUMN-major flattening, bit k = pixel (y = k % H, x = k / H), tail
//                        bits zero, plus one integer record (area, extent, wrap) -- pycoco/maskApi.c:135-151 (rleToBbox)
//   transitions       <- the run boundaries of rleEncode: positions k with bit(k) != bit(k - 1), bit(-1) = 0
//   pair intersections<- pycoco/maskApi.c:239-260 (rleIouInterUnion) under pycoco/_mask.pyx:293-380 (iouIntUni)
//
// Integer arithmetic only; no atomics, every result is independent of scheduling.  The strings themselves (LEB128-like
// characters) are written and parsed by the host.
#include "maskwords.h"
#include <limits.h>

#define STRIP_MAX_H 4096        // the strip kernel keeps 64 columns of H bits in LDS (65 words per column at most)
#define MAX_MASKS 65535          // masks per call: they are the grid's second dimension

__device__ __forceinline__ u64 low_bits(int len) { return len < 64 ? (1ULL << len) - 1 : ~0ULL; }

// ------------------------------------------------------------------------------------ pack
// 64 columns of all H rows are one contiguous, word-aligned range of k.  Lane = column: every load of a wave is 64
// consecutive bytes of one image row; each lane collects the bits of 64 rows of its column, the block keeps the strip as
// per-column bit arrays in LDS and then cuts the output words out of them (a word spans two columns, or many when H < 64).
__global__ __launch_bounds__(256) void pack_strip_kernel(const unsigned char* __restrict__ masks, int H, int W, long nw,
                                                         u64* __restrict__ words) {
  extern __shared__ u64 col[];   // [64][ncp]: bit y of column x0 + c is bit (y & 63) of col[c * ncp + (y >> 6)]
  const int nc = (H + 63) >> 6, ncp = nc | 1;
  const int x0 = blockIdx.x * 64, cx = min(64, W - x0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned char* src = masks + (long)blockIdx.y * H * W;
  for (int c = wave; c < nc; c += 4) {
    const int y0 = c * 64, ny = min(64, H - y0);
    u64 bits = 0;
    if (lane < cx)
      for (int i = 0; i < ny; i++) bits |= (u64)(src[(long)(y0 + i) * W + x0 + lane] != 0) << i;
    col[lane * ncp + c] = bits;
  }
  __syncthreads();
  const long kbase = (long)x0 * H, kend = kbase + (long)cx * H;   // kbase is a multiple of 64
  const int nwords = (int)((kend - kbase + 63) >> 6);
  u64* dst = words + (long)blockIdx.y * nw + (kbase >> 6);
  for (int j = threadIdx.x; j < nwords; j += 256) {
    const long kw = kbase + 64L * j, ke = min(kw + 64, kend);
    long k = kw;
    u64 w = 0;
    while (k < ke) {
      const int xl = (int)((k - kbase) / H), y = (int)((k - kbase) - (long)xl * H);
      const int len = (int)min((long)(H - y), ke - k);
      const u64* cp = col + xl * ncp;
      const int q = y >> 6, s = y & 63;
      u64 v = cp[q] >> s;
      if (s && q + 1 < nc) v |= cp[q + 1] << (64 - s);
      w |= (v & low_bits(len)) << (int)(k - kw);
      k += len;
    }
    dst[j] = w;
  }
}

// H > STRIP_MAX_H: one thread per word, bytes read with a stride of one image row
__global__ __launch_bounds__(256) void pack_word_kernel(const unsigned char* __restrict__ masks, int H, int W, long nw,
                                                        u64* __restrict__ words) {
  const long j = blockIdx.x * 256L + threadIdx.x;
  if (j >= nw) return;
  const unsigned char* src = masks + (long)blockIdx.y * H * W;
  const long hw = (long)H * W, ke = min(j * 64 + 64, hw);
  long k = j * 64;
  int x = (int)(k / H), y = (int)(k - (long)x * H);
  u64 w = 0;
  for (int b = 0; k < ke; k++, b++) {
    w |= (u64)(src[(long)y * W + x] != 0) << b;
    if (++y == H) { y = 0; x++; }
  }
  words[(long)blockIdx.y * nw + j] = w;
}

// ------------------------------------------------------------------------------------ expand from runs
// ends = inclusive prefix sums of a mask's run lengths (run r covers [ends[r-1], ends[r]), runs of odd index are ones).
// A thread owns one word: binary search for the run that holds the word's first position, then walk.
__global__ __launch_bounds__(256) void expand_kernel(const int* __restrict__ ends, const long* __restrict__ off, int H, int W,
                                                     long nw, u64* __restrict__ words) {
  const long j = blockIdx.x * 256L + threadIdx.x;
  if (j >= nw) return;
  const long lo = off[blockIdx.y], hi = off[blockIdx.y + 1];
  const long hw = (long)H * W, k0 = j * 64, kend = min(k0 + 64, hw);
  long a = lo, b = hi;               // first r in [lo, hi) with ends[r] > k0
  while (a < b) {
    const long mid = (a + b) >> 1;
    if ((long)ends[mid] > k0) b = mid; else a = mid + 1;
  }
  long r = a, pos = k0;
  u64 w = 0;
  while (r < hi && pos < kend) {
    const long eraw = ends[r], e = min(eraw, kend);
    if (e > pos) {
      if ((r - lo) & 1) w |= low_bits((int)(e - pos)) << (int)(pos - k0);
      pos = e;
    }
    if (eraw >= kend) break;
    r++;
  }
  words[(long)blockIdx.y * nw + j] = w;
}

// ------------------------------------------------------------------------------------ record
__device__ __forceinline__ int block_reduce(int v, int op, int* sh) {   // op 0 sum, 1 min, 2 max; 256 threads
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const int a = sh[threadIdx.x], b = sh[threadIdx.x + o];
      sh[threadIdx.x] = op == 0 ? a + b : (op == 1 ? min(a, b) : max(a, b));
    }
    __syncthreads();
  }
  return sh[0];
}

// one block per mask: area, extent and `wrap` (some column x < W-1 has its bottom pixel and column x+1 its top pixel set:
// the run-based rleToBbox then reports the full height)
__global__ __launch_bounds__(256) void record_kernel(const u64* __restrict__ words, int H, int W, long nw, int* __restrict__ rec) {
  __shared__ int sh[256];
  const u64* wp = words + (long)blockIdx.x * nw;
  const long hw = (long)H * W;
  int area = 0, xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1, wrap = 0;
  for (long j = threadIdx.x; j < nw; j += 256) {
    const u64 w = wp[j];
    if (!w) continue;
    area += __popcll(w);
    const u64 nxt = j + 1 < nw ? wp[j + 1] : 0;
    const u64 pairs = w & ((w >> 1) | (nxt << 63));   // bit b: positions 64 j + b and 64 j + b + 1 both set
    const long k0 = j * 64, klast = k0 + 63 - __builtin_clzll(w);
    long k = k0 + __builtin_ctzll(w);
    xmin = min(xmin, (int)(k / H));
    xmax = max(xmax, (int)(klast / H));
    while (true) {   // the set bits of this word, column by column; k is a set bit
      const int x = (int)(k / H), y = (int)(k - (long)x * H);
      const long ce = (long)(x + 1) * H, e = min(ce, klast + 1);
      const u64 seg = (w >> (int)(k - k0)) & low_bits((int)(e - k));   // bit 0 is set
      ymin = min(ymin, y);
      ymax = max(ymax, y + 63 - __builtin_clzll(seg));
      if (e == ce && ce < hw) wrap |= (int)((pairs >> (int)(ce - 1 - k0)) & 1);
      if (e > klast) break;
      k = e + __builtin_ctzll(w >> (int)(e - k0));   // e - k0 < 64 and a set bit lies at or after e
    }
  }
  area = block_reduce(area, 0, sh);
  xmin = block_reduce(xmin, 1, sh);
  xmax = block_reduce(xmax, 2, sh);
  ymin = block_reduce(ymin, 1, sh);
  ymax = block_reduce(ymax, 2, sh);
  wrap = block_reduce(wrap, 2, sh);
  if (threadIdx.x < REC) {
    const int v[REC] = {area, xmin, xmax, ymin, ymax, wrap, 0, 0};
    rec[(long)blockIdx.x * REC + threadIdx.x] = (area || threadIdx.x == 0) ? v[threadIdx.x] : 0;   // empty mask: all zero
  }
}

// ------------------------------------------------------------------------------------ transitions
__device__ __forceinline__ u64 trans_word(const u64* __restrict__ wp, long j, long nw, long hw) {
  const u64 w = wp[j], carry = j ? wp[j - 1] >> 63 : 0;
  u64 t = w ^ ((w << 1) | carry);
  const int tail = (int)(hw & 63);
  if (j == nw - 1 && tail) t &= (1ULL << tail) - 1;
  return t;
}

__global__ __launch_bounds__(256) void trans_count_kernel(const u64* __restrict__ words, int H, int W, long nw, int* __restrict__ counts) {
  __shared__ int sh[256];
  const u64* wp = words + (long)blockIdx.x * nw;
  const long hw = (long)H * W;
  int c = 0;
  for (long j = threadIdx.x; j < nw; j += 256) c += __popcll(trans_word(wp, j, nw, hw));
  c = block_reduce(c, 0, sh);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// one block per mask walks its words 256 at a time; an exclusive scan of the words' counts places every position
__global__ __launch_bounds__(256) void trans_emit_kernel(const u64* __restrict__ words, int H, int W, long nw, const long* __restrict__ off,
                                                         int* __restrict__ pos) {
  __shared__ int sc[256];
  const u64* wp = words + (long)blockIdx.x * nw;
  const long hw = (long)H * W, lim = off[blockIdx.x + 1];
  long base = off[blockIdx.x];
  const int tid = threadIdx.x;
  for (long c0 = 0; c0 < nw; c0 += 256) {
    const long j = c0 + tid;
    u64 t = j < nw ? trans_word(wp, j, nw, hw) : 0;
    const int cnt = __popcll(t);
    sc[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int v = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    long at = base + sc[tid] - cnt;
    base += sc[255];
    while (t) {
      if (at < lim) pos[at] = (int)(j * 64 + __builtin_ctzll(t));
      at++;
      t &= t - 1;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ pair intersections
// one wave per (detection, ground truth): the boxes by rleToBbox's rule, then popcount(D & G) over the words of the
// overlapping columns (contiguous in this layout); -1 marks a pair of disjoint boxes (box_of: maskwords.h)
__global__ __launch_bounds__(256) void pair_kernel(const u64* __restrict__ dwords, const int* __restrict__ drec, int m,
                                                   const u64* __restrict__ gwords, const int* __restrict__ grec, int n, int H,
                                                   long nw, int* __restrict__ out) {
  const long pair = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (pair >= (long)m * n) return;
  const int lane = threadIdx.x & 63;
  const int d = (int)(pair / n), g = (int)(pair - (long)d * n);
  int dx, dy, dw, dh, gx, gy, gw, gh;
  box_of(drec + (long)d * REC, H, dx, dy, dw, dh);
  box_of(grec + (long)g * REC, H, gx, gy, gw, gh);
  const int xlo = max(dx, gx), ow = min(dx + dw, gx + gw) - xlo;
  const int oh = min(dy + dh, gy + gh) - max(dy, gy);
  if (ow <= 0 || oh <= 0) {
    if (lane == 0) out[pair] = -1;
    return;
  }
  // columns outside [xlo, xlo + ow) are empty in at least one of the two masks, so whole words may be taken at both ends
  const long j0 = max(((long)xlo * H) >> 6, 0L), j1 = min(((long)(xlo + ow) * H + 63) >> 6, nw);
  const u64* dp = dwords + (long)d * nw;
  const u64* gp = gwords + (long)g * nw;
  int c = 0;
  for (long j = j0 + lane; j < j1; j += 64) c += __popcll(dp[j] & gp[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) out[pair] = c;
}

// ------------------------------------------------------------------------------------ entry points
static int records(const u64* words, int n, int H, int W, int32_t* rec, hipStream_t s) {
  hipLaunchKernelGGL(record_kernel, dim3(n), dim3(256), 0, s, words, H, W, words_of(H, W), rec);
  MMT_LAUNCH_CHECK();
  return 0;
}

// for mmt_paste_mask_words (csrc/masks.hip), whose kernel writes words and leaves the records to this one
int mmt_mask_records(const uint64_t* words, int n, int H, int W, int32_t* rec, hipStream_t s) {
  return records((const u64*)words, n, H, W, rec, s);
}

extern "C" int mmt_mask_pack(const uint8_t* masks, int n, int H, int W, uint64_t* words, int32_t* rec, void* stream) {
  if (n < 0 || n > MAX_MASKS || bad_size(H, W)) return MMT_EINVAL;
  if (n == 0) return 0;
  if (!masks || !words || !rec) return MMT_EINVAL;
  const long nw = words_of(H, W);
  if (H <= STRIP_MAX_H) {
    const size_t lds = (size_t)64 * (((H + 63) >> 6) | 1) * sizeof(u64);
    hipLaunchKernelGGL(pack_strip_kernel, dim3(mmt_cdiv(W, 64), n), dim3(256), lds, (hipStream_t)stream, masks, H, W, nw, (u64*)words);
  } else {
    hipLaunchKernelGGL(pack_word_kernel, dim3(mmt_cdiv(nw, 256), n), dim3(256), 0, (hipStream_t)stream, masks, H, W, nw, (u64*)words);
  }
  MMT_LAUNCH_CHECK();
  return records((const u64*)words, n, H, W, rec, (hipStream_t)stream);
}

extern "C" int mmt_mask_expand(const int32_t* ends, const int64_t* off, int n, int H, int W, uint64_t* words, int32_t* rec,
                               void* stream) {
  if (n < 0 || n > MAX_MASKS || bad_size(H, W)) return MMT_EINVAL;
  if (n == 0) return 0;
  if (!ends || !off || !words || !rec) return MMT_EINVAL;
  const long nw = words_of(H, W);
  hipLaunchKernelGGL(expand_kernel, dim3(mmt_cdiv(nw, 256), n), dim3(256), 0, (hipStream_t)stream, ends, (const long*)off, H, W, nw,
                     (u64*)words);
  MMT_LAUNCH_CHECK();
  return records((const u64*)words, n, H, W, rec, (hipStream_t)stream);
}

extern "C" int mmt_mask_transition_counts(const uint64_t* words, int n, int H, int W, int32_t* counts, void* stream) {
  if (n < 0 || n > MAX_MASKS || bad_size(H, W)) return MMT_EINVAL;
  if (n == 0) return 0;
  if (!words || !counts) return MMT_EINVAL;
  hipLaunchKernelGGL(trans_count_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const u64*)words, H, W, words_of(H, W), counts);
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmt_mask_transition_positions(const uint64_t* words, int n, int H, int W, const int64_t* off, int32_t* pos,
                                             void* stream) {
  if (n < 0 || n > MAX_MASKS || bad_size(H, W)) return MMT_EINVAL;
  if (n == 0) return 0;
  if (!words || !off || !pos) return MMT_EINVAL;
  hipLaunchKernelGGL(trans_emit_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const u64*)words, H, W, words_of(H, W),
                     (const long*)off, pos);
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmt_mask_pair_intersections(const uint64_t* dwords, const int32_t* drec, int m, const uint64_t* gwords,
                                           const int32_t* grec, int n, int H, int W, int32_t* inter, void* stream) {
  if (m < 0 || n < 0 || m > MAX_MASKS || n > MAX_MASKS || bad_size(H, W)) return MMT_EINVAL;
  if (m == 0 || n == 0) return 0;
  if (!dwords || !drec || !gwords || !grec || !inter) return MMT_EINVAL;
  hipLaunchKernelGGL(pair_kernel, dim3(mmt_cdiv((long)m * n, 4)), dim3(256), 0, (hipStream_t)stream, (const u64*)dwords, drec, m,
                     (const u64*)gwords, grec, n, H, words_of(H, W), inter);
  MMT_LAUNCH_CHECK();
  return 0;
}
