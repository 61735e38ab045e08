// Polygons rasterised at IMAGE size into the run-length codec's mask words (csrc/maskeval.hip: bit k = pixel (y = k % H,
// x = k / H), tail bits zero), and the words summed back into a row-major integral map:
//
//   polygon_mask_words  <- structures/segmentation_mask.py:127-137 (Polygons.convert("mask")): pycoco/_mask.pyx frPyObjects ->
//                          pycoco/maskApi.c:166-206 (rleFrPoly), :53-74 (rleMerge, union) and :47-51 (rleDecode)
//   mask_words_integral <- structures/segmentation_mask.py:174-181 (SegmentationMask.decode: the sum over instances)
//
// csrc/masks.hip states the identity: after the x5 boundary walk rleFrPoly turns the crossings a_j = x * H + y into
//   mask[q] = (#{j : a_j <= q}) mod 2      (q = column-major pixel index).
// polygon_kernel there keeps one ROI's M x M <= 32 x 32 pixels in a wave's registers.  At image size the same mask is a PREFIX
// XOR over a toggle bitmap: flip bit a_j for every crossing with a_j < H * W (a crossing at a_j = H * W lies behind the last
// pixel and is dropped, never written), then mask[q] = T[0] ^ ... ^ T[q].  An instance is the OR of its polygons' fills.
//
// Phases are separate launches (the rule of csrc/ordered.h: nothing is handed from block to block inside a launch):
//   1 clear the toggle planes (one per polygon)             4 fill: a thread owns word j of an instance, loops over its polygons:
//   2 walk: one wave per (edge, chunk of steps); every        in-word prefix XOR by shifts, carry = wave scan of the word
//     step of the walk is closed-form in t, a crossing at     parities ^ the 64-word block's prefix of phase 3; OR; one store
//     step d needs steps d and d - 1 only; 64-bit atomicXor 5 records (csrc/maskeval.hip)
//   3 parity of every 64-word block of a plane, then their exclusive prefix per plane
// The atomics are integer XORs: exact, order-free, the same bits run to run.
//
// Built with -ffp-contract=off: the double expressions of the walk must round like the C code.
#include "common.h"

typedef unsigned long long u64;

#define PF_MAX_MASKS 65535     // instances per call: the fill grid's second dimension
#define PF_STEPS 512           // steps of one edge that a wave takes per visit: 8 per lane
#define PF_MAX_CHUNKS 16

static inline bool pf_bad_size(int H, int W) { return H <= 0 || W <= 0 || (long)H * (long)W >= (1L << 31); }
static inline long pf_words(int H, int W) { return ((long)H * W + 63) >> 6; }
static inline long pf_blocks(long nw) { return (nw + 63) >> 6; }

// ------------------------------------------------------------------------------------ 2. walk
// point t of the edge's dense walk (maskApi.c:176-186)
__device__ __forceinline__ void pf_point(bool xmajor, int xs, int ys, double s, int t, int& u, int& v) {
  if (xmajor) { u = t + xs; v = (int)(ys + s * t + .5); }
  else { v = t + ys; u = (int)(xs + s * t + .5); }
}

__global__ __launch_bounds__(256) void pf_walk_kernel(const float* __restrict__ xy, const int* __restrict__ poly_off, int NP,
                                                      int v_first, int n_edges, int H, int W, long nw, u64* __restrict__ planes) {
  const int lane = threadIdx.x & 63;
  const long e = blockIdx.x * 4L + (threadIdx.x >> 6);   // wave-uniform
  if (e >= n_edges) return;
  const int vtx = v_first + (int)e;
  // the polygon that owns vertex vtx: the last p with poly_off[p] <= vtx (empty polygons repeat an offset)
  int lo = 0, hi = NP;            // first p in [0, NP] with poly_off[p] > vtx
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (poly_off[mid] > vtx) hi = mid; else lo = mid + 1;
  }
  const int p = lo - 1;
  if (p < 0 || p >= NP) return;
  const int v0 = poly_off[p], k = poly_off[p + 1] - v0;
  const int j = vtx - v0, j1 = (j + 1 == k) ? 0 : j + 1;
  const double scale = 5;
  int xs = (int)(scale * (double)xy[(long)(v0 + j) * 2 + 0] + .5), ys = (int)(scale * (double)xy[(long)(v0 + j) * 2 + 1] + .5);
  int xe = (int)(scale * (double)xy[(long)(v0 + j1) * 2 + 0] + .5), ye = (int)(scale * (double)xy[(long)(v0 + j1) * 2 + 1] + .5);
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  if (dx == 0) return;            // the column never changes: no crossing
  const bool xmajor = dx >= dy;
  const bool flip = (xmajor && xs > xe) || (!xmajor && ys > ye);
  if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
  const double s = xmajor ? (double)(ye - ys) / dx : (double)(xe - xs) / dy;
  const long n = xmajor ? dx : dy;
  const long hw = (long)H * W;
  u64* plane = planes + (long)p * nw;
  for (long d0 = 1 + (long)blockIdx.y * PF_STEPS; d0 <= n; d0 += (long)gridDim.y * PF_STEPS) {
    const long dend = min(d0 + PF_STEPS - 1, n);
    for (long d = d0 + lane; d <= dend; d += 64) {
      int u, v, pu, pv;
      pf_point(xmajor, xs, ys, s, (int)(flip ? n - d : d), u, v);
      pf_point(xmajor, xs, ys, s, (int)(flip ? n - d + 1 : d - 1), pu, pv);
      if (u == pu) continue;
      double xd = (double)(u < pu ? u : u - 1);
      xd = (xd + .5) / scale - .5;
      if (floor(xd) != xd || xd < 0 || xd > W - 1) continue;
      double yd = (double)(v < pv ? v : pv);
      yd = (yd + .5) / scale - .5;
      if (yd < 0) yd = 0; else if (yd > H) yd = H;
      yd = ceil(yd);
      const long a = (long)(int)xd * H + (int)yd;     // 0 <= a <= H * W
      if (a < hw) atomicXor(plane + (a >> 6), 1ULL << (int)(a & 63));
    }
  }
}

// ------------------------------------------------------------------------------------ 3. block parities
// one wave per 64-word block of a plane: par[p][b] = parity of the block's toggles
__global__ __launch_bounds__(256) void pf_block_parity_kernel(const u64* __restrict__ planes, int NP, long nw, long nb,
                                                              int* __restrict__ par) {
  const int lane = threadIdx.x & 63;
  const long b = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (b >= nb) return;
  const long j = b * 64 + lane;
  for (int p = blockIdx.y; p < NP; p += gridDim.y) {
    const u64 t = j < nw ? planes[(long)p * nw + j] : 0;
    const u64 odd = __ballot(__popcll(t) & 1);
    if (lane == 0) par[(long)p * nb + b] = __popcll(odd) & 1;
  }
}

// one wave per plane: par[p][b] <- par[p][0] ^ ... ^ par[p][b - 1], in place
__global__ __launch_bounds__(64) void pf_block_prefix_kernel(long nb, int* __restrict__ par) {
  const int lane = threadIdx.x;
  int* pp = par + (long)blockIdx.x * nb;
  int carry = 0;
  for (long b0 = 0; b0 < nb; b0 += 64) {
    const long b = b0 + lane;
    const int v = b < nb ? pp[b] : 0;
    const u64 odd = __ballot(v & 1);
    if (b < nb) pp[b] = carry ^ (__popcll(odd & ((1ULL << lane) - 1)) & 1);
    carry ^= __popcll(odd) & 1;
  }
}

// ------------------------------------------------------------------------------------ 4. fill
__global__ __launch_bounds__(256) void pf_fill_kernel(const u64* __restrict__ planes, const int* __restrict__ par,
                                                      const int* __restrict__ inst_poly, int NP, long nw, long nb, int tail,
                                                      u64* __restrict__ words) {
  const int lane = threadIdx.x & 63;
  const long b = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (b >= nb) return;            // whole waves: the ballots below are complete
  const int g = blockIdx.y;
  const long j = b * 64 + lane;
  const int ps = max(inst_poly[2 * g], 0), pe = min(inst_poly[2 * g + 1], NP);
  u64 acc = 0;
  for (int p = ps; p < pe; p++) {
    const u64 t = j < nw ? planes[(long)p * nw + j] : 0;
    u64 x = t;                    // bit i <- t[0] ^ ... ^ t[i]
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
    const u64 odd = __ballot((int)(x >> 63));
    const int carry = par[(long)p * nb + b] ^ (__popcll(odd & ((1ULL << lane) - 1)) & 1);
    acc |= carry ? ~x : x;
  }
  if (j < nw) {
    if (j == nw - 1 && tail) acc &= (1ULL << tail) - 1;
    words[(long)g * nw + j] = acc;
  }
}

// ------------------------------------------------------------------------------------ integral map
// pack_strip_kernel (csrc/maskeval.hip) backwards.  A block owns a tile of 64 columns x 64 rows: lane = column, its 64 rows are
// 64 consecutive bits of the flattening (cut out of two words).  The block's four waves share the image's instances, each counts
// its own into 64 registers, and the four counts meet in LDS (integer adds: any order gives the same sums).  Row i of the tile is
// then 64 consecutive LDS words: every store is 64 consecutive ints of one image row.
__global__ __launch_bounds__(256) void pf_integral_kernel(const u64* __restrict__ words, int g0, int g1, int H, int W, long nw,
                                                          int* __restrict__ seg) {
  __shared__ int tile[64 * 64];   // [row][column]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nby = (H + 63) >> 6;
  const int bx = blockIdx.x / nby, by = blockIdx.x - bx * nby;   // the bands of one strip of columns are neighbours
  const int x = bx * 64 + lane, y0 = by * 64, ny = min(64, H - y0);
  const bool in = x < W;
  const long k = (long)x * H + y0, jw = k >> 6;
  const int s = (int)(k & 63);
  const u64 keep = ny < 64 ? (1ULL << ny) - 1 : ~0ULL;
  for (int i = threadIdx.x; i < 64 * 64; i += 256) tile[i] = 0;
  int cnt[64];
#pragma unroll
  for (int i = 0; i < 64; i++) cnt[i] = 0;
  for (int g = g0 + wave; g < g1; g += 4) {
    const u64* wp = words + (long)g * nw;
    u64 v = 0;
    if (in) {                     // (x < W: k < H * W, so jw < nw)
      v = wp[jw] >> s;
      if (s && jw + 1 < nw) v |= wp[jw + 1] << (64 - s);
      v &= keep;
    }
    const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int i = 0; i < 32; i++) {
      cnt[i] += (lo >> i) & 1u;
      cnt[32 + i] += (hi >> i) & 1u;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 64; i++)
    if (cnt[i]) atomicAdd(&tile[i * 64 + lane], cnt[i]);
  __syncthreads();
  if (!in) return;
  for (int i = wave; i < ny; i += 4) seg[(long)(y0 + i) * W + x] = tile[i * 64 + lane];
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int mmt_polygon_mask_words_workspace(int NP, int H, int W, int64_t* words_needed) {
  if (NP < 0 || pf_bad_size(H, W) || !words_needed) return MMT_EINVAL;
  const long nw = pf_words(H, W), nb = pf_blocks(nw);
  *words_needed = (int64_t)NP * nw + ((int64_t)NP * nb + 1) / 2;   // planes, then one int per 64-word block
  return 0;
}

extern "C" int mmt_polygon_mask_words(const float* poly_xy, const int32_t* poly_off, int NP, const int32_t* inst_poly, int G,
                                      int H, int W, uint64_t* ws, int64_t ws_words, uint64_t* words, int32_t* rec,
                                      void* stream) {
  if (G < 0 || G > PF_MAX_MASKS || NP < 0 || pf_bad_size(H, W)) return MMT_EINVAL;
  if (G == 0) return 0;
  if (!poly_off || !inst_poly || !words || !rec) return MMT_EINVAL;
  int64_t need = 0;
  mmt_polygon_mask_words_workspace(NP, H, W, &need);
  if (ws_words < need || (need > 0 && !ws)) return MMT_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  // what the launches are sized by lives on the device: the polygon ranges (checked here) and the vertex range
  int32_t voff[2] = {0, 0};
  {
    int32_t buf[2 * 2048];
    for (int g = 0; g < G; g += 2048) {
      const int n = G - g < 2048 ? G - g : 2048;
      hipError_t er = hipMemcpyAsync(buf, inst_poly + 2 * (long)g, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost, s);
      if (er == hipSuccess) er = hipStreamSynchronize(s);
      if (er != hipSuccess) return (int)er;
      for (int i = 0; i < n; i++)
        if (buf[2 * i] < 0 || buf[2 * i] > NP || buf[2 * i + 1] < 0 || buf[2 * i + 1] > NP) return MMT_EINVAL;
    }
    hipError_t er = hipMemcpyAsync(&voff[0], poly_off, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipMemcpyAsync(&voff[1], poly_off + NP, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    if (er != hipSuccess) return (int)er;
  }
  const long n_edges = (long)voff[1] - voff[0];   // a polygon of k vertices has k edges
  if (voff[0] < 0 || n_edges < 0 || (n_edges > 0 && !poly_xy)) return MMT_EINVAL;
  const long nw = pf_words(H, W), nb = pf_blocks(nw);
  u64* planes = (u64*)ws;
  int* par = (int*)(planes + (long)NP * nw);
  if (NP > 0) {
    const hipError_t er = hipMemsetAsync(planes, 0, sizeof(u64) * (size_t)NP * nw, s);
    if (er != hipSuccess) return (int)er;
    if (n_edges > 0) {
      const int chunks = (int)min((long)PF_MAX_CHUNKS, max(1L, (5L * max(H, W) + PF_STEPS - 1) / PF_STEPS));
      hipLaunchKernelGGL(pf_walk_kernel, dim3(mmt_cdiv(n_edges, 4), chunks), dim3(256), 0, s, poly_xy, poly_off, NP, voff[0],
                         (int)n_edges, H, W, nw, planes);
      MMT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pf_block_parity_kernel, dim3(mmt_cdiv(nb, 4), NP < 65535 ? NP : 65535), dim3(256), 0, s, planes, NP, nw,
                       nb, par);
    MMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(pf_block_prefix_kernel, dim3(NP), dim3(64), 0, s, nb, par);
    MMT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pf_fill_kernel, dim3(mmt_cdiv(nb, 4), G), dim3(256), 0, s, planes, par, inst_poly, NP, nw, nb,
                     (int)(((long)H * W) & 63), (u64*)words);
  MMT_LAUNCH_CHECK();
  return mmt_mask_records(words, G, H, W, rec, s);
}

extern "C" int mmt_mask_words_integral(const uint64_t* words, const int32_t* img_off, int N, int H, int W, int32_t* seg,
                                       void* stream) {
  if (N < 0 || pf_bad_size(H, W)) return MMT_EINVAL;
  if (N == 0) return 0;
  if (!img_off || !seg) return MMT_EINVAL;
  for (int n = 0; n < N; n++)
    if (img_off[n] < 0 || img_off[n + 1] < img_off[n]) return MMT_EINVAL;
  if (img_off[N] > PF_MAX_MASKS || (img_off[N] > img_off[0] && !words)) return MMT_EINVAL;
  const long nw = pf_words(H, W);
  const long tiles = (long)((H + 63) >> 6) * ((W + 63) >> 6);   // (H * W < 2^31: fewer than 2^19)
  for (int n = 0; n < N; n++) {
    hipLaunchKernelGGL(pf_integral_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const u64*)words,
                       img_off[n], img_off[n + 1], H, W, nw, seg + (long)n * H * W);
    MMT_LAUNCH_CHECK();
  }
  return 0;
}
