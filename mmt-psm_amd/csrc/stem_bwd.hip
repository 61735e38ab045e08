// Backward of the ResNet stem (FREEZE_CONV_BODY_AT 0): include/mmtpsm.h: mmt_maxpool3x3s2_backward, mmt_stem_wgrad.
//
// The max pool's gradient is a GATHER: a thread owns four channels of a 2 x 2 block of the pool's input, and for each element
// visits the (at most 2 x 2) windows that contain it in ascending (ho, wo) order and adds a window's gradient when the element is
// that window's FIRST maximum in (kh, kw) scan order -- ATen's rule (a later tap replaces the running maximum only when it is
// strictly larger; taps outside the image never win).  The ReLU mask of the pooled tensor's producer, (y > 0), is applied on the
// way out.  Every element is written, zeros included: no atomics, nothing for the caller to clear (the form of gconv_dgrad_s2_kernel, csrc/conv_group.hip).
//
// The weight gradient of the 7x7 / stride 2 / pad 3, 3 -> 64 convolution reads the image itself (NCHW, three channels) and runs on
// the exact fp32-input MFMA (v_mfma_f32_16x16x4_f32) like csrc/conv_group.hip: M = 64 output channels (one 16-channel slice per
// wave), N = the 147 (kh, kw, ci) filter elements in the parameter's own memory order, padded to ten 16-column tiles, K = output
// pixels, four per MFMA.  A block keeps its 64 x 160 sums in accumulators over a strided range of 4 x 16 pixel tiles -- image
// tile with halo and gradient tile in LDS, the next tile's operands on their way into registers while this tile's MFMAs run -- and
// adds them to dw with fp32 atomics (the form of mmt_conv_wgrad).  Deterministic mode (mmt_stem_wgrad_ordered): the same kernel is
// handed a workspace, stores its sums there with plain 16-byte stores instead, and a second launch (csrc/ordered.h) adds a dw
// element's partials in ascending block order.
#include "common.h"
#include "ordered.h"

namespace {

// One thread owns four channels of the 2 x 2 block of y at rows 2a, 2a + 1 and columns 2b, 2b + 1.  The (at most four) windows that
// contain one of its elements are (a + i, b + j), i, j in {0, 1}; together they span the 5 x 5 patch at (2a - 1, 2b - 1), read once
// into registers: 6.25 loads per element instead of 9 per (element, window).
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ y, const float* __restrict__ g, float* __restrict__ dy,
                                                          int N, int H, int W, int C, int Ho, int Wo) {
  const int C4 = C / 4;
  const long total = (long)N * Ho * Wo * C4;
  const float NEG = -__builtin_huge_valf();
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c4 = (int)(idx % C4);
    long r = idx / C4;
    const int b = (int)(r % Wo); r /= Wo;
    const int a = (int)(r % Ho);
    const int n = (int)(r / Ho);
    const float* yn = y + (long)n * H * W * C + c4 * 4;
    // the patch from clamped addresses (all loads in flight at once); a tap outside the image never wins: -inf
    f32x4 t[5][5];
#pragma unroll
    for (int pr = 0; pr < 5; ++pr) {
      const int ih = 2 * a - 1 + pr;
      const int ihc = min(max(ih, 0), H - 1);
#pragma unroll
      for (int pc = 0; pc < 5; ++pc) {
        const int iw = 2 * b - 1 + pc;
        const int iwc = min(max(iw, 0), W - 1);
        const f32x4 v = *reinterpret_cast<const f32x4*>(yn + ((long)ihc * W + iwc) * C);
        t[pr][pc] = (ih == ihc && iw == iwc) ? v : (f32x4){NEG, NEG, NEG, NEG};
      }
    }
    // per window: its gradient and the place (kh * 3 + kw) of its first maximum in scan order (a later tap replaces the running
    // maximum only when it is strictly larger); -1 for a window the pool does not have
    f32x4 gw[2][2];
    int first[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool have = a + i < Ho && b + j < Wo;
        const int hoc = min(a + i, Ho - 1), woc = min(b + j, Wo - 1);
        gw[i][j] = *reinterpret_cast<const f32x4*>(g + (((long)n * Ho + hoc) * Wo + woc) * C + c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float m = NEG;
          int at = -1;
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            const float v = t[2 * i + k / 3][2 * j + k % 3][e];
            if (v > m) { m = v; at = k; }
          }
          first[i][j][e] = have ? at : -1;
        }
      }
    // element (di, dj) of the block sits at (1 + di - 2 i, 1 + dj - 2 j) of window (i, j); its windows in ascending (ho, wo) order
#pragma unroll
    for (int di = 0; di < 2; ++di)
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) {
        const int h = 2 * a + di, w = 2 * b + dj;
        if (h >= H || w >= W) continue;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i <= di; ++i)
#pragma unroll
          for (int j = 0; j <= dj; ++j) {
            const int me = (1 + di - 2 * i) * 3 + (1 + dj - 2 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (first[i][j][e] == me) acc[e] += gw[i][j][e];
          }
        const f32x4 v = t[1 + di][1 + dj];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (!(v[e] > 0.f)) acc[e] = 0.f;
        *reinterpret_cast<f32x4*>(dy + (((long)n * H + h) * W + w) * C + c4 * 4) = acc;
      }
  }
}

// ---- weight gradient of the stem convolution
constexpr int SW_TH = 4;                      // output rows per tile
constexpr int SW_IR = (SW_TH - 1) * 2 + 7;    // image rows of a tile, halo included
constexpr int SW_IC = 15 * 2 + 7;             // image columns
constexpr int SW_ICP = SW_IC + 2;             // row stride in LDS
constexpr int SW_LS = 64 + 4;                 // floats per gradient pixel in LDS (16-byte aligned, pixel p starts at bank 4 p)
constexpr int SW_NT = 10;                     // 16-column tiles over the 147 filter elements
constexpr int SW_X = 3 * SW_IR * SW_ICP;      // floats of the image tile

struct SwArgs {
  const float* x;         // [N][3][H][W]
  const float* dy;        // [N][Ho][Wo][64]
  const float* rowscale;  // [64] or null
  float* dw;              // [64][7][7][3], accumulated into
  float* ws;              // null: atomics into dw.  Else the ordered form's partials, [block][wave][column tile][lane][e]
  int N, H, W, Ho, Wo;
  int tiles_w, tiles_img, tiles;
};

// The ordered form's workspace: a block's accumulators as they sit in registers, one 16-byte store per lane and column tile (1 KB in
// a row per wave), the 13 padding columns included.  workspace quad -> dw index of its element e (csrc/ordered.h: ordered_finish_wide)
constexpr int SW_BLOCK_FLOATS = 4 * SW_NT * 64 * 4;
struct SwFinishMap {
  __device__ long operator()(long q, int e) const {
    const int lane = (int)(q & 63), t = (int)((q >> 6) % SW_NT), wv = (int)((q >> 6) / SW_NT);
    const int el = t * 16 + (lane & 15);
    return el < 147 ? (long)(wv * 16 + 4 * (lane >> 4) + e) * 147 + el : -1;
  }
};

__global__ __launch_bounds__(256) void stem_wgrad_kernel(SwArgs p) {
  __shared__ __attribute__((aligned(16))) float xl[SW_X];
  __shared__ __attribute__((aligned(16))) float dl[SW_TH * 16 * SW_LS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;

  // column j of tile t is filter element 16 t + j = (kh * 7 + kw) * 3 + ci; the 13 columns past 147 repeat the last element and
  // are not written out
  int off[SW_NT];
#pragma unroll
  for (int t = 0; t < SW_NT; ++t) {
    const int e = min(t * 16 + i, 146);
    const int ci = e % 3, tap = e / 3;
    off[t] = (ci * SW_IR + tap / 7) * SW_ICP + tap % 7;
  }
  f32x4 acc[SW_NT];
#pragma unroll
  for (int t = 0; t < SW_NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // a tile's operands travel global -> registers -> LDS; the loads of the NEXT tile are issued before this tile's MFMAs and land
  // while they run (6 image values and 4 x 4 gradient values per thread)
  constexpr int XPT = (3 * SW_IR * SW_IC + 255) / 256;
  float xr[XPT];
  f32x4 dr[SW_TH];
  auto fetch = [&](int tile) {
    const int n = tile / p.tiles_img, tin = tile - n * p.tiles_img;
    const int oh0 = (tin / p.tiles_w) * SW_TH, ow0 = (tin % p.tiles_w) * 16;
#pragma unroll
    for (int k = 0; k < XPT; ++k) {
      const int idx = threadIdx.x + k * 256;
      const int c = idx % SW_IC, rc = idx / SW_IC;
      const int r = rc % SW_IR, ci = rc / SW_IR;
      const int h = 2 * oh0 - 3 + r, w = 2 * ow0 - 3 + c;
      float val = 0.f;
      if (ci < 3 && h >= 0 && w >= 0 && h < p.H && w < p.W) val = p.x[(((long)n * 3 + ci) * p.H + h) * p.W + w];
      xr[k] = val;
    }
#pragma unroll
    for (int k = 0; k < SW_TH; ++k) {
      const int idx = threadIdx.x + k * 256;
      const int pix = idx >> 4, v = idx & 15;
      const int oh = oh0 + (pix >> 4), ow = ow0 + (pix & 15);
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (oh < p.Ho && ow < p.Wo) val = *reinterpret_cast<const f32x4*>(p.dy + (((long)n * p.Ho + oh) * p.Wo + ow) * 64 + v * 4);
      dr[k] = val;
    }
  };
  if ((int)blockIdx.x < p.tiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    __syncthreads();   // the previous tile's reads are done
#pragma unroll
    for (int k = 0; k < XPT; ++k) {
      const int idx = threadIdx.x + k * 256;
      const int c = idx % SW_IC, rc = idx / SW_IC;
      if (rc < 3 * SW_IR) xl[rc * SW_ICP + c] = xr[k];
    }
#pragma unroll
    for (int k = 0; k < SW_TH; ++k) {
      const int idx = threadIdx.x + k * 256;
      *reinterpret_cast<f32x4*>(dl + (idx >> 4) * SW_LS + (idx & 15) * 4) = dr[k];
    }
    __syncthreads();
    if (tile + (int)gridDim.x < p.tiles) fetch(tile + gridDim.x);
    // A[row = co][k = pixel] = dy, B[k = pixel][col = filter element] = x at the element's tap and channel
#pragma unroll
    for (int r = 0; r < SW_TH; ++r) {
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        const int pc = ch * 4 + kq;
        const float a = dl[(r * 16 + pc) * SW_LS + wv * 16 + i];
        const float* xb = xl + (2 * r) * SW_ICP + 2 * pc;
#pragma unroll
        for (int t = 0; t < SW_NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[off[t]], acc[t], 0, 0, 0);
      }
    }
  }

  // D[row = 4 (lane >> 4) + e -> co][col = lane & 15 -> filter element]
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int co = wv * 16 + 4 * kq + e;
    const float rs = p.rowscale ? p.rowscale[co] : 1.f;
    if (p.ws) {                                       // (wave-uniform) ordered form: scaled in place, stored below
#pragma unroll
      for (int t = 0; t < SW_NT; ++t) acc[t][e] *= rs;
      continue;
    }
#pragma unroll
    for (int t = 0; t < SW_NT; ++t) {
      const int el = t * 16 + i;
      if (el < 147) atomicAdd(p.dw + co * 147 + el, rs * acc[t][e]);
    }
  }
  if (p.ws) {
    float* wp = p.ws + (long)blockIdx.x * SW_BLOCK_FLOATS + (wv * SW_NT * 64 + lane) * 4;
#pragma unroll
    for (int t = 0; t < SW_NT; ++t) *reinterpret_cast<f32x4*>(wp + t * 256) = acc[t];
  }
}

}  // namespace

extern "C" int mmt_maxpool3x3s2_backward(const float* y, const float* g, float* dy, int N, int H, int W, int C, void* stream) {
  if (!y || !g || !dy || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return MMT_EINVAL;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long total = (long)N * Ho * Wo * (C / 4);   // one thread per 2 x 2 block of y and four channels
  long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, g, dy, N, H, W, C, Ho, Wo);
  MMT_LAUNCH_CHECK();
  return 0;
}

namespace {

// the shape half of the arguments -> the block count (a function of the shape alone), 0 for a shape that is not taken
int stem_wgrad_blocks(SwArgs& a, int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  a.N = N; a.H = H; a.W = W; a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
  a.tiles_w = mmt_cdiv(a.Wo, 16);
  a.tiles_img = a.tiles_w * mmt_cdiv(a.Ho, SW_TH);
  const long tiles = (long)a.tiles_img * N;
  if (tiles > 0x7fffffffL) return 0;
  a.tiles = (int)tiles;
  // two blocks per CU: pixel ranges across blocks, summed by the atomics (9408 per block) or in block order by the finish
  return a.tiles < 512 ? a.tiles : 512;
}

}  // namespace

extern "C" int mmt_stem_wgrad(const float* x, const float* dy, const float* rowscale, float* dw, int N, int H, int W, void* stream) {
  SwArgs a{};
  const int blocks = stem_wgrad_blocks(a, N, H, W);
  if (!x || !dy || !dw || blocks == 0) return MMT_EINVAL;
  a.x = x; a.dy = dy; a.rowscale = rowscale; a.dw = dw;
  hipLaunchKernelGGL(stem_wgrad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" long mmt_stem_wgrad_ws_floats(int N, int H, int W) {
  SwArgs a{};
  const int blocks = stem_wgrad_blocks(a, N, H, W);
  return blocks == 0 ? MMT_EINVAL : (long)blocks * SW_BLOCK_FLOATS;
}

extern "C" int mmt_stem_wgrad_ordered(const float* x, const float* dy, const float* rowscale, float* dw, int N, int H, int W, float* ws,
                                      long ws_floats, void* stream) {
  SwArgs a{};
  const int blocks = stem_wgrad_blocks(a, N, H, W);
  if (!x || !dy || !dw || blocks == 0 || !ws || ws_floats < (long)blocks * SW_BLOCK_FLOATS) return MMT_EINVAL;
  a.x = x; a.dy = dy; a.rowscale = rowscale; a.dw = dw; a.ws = ws;
  hipLaunchKernelGGL(stem_wgrad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  MMT_LAUNCH_CHECK();
  return ordered_finish_wide(ws, blocks, SW_BLOCK_FLOATS, dw, SwFinishMap{}, (hipStream_t)stream);
}
