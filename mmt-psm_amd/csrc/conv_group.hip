// Grouped 3x3 convolution (ResNeXt conv2: C = G * Cg channels in and out, pad 1, stride 1 or 2) on the exact fp32-input MFMA
// (v_mfma_f32_16x16x4_f32): forward, data gradient, weight gradient.  include/mmtpsm.h: mmt_gconv3x3_*.
//
// One block = one spatial tile of TH x 16 output pixels x one channel slab of CS = max(Cg, 32) channels.  The slab's input tile (with
// its halo) is read ONCE into LDS and serves all 9 taps and every group of the slab.  A wave owns a 16-channel slice of the slab's
// outputs (the MFMA's M), 16 pixels of an output row are its N, and K runs over (tap, input channel of the slice's group).  Cg = 8
// packs two groups block-diagonally into one 16 x 16 tile (the off-diagonal weights are zeros in registers: half of that stage's
// MFMA work is padding; the stage sits near the HBM line either way).  Weights come from global memory (L2) straight into
// registers, four consecutive channels per lane: K is walked in the order (4 kq + j) so that one 16-byte load feeds four MFMAs on
// both operands.
//
// The data gradient at stride 1 is the same kernel on transformed weights wt[ci][2-kh][2-kw][co] = scale[co] w[co][kh][kw][ci]
// (gconv_flip_kernel); at stride 2 a gather kernel by parity class of the dx pixel (gconv_dgrad_s2_kernel): every dx element has
// one owner and is written, zeros included.
// The weight gradient keeps a slab's (co, ci, tap) tile sums in accumulators over a strided range of spatial tiles and adds them to
// dw with fp32 atomics (the form of mmt_conv_wgrad).
#include "common.h"

namespace {

struct GcArgs {
  const float* x;      // [N][IH][IW][C]
  const float* w;      // [C][3][3][Cg]
  const float* scale;  // [C] or null
  const float* shift;  // [C] or null
  const float* mask;   // like y, or null: y = mask > 0 ? y : 0
  float* y;            // [N][OH][OW][C]
  int N, IH, IW, OH, OW, C, Cg;
  int relu;
  int tiles_w, tiles;  // spatial tiles per image row / per image
};

template <int CS> constexpr int lds_stride() { return CS + 4; }   // floats per pixel: 16-byte aligned, pixel p starts at bank 4 p (mod 64)

// x tile with halo -> LDS [IR][IC][CS + 4]; zeros outside the image (the padding)
template <int CS, int S, int TH>
__device__ __forceinline__ void load_x_tile(float* xl, const float* __restrict__ x, int n, int oh0, int ow0, int c0, int IH, int IW, int C) {
  constexpr int IR = (TH - 1) * S + 3, IC = 15 * S + 3, LS = lds_stride<CS>(), V = CS / 4;
  for (int idx = threadIdx.x; idx < IR * IC * V; idx += 256) {
    const int pix = idx / V, v = idx - pix * V;
    const int r = pix / IC, c = pix - r * IC;
    const int h = oh0 * S - 1 + r, w_ = ow0 * S - 1 + c;
    const bool ok = h >= 0 && w_ >= 0 && h < IH && w_ < IW;
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (ok) val = *reinterpret_cast<const f32x4*>(x + (((long)n * IH + h) * IW + w_) * C + c0 + v * 4);
    *reinterpret_cast<f32x4*>(xl + pix * LS + v * 4) = val;
  }
}

// CS: channels of the slab; KC: input channels a 16-channel output slice reads (16 for Cg <= 16, else Cg); S: stride; TH: output rows
template <int CS, int KC, int S, int TH>
__global__ __launch_bounds__(256) void gconv_fwd_kernel(GcArgs p) {
  extern __shared__ __attribute__((aligned(16))) float gc_lds[];
  constexpr int NSUB = CS / 16, NGRP = 4 / NSUB, MT = TH / NGRP, IC = 15 * S + 3, LS = lds_stride<CS>();
  static_assert(TH % NGRP == 0, "rows split evenly over the waves");
  const int tile = blockIdx.x, n = blockIdx.z, c0 = blockIdx.y * CS;
  const int oh0 = (tile / p.tiles_w) * TH, ow0 = (tile % p.tiles_w) * 16;
  load_x_tile<CS, S, TH>(gc_lds, p.x, n, oh0, ow0, c0, p.IH, p.IW, p.C);
  __syncthreads();

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int sub = wv % NSUB, grp = wv / NSUB;
  const int i = lane & 15, kq = lane >> 4;
  const int co = c0 + sub * 16 + i;                  // A row of this lane
  const int kin0 = (KC == 16) ? sub * 16 : 0;        // first slab channel this slice reads
  // weights of (co, tap, 16-channel chunk kc): four consecutive channels 4 kq .. 4 kq + 3 of the chunk
  const bool diag = p.Cg == 8;                        // two groups in the tile: block-diagonal
  const bool wok = !diag || (kq >> 1) == (i >> 3);
  const float* wp = p.w + (long)co * 9 * p.Cg + (diag ? 4 * (kq & 1) : 4 * kq);
  const float* xb = gc_lds + (i * S) * LS + kin0 + 4 * kq;

  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int NK = KC / 16, STEPS = 9 * NK;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 a_next = wok ? *reinterpret_cast<const f32x4*>(wp) : zero4;
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int tap = st / NK, kc = st % NK, kh = tap / 3, kw = tap % 3;
    const f32x4 a = a_next;
    if (st + 1 < STEPS) {
      const int tap2 = (st + 1) / NK, kc2 = (st + 1) % NK;
      a_next = wok ? *reinterpret_cast<const f32x4*>(wp + tap2 * p.Cg + kc2 * 16) : zero4;
    }
    f32x4 b[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int r = grp + NGRP * m;
      b[m] = *reinterpret_cast<const f32x4*>(xb + ((r * S + kh) * IC + kw) * LS + kc * 16);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[m][j], acc[m], 0, 0, 0);
  }

  // D[row = 4 (lane >> 4) + e][col = lane & 15]: four consecutive output channels of pixel (lane & 15)
  const int cq = c0 + sub * 16 + 4 * kq;
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + cq);
  if (p.shift) sh = *reinterpret_cast<const f32x4*>(p.shift + cq);
  const int ow = ow0 + i;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int oh = oh0 + grp + NGRP * m;
    if (oh < p.OH && ow < p.OW) {
      const long o = (((long)n * p.OH + oh) * p.OW + ow) * p.C + cq;
      f32x4 v = acc[m] * sc + sh;
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __builtin_elementwise_maximum(v[e], 0.f);   // (keeps NaN, fmaxf would not)
      }
      if (p.mask) {
        const f32x4 mk = *reinterpret_cast<const f32x4*>(p.mask + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = mk[e] > 0.f ? v[e] : 0.f;
      }
      *reinterpret_cast<f32x4*>(p.y + o) = v;
    }
  }
}

// wt[g Cg + ci][2 - kh][2 - kw][col] = scale[g Cg + col] * w[g Cg + col][kh][kw][ci]
__global__ void gconv_flip_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ wt, int C, int Cg) {
  const long total = (long)C * 9 * Cg;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int col = (int)(idx % Cg);
    const int tap = (int)((idx / Cg) % 9);
    const int row = (int)(idx / (9 * Cg));
    const int g = row / Cg, ci = row - g * Cg, src = g * Cg + col;
    float v = w[((long)src * 9 + (8 - tap)) * Cg + ci];
    if (scale) v *= scale[src];
    wt[idx] = v;
  }
}

// Data gradient at stride 2, gather form by parity class.  dx pixel (2 a + ph, 2 b + pw) receives tap (kh, kw) of dy pixel
// (a + dr, b + dc) exactly when kh = ph + 1 (mod 2), dr = (ph + 1 - kh) / 2 (likewise kw, dc): 1, 2, 2 and 4 taps for the four classes,
// nine in all -- the useful work of the forward, no zero-interleaved copy of dy.  One block = TA x 16 dy pixels with one more row and
// column of halo = 2 TA x 32 dx pixels x one channel slab; an MFMA's 16 pixels are the 16 columns b of one class and one row a.
// p.x = dy [N][IH][IW][C], p.w = the transformed weights wt (gconv_flip_kernel: tap t sits at 8 - t), p.y = dx [N][OH][OW][C].
template <int CS, int KC>
__global__ __launch_bounds__(256) void gconv_dgrad_s2_kernel(GcArgs p) {
  extern __shared__ __attribute__((aligned(16))) float gc_lds[];
  constexpr int TA = 4, NSUB = CS / 16, NGRP = 4 / NSUB, MT = TA / NGRP, IC = 17, LS = lds_stride<CS>(), V = CS / 4, NK = KC / 16;
  const int tile = blockIdx.x, n = blockIdx.z, c0 = blockIdx.y * CS;
  const int a0 = (tile / p.tiles_w) * TA, b0 = (tile % p.tiles_w) * 16;
  for (int idx = threadIdx.x; idx < (TA + 1) * IC * V; idx += 256) {
    const int pix = idx / V, v = idx - pix * V;
    const int r = pix / IC, c = pix - r * IC;
    const int h = a0 + r, w_ = b0 + c;
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (h < p.IH && w_ < p.IW) val = *reinterpret_cast<const f32x4*>(p.x + (((long)n * p.IH + h) * p.IW + w_) * p.C + c0 + v * 4);
    *reinterpret_cast<f32x4*>(gc_lds + pix * LS + v * 4) = val;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int sub = wv % NSUB, grp = wv / NSUB;
  const int i = lane & 15, kq = lane >> 4;
  const int row = c0 + sub * 16 + i;                 // A row of this lane: a dx channel
  const int kin0 = (KC == 16) ? sub * 16 : 0;
  const bool diag = p.Cg == 8;
  const bool wok = !diag || (kq >> 1) == (i >> 3);
  const float* wp = p.w + (long)row * 9 * p.Cg + (diag ? 4 * (kq & 1) : 4 * kq);
  const float* xb = gc_lds + i * LS + kin0 + 4 * kq;
  const int cq = c0 + sub * 16 + 4 * kq;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const int ph = cls >> 1, pw = cls & 1;
    f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = zero4;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      if ((kh & 1) == ph) continue;
      const int dr = (ph + 1 - kh) / 2;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        if ((kw & 1) == pw) continue;
        const int dc = (pw + 1 - kw) / 2;
        const int tapw = 8 - (kh * 3 + kw);
#pragma unroll
        for (int kc = 0; kc < NK; ++kc) {
          const f32x4 a = wok ? *reinterpret_cast<const f32x4*>(wp + tapw * p.Cg + kc * 16) : zero4;
          f32x4 b[MT];
#pragma unroll
          for (int m = 0; m < MT; ++m) b[m] = *reinterpret_cast<const f32x4*>(xb + ((grp + NGRP * m + dr) * IC + dc) * LS + kc * 16);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[m][j], acc[m], 0, 0, 0);
        }
      }
    }
    const int ow = 2 * (b0 + i) + pw;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int oh = 2 * (a0 + grp + NGRP * m) + ph;
      if (oh < p.OH && ow < p.OW) {
        const long o = (((long)n * p.OH + oh) * p.OW + ow) * p.C + cq;
        f32x4 v = acc[m];
        if (p.mask) {
          const f32x4 mk = *reinterpret_cast<const f32x4*>(p.mask + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = mk[e] > 0.f ? v[e] : 0.f;
        }
        *reinterpret_cast<f32x4*>(p.y + o) = v;
      }
    }
  }
}

struct GwArgs {
  const float* x;         // [N][IH][IW][C]
  const float* dy;        // [N][OH][OW][C]
  const float* rowscale;  // [C] or null
  float* dw;              // [C][3][3][Cg], accumulated into
  int N, IH, IW, OH, OW, C, Cg;
  int tiles_w, tiles_img, tiles;  // spatial tiles per image row / per image / in all
};

template <int CS, int KC, int S, int TH>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(GwArgs p) {
  extern __shared__ __attribute__((aligned(16))) float gc_lds[];
  constexpr int IR = (TH - 1) * S + 3, IC = 15 * S + 3, LS = lds_stride<CS>(), V = CS / 4;
  constexpr int NCI = (KC == 64) ? 4 : 1;     // 16-channel input slices per wave
  constexpr int RS = (KC == 16) ? 2 : 1;      // waves that share a (co, ci) slice pair split the tile's rows
  float* xl = gc_lds;
  float* dl = gc_lds + IR * IC * LS;          // dy tile [TH][16][CS + 4]
  const int c0 = blockIdx.y * CS;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int co_sub = (KC == 64) ? wv : (wv & 1);
  const int ci_sub0 = (KC == 64) ? 0 : (KC == 32 ? (wv >> 1) : co_sub);
  const int r0 = (KC == 16) ? (wv >> 1) : 0;

  f32x4 acc[NCI][9];
#pragma unroll
  for (int c = 0; c < NCI; ++c)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[c][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int n = tile / p.tiles_img, tin = tile - n * p.tiles_img;
    const int oh0 = (tin / p.tiles_w) * TH, ow0 = (tin % p.tiles_w) * 16;
    __syncthreads();   // the previous tile's reads are done
    load_x_tile<CS, S, TH>(xl, p.x, n, oh0, ow0, c0, p.IH, p.IW, p.C);
    for (int idx = threadIdx.x; idx < TH * 16 * V; idx += 256) {
      const int pix = idx / V, v = idx - pix * V;
      const int oh = oh0 + pix / 16, ow = ow0 + (pix & 15);
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (oh < p.OH && ow < p.OW) val = *reinterpret_cast<const f32x4*>(p.dy + (((long)n * p.OH + oh) * p.OW + ow) * p.C + c0 + v * 4);
      *reinterpret_cast<f32x4*>(dl + pix * LS + v * 4) = val;
    }
    __syncthreads();
    // A[row = co][k = pixel] = dy, B[k = pixel][col = ci] = x at the tap's offset; K = the tile's pixels, four per MFMA
    for (int r = r0; r < TH; r += RS) {
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        const int pc = ch * 4 + kq;
        const float a = dl[(r * 16 + pc) * LS + co_sub * 16 + i];
        const float* xb = xl + ((r * S) * IC + pc * S) * LS + ci_sub0 * 16 + i;
#pragma unroll
        for (int c = 0; c < NCI; ++c)
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const float b = xb[((t / 3) * IC + (t % 3)) * LS + c * 16];
            acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[c][t], 0, 0, 0);
          }
      }
    }
  }

  // D[row = 4 (lane >> 4) + e -> co][col = lane & 15 -> ci]
  const bool diag = p.Cg == 8;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int col = 4 * kq + e;                       // output channel inside the 16-channel slice
    const int co = c0 + co_sub * 16 + col;
    const float rs = p.rowscale ? p.rowscale[co] : 1.f;
    if (diag && (col >> 3) != (i >> 3)) continue;     // the other group's block of a block-diagonal tile
#pragma unroll
    for (int c = 0; c < NCI; ++c) {
      const int cig = diag ? (i & 7) : ((KC == 16 ? 0 : (ci_sub0 + c) * 16) + i);
#pragma unroll
      for (int t = 0; t < 9; ++t) atomicAdd(p.dw + ((long)co * 9 + t) * p.Cg + cig, rs * acc[c][t][e]);
    }
  }
}

bool gconv_shape_ok(int N, int H, int W, int C, int Cg, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || N > 65535) return false;
  if (!(Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64)) return false;
  if (C <= 0 || C % Cg || C % 32 || C / 32 > 65535) return false;
  if (stride != 1 && stride != 2) return false;
  return true;
}

template <int CS, int S, int TH>
constexpr size_t fwd_lds() { return (size_t)((TH - 1) * S + 3) * (15 * S + 3) * lds_stride<CS>() * sizeof(float); }
template <int CS, int S, int TH>
constexpr size_t wg_lds() { return fwd_lds<CS, S, TH>() + (size_t)TH * 16 * lds_stride<CS>() * sizeof(float); }

template <int CS, int KC, int S, int TH>
int launch_fwd(GcArgs& a, hipStream_t st) {
  static_assert(fwd_lds<CS, S, TH>() <= 64 * 1024, "LDS tile");
  a.tiles_w = mmt_cdiv(a.OW, 16);
  a.tiles = a.tiles_w * mmt_cdiv(a.OH, TH);
  constexpr size_t lds = fwd_lds<CS, S, TH>();
  hipLaunchKernelGGL((gconv_fwd_kernel<CS, KC, S, TH>), dim3(a.tiles, a.C / CS, a.N), dim3(256), lds, st, a);
  MMT_LAUNCH_CHECK();
  return 0;
}

template <int CS, int KC>
int launch_dgrad_s2(GcArgs& a, hipStream_t st) {
  a.tiles_w = mmt_cdiv(a.IW, 16);
  a.tiles = a.tiles_w * mmt_cdiv(a.IH, 4);
  constexpr size_t lds = (size_t)5 * 17 * lds_stride<CS>() * sizeof(float);
  hipLaunchKernelGGL((gconv_dgrad_s2_kernel<CS, KC>), dim3(a.tiles, a.C / CS, a.N), dim3(256), lds, st, a);
  MMT_LAUNCH_CHECK();
  return 0;
}

int dispatch_fwd(GcArgs& a, int s, hipStream_t st) {
  if (a.Cg <= 16) return s == 1 ? launch_fwd<32, 16, 1, 8>(a, st) : launch_fwd<32, 16, 2, 4>(a, st);
  if (a.Cg == 32) return s == 1 ? launch_fwd<32, 32, 1, 8>(a, st) : launch_fwd<32, 32, 2, 4>(a, st);
  return s == 1 ? launch_fwd<64, 64, 1, 8>(a, st) : launch_fwd<64, 64, 2, 2>(a, st);
}

template <int CS, int KC, int S, int TH>
int launch_wgrad(GwArgs& a, hipStream_t st) {
  static_assert(wg_lds<CS, S, TH>() <= 64 * 1024, "LDS tiles");
  a.tiles_w = mmt_cdiv(a.OW, 16);
  a.tiles_img = a.tiles_w * mmt_cdiv(a.OH, TH);
  a.tiles = a.tiles_img * a.N;
  const int slabs = a.C / CS;
  int split = mmt_cdiv(768, slabs);   // ~3 blocks per CU in all: pixel ranges across blocks, summed by the atomics
  if (split > a.tiles) split = a.tiles;
  constexpr size_t lds = wg_lds<CS, S, TH>();
  hipLaunchKernelGGL((gconv_wgrad_kernel<CS, KC, S, TH>), dim3(split, slabs), dim3(256), lds, st, a);
  MMT_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int mmt_gconv3x3_forward(const float* x, const float* w, const float* scale, const float* shift, float* y, int N, int H, int W,
                                    int C, int Cg, int stride, int relu, void* stream) {
  if (!x || !w || !y || !gconv_shape_ok(N, H, W, C, Cg, stride)) return MMT_EINVAL;
  GcArgs a{};
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.mask = nullptr; a.y = y;
  a.N = N; a.IH = H; a.IW = W; a.OH = (H - 1) / stride + 1; a.OW = (W - 1) / stride + 1; a.C = C; a.Cg = Cg;
  a.relu = relu != 0;
  return dispatch_fwd(a, stride, (hipStream_t)stream);
}

extern "C" int mmt_gconv3x3_dgrad(const float* dy, const float* w, const float* scale, const float* mask, float* wt, float* dx, int N,
                                  int H, int W, int C, int Cg, int stride, void* stream) {
  if (!dy || !w || !wt || !dx || !gconv_shape_ok(N, H, W, C, Cg, stride)) return MMT_EINVAL;
  const long total = (long)C * 9 * Cg;
  int blocks = mmt_cdiv(total, 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(gconv_flip_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, scale, wt, C, Cg);
  MMT_LAUNCH_CHECK();
  GcArgs a{};
  a.x = dy; a.w = wt; a.scale = nullptr; a.shift = nullptr; a.mask = mask; a.y = dx;
  a.N = N; a.IH = (H - 1) / stride + 1; a.IW = (W - 1) / stride + 1; a.OH = H; a.OW = W; a.C = C; a.Cg = Cg;
  a.relu = 0;
  if (stride == 1) return dispatch_fwd(a, 1, (hipStream_t)stream);
  if (Cg <= 16) return launch_dgrad_s2<32, 16>(a, (hipStream_t)stream);
  if (Cg == 32) return launch_dgrad_s2<32, 32>(a, (hipStream_t)stream);
  return launch_dgrad_s2<64, 64>(a, (hipStream_t)stream);
}

extern "C" int mmt_gconv3x3_wgrad(const float* x, const float* dy, const float* rowscale, float* dw, int N, int H, int W, int C, int Cg,
                                  int stride, void* stream) {
  if (!x || !dy || !dw || !gconv_shape_ok(N, H, W, C, Cg, stride)) return MMT_EINVAL;
  GwArgs a{};
  a.x = x; a.dy = dy; a.rowscale = rowscale; a.dw = dw;
  a.N = N; a.IH = H; a.IW = W; a.OH = (H - 1) / stride + 1; a.OW = (W - 1) / stride + 1; a.C = C; a.Cg = Cg;
  hipStream_t st = (hipStream_t)stream;
  if (Cg <= 16) return stride == 1 ? launch_wgrad<32, 16, 1, 8>(a, st) : launch_wgrad<32, 16, 2, 4>(a, st);
  if (Cg == 32) return stride == 1 ? launch_wgrad<32, 32, 1, 8>(a, st) : launch_wgrad<32, 32, 2, 4>(a, st);
  return stride == 1 ? launch_wgrad<64, 64, 1, 4>(a, st) : launch_wgrad<64, 64, 2, 2>(a, st);
}
