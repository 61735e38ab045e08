// The ResNet stem as ONE kernel (round 5): conv 7x7 / stride 2 / pad 3 (3 -> 64) + FrozenBatchNorm + ReLU + max pool 3x3 / stride 2 /
// pad 1 -- reference modeling/backbone/resnet.py:288-293 `StemWithFixedBatchNorm.forward` with layers/batch_norm.py:19-24 folded
// in.  The stem is frozen (FREEZE_CONV_BODY_AT = 2): forward only.
//
// Before: a library copy built the 16-channel space-to-depth image, the tiled kernel ran the 4x4 / stride-1 convolution over it
// (429 us for the teacher's 8 x 1024^2 batch, 3.2 x its HBM time: K = 256 leaves 16 steps per tile to pay for a tile's prologue and
// epilogue), wrote 537 MB of ReLU output, and maxpool_kernel read them back (108 us).  The round trip of those 537 MB is the
// larger half of the cost, and nothing downstream wants the un-pooled tensor.  Here a block owns a tile of 7 x 15 POOLED pixels:
//   * the 16 x 32 convolution outputs under it (rows 2 py0 - 1 .., columns 2 px0 - 1 ..: every pooling window of the tile; one MFMA
//     row tile = one output row) need a 19 x 35 patch of space-to-depth pixels (16 channels = the 2 x 2 parity x RGB + 0).  The patch
//     is gathered ONCE from the NCHW image -- 8-byte loads, coalesced along W --, scaled by the power of two of the image's recorded
//     maximum, split into its two fp16 terms and written to LDS as the A-plane image of the convolution kernels (32 bytes per pixel
//     and plane, half ^= (pixel >> 3) & 1); the 16 taps (a, b) of the 4 x 4 filter read their fragments from it at pixel offset
//     35 a + b: no im2col traffic at all;
//   * the packed weight planes of all 16 steps (64 KB) are copied into LDS once; the main loop is 16 steps of 8 fragment reads + 12
//     MFMAs per wave (8 waves, 2 output rows x 64 channels each) with no barrier and no copy in it;
//   * epilogue: scale / shift / ReLU in registers; vertical maximum of a wave's two rows in registers, the third row (the next
//     wave's first) and the horizontal 3-maximum through LDS; 16-byte coalesced stores of the pooled tile; statistics of the output.
// Same products in the same order as the tiled kernel on the space-to-depth image and the same maximum: bit-identical to the
// three-launch path (tests/test_stem_gpu.py).  Arithmetic: two-term fp16 split, 3 products per multiply (mode 3 default).
//
// Roofline: HBM -- 12 B read per input pixel, 64 B written per output pixel (8 x 1024^2: 101 + 134 MB = 47 us at 5 TB/s); the matrix
// work (39.5 GFLOP x 3 products, 1.22 x redundant rows / columns of overlapping tiles) is 58 us at the dense fp16 peak.
#include "conv_shared.h"

namespace {

struct StemP {
  const float* x;                      // [N][3][H][W] fp32
  const unsigned short* wpl; long wpl_stride;   // packed fp16 planes of the space-to-depth filter [64][(a, b, 16 ch) = 256]
  const float* w;                      // the same filter in fp32 ([64][4][4][16]), for the exact path
  const float* scale; const float* shift;
  float* y;                            // [N][Hp][Wp][64] fp32
  const float* x_slot;                 // statistics slot of x: [0] = max |x| (the scale is derived from it), sums / counts for the guard
  const float* s_w;                    // scale of the weight planes
  unsigned* amax_out; int amax_stats;
  int N, H, W, Hc, Wc, Hp, Wp, tiles_y, tiles_x;
};

constexpr int SPH = 19, SPW = 35, SPIX = SPH * SPW;          // patch of space-to-depth pixels
constexpr int SPL = 672 * 32;                                 // bytes of one plane of the patch (665 pixels, padded)
constexpr int SB_OFF = 2 * SPL;                               // weight planes behind the two patch planes
constexpr int STEM_LDS = 128 * 1024;                          // loop: 2 x 21 KB + 64 KB; epilogue: 64 KB + 56 KB

__device__ __forceinline__ float stem_exact(const StemP& p, int n, int oy, int ox, int co) {
  // conv output (oy, ox, co) with fp32 FMAs straight from the image (the fp16 split's slow, exact path)
  float acc = 0.f;
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++) {
      const int si = oy - 2 + a, sj = ox - 2 + b;
      if ((unsigned)si >= (unsigned)p.Hc || (unsigned)sj >= (unsigned)p.Wc) continue;
      for (int ch = 0; ch < 16; ch++) {
        const int c = ch & 3;
        if (c == 3) continue;
        const float xv = p.x[(((long)n * 3 + c) * p.H + 2 * si + (ch >> 3)) * p.W + 2 * sj + ((ch >> 2) & 1)];
        acc = fmaf(xv, p.w[((co * 4 + a) * 4 + b) * 16 + ch], acc);
      }
    }
  return acc;
}

__global__ __launch_bounds__(512) void stem_fused_kernel(const StemP p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* const sm = (char*)lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = blockIdx.x;
  const int tx = bid % p.tiles_x; bid /= p.tiles_x;
  const int ty = bid % p.tiles_y;
  const int n = bid / p.tiles_y;
  const int py0 = ty * 7, px0 = tx * 15;
  const int oy0 = 2 * py0 - 1, ox0 = 2 * px0 - 1;              // first convolution output of the tile
  const int sy0 = oy0 - 2, sx0 = ox0 - 2;                      // first space-to-depth pixel of the patch
  const F16Guard guard = f16_guard_load(p.x_slot);
  const float sx = f16_scale_of(*p.x_slot);

  if (f16_guard_bad(guard)) {   // an image whose dynamic range defeats fp16 (uniform over the grid): exact products, element by element
    float amx = 0.f;
    for (int o = tid; o < 7 * 15 * 64; o += 512) {
      const int co = o & 63, q = (o >> 6) % 15, j = (o >> 6) / 15;
      const int py = py0 + j, px = px0 + q;
      if (py >= p.Hp || px >= p.Wp) continue;
      float m = 0.f;
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          const int oy = 2 * py + dy, ox = 2 * px + dx;
          if ((unsigned)oy >= (unsigned)p.Hc || (unsigned)ox >= (unsigned)p.Wc) continue;
          m = fmaxf(m, fmaxf(stem_exact(p, n, oy, ox, co) * p.scale[co] + p.shift[co], 0.f));
        }
      p.y[(((long)n * p.Hp + py) * p.Wp + px) * 64 + co] = m;
      amx = fmaxf(amx, m);
    }
    if (p.amax_out && amx > 0.f) atomicMax(p.amax_out, __builtin_bit_cast(unsigned, amx));
    return;
  }

  // ---- the weight planes of all 16 steps: 64 copies of 1 KiB, eight per wave.  LDS image: [plane][step][32-channel block][1 KiB]
  {
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)p.wpl, 0, 0x7ffffff0, 0x00020000);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int item = wave + 8 * i, q = item >> 5, rest = item & 31;   // rest = step * 2 + block: the planes' own order
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b, (lds_ptr_t)(sm + SB_OFF + item * 1024), 16,
                                               (int)((q * p.wpl_stride + (long)rest * 512 + lane * 8) * 2), 0, 0, 0);
    }
  }
  // ---- the patch: item = (pixel, row parity bh): three 8-byte loads (c = 0, 1, 2 at columns 2 sj, 2 sj + 1), one 16-byte LDS store
  // per plane.  16 channels of a pixel = (bh, bw, c) with c = 3 zero: the order of StemWithFixedBatchNorm._s2d_weight
  typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int rnd = 0; rnd < 3; rnd++) {
    const int item = tid + 512 * rnd;
    if (item < 2 * SPIX) {
      const int pix = item >> 1, bh = item & 1;
      const int pr = pix / SPW, pc = pix - pr * SPW;
      const int si = sy0 + pr, sj = sx0 + pc;
      f32x2 v[3];
      const bool ok = (unsigned)si < (unsigned)p.Hc && (unsigned)sj < (unsigned)p.Wc;
#pragma unroll
      for (int c = 0; c < 3; c++)
        v[c] = ok ? *(const f32x2*)(p.x + (((long)n * 3 + c) * p.H + 2 * si + bh) * p.W + 2 * sj) : f32x2{0.f, 0.f};
      uint2 o0[2], o1[2];
      split4h(f32x4{v[0][0], v[1][0], v[2][0], 0.f}, sx, o0);     // bw = 0: c0 c1 c2 0
      split4h(f32x4{v[0][1], v[1][1], v[2][1], 0.f}, sx, o1);     // bw = 1
      char* const dst = sm + pix * 32 + ((bh ^ (pix >> 3)) & 1) * 16;
      *(uint4*)dst = uint4{o0[0].x, o0[0].y, o1[0].x, o1[0].y};
      *(uint4*)(dst + SPL) = uint4{o0[1].x, o0[1].y, o1[1].x, o1[1].y};
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- main loop: wave w owns output rows 2 w, 2 w + 1 of the tile (a = 0, 1) x 64 channels (b = 0, 1)
  const int lr = lane & 31, kh2 = lane >> 5;
  const int boff = SB_OFF + lr * 32 + (((kh2 ^ (lr >> 3)) & 1) << 4);
  auto a_addr = [&](int a, int ta, int tb) {
    const int pidx = (2 * wave + a + ta) * SPW + lr + tb;
    return pidx * 32 + (((kh2 ^ (pidx >> 3)) & 1) << 4);
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
  auto fread = [&](int s, f16x8 (&fa)[2][2], f16x8 (&fb)[2][2]) {
    const int ta = s >> 2, tb = s & 3;
#pragma unroll
    for (int a = 0; a < 2; a++) {
      const int ad = a_addr(a, ta, tb);
      fa[0][a] = *(const f16x8*)(sm + ad);
      fa[1][a] = *(const f16x8*)(sm + ad + SPL);
    }
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int b = 0; b < 2; b++) fb[q][b] = *(const f16x8*)(sm + boff + ((q * 16 + s) * 2 + b) * 1024);
  };
  auto mma = [&](const f16x8 (&fa)[2][2], const f16x8 (&fb)[2][2]) {   // products (h, l), (l, h), (h, h): the tiled kernel's order
#pragma unroll
    for (int pr = 0; pr < 3; pr++) {
      const int qa = pr == 1 ? 1 : 0, qb = pr == 0 ? 1 : 0;
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[qa][a], fb[qb][b], acc[a][b], 0, 0, 0);
    }
  };
  {
    f16x8 faP[2][2], fbP[2][2], faQ[2][2], fbQ[2][2];
    fread(0, faP, fbP);
#pragma unroll
    for (int s = 0; s < 16; s += 2) {
      fread(s + 1, faQ, fbQ);
      mma(faP, fbP);
      if (s + 2 < 16) fread(s + 2, faP, fbP);
      mma(faQ, fbQ);
    }
  }
  __syncthreads();   // everybody is done with the patch and the weights: LDS becomes the pooling stage

  // ---- epilogue.  acc[a][b][r]: output row 2 w + a, column 8 (r / 4) + r % 4 + 4 (lane / 32), channel 32 b + lane % 32
  const int col_l = lane & 31, rq = lane >> 5;
  const float inv = 1.f / (sx * *p.s_w);
  float sc[2], sh[2];
#pragma unroll
  for (int b = 0; b < 2; b++) { sc[b] = p.scale[b * 32 + col_l] * inv; sh[b] = p.shift[b * 32 + col_l]; }
  f32x16 m01[2];
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int ox = ox0 + 8 * (r >> 2) + (r & 3) + 4 * rq;
      const bool cok = (unsigned)ox < (unsigned)p.Wc;
      float v[2];
#pragma unroll
      for (int a = 0; a < 2; a++) {
        const int oy = oy0 + 2 * wave + a;
        const float t = fmaxf(acc[a][b][r] * sc[b] + sh[b], 0.f);
        v[a] = (cok && (unsigned)oy < (unsigned)p.Hc) ? t : 0.f;   // outside the image: no candidate (every window holds a value >= 0)
      }
      acc[0][b][r] = v[0];
      m01[b][r] = fmaxf(v[0], v[1]);
    }
  float* const xr = lds;                 // [wave][32 columns][64 channels]: a wave's FIRST row, for the wave above it
  float* const hv = lds + 8 * 32 * 64;   // [7 pooled rows][32 columns][64 channels]: vertical maxima
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int r = 0; r < 16; r++)
      xr[(wave * 32 + 8 * (r >> 2) + (r & 3) + 4 * rq) * 64 + b * 32 + col_l] = acc[0][b][r];
  __syncthreads();
  if (wave < 7) {
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int col = 8 * (r >> 2) + (r & 3) + 4 * rq;
        hv[(wave * 32 + col) * 64 + b * 32 + col_l] = fmaxf(m01[b][r], xr[((wave + 1) * 32 + col) * 64 + b * 32 + col_l]);
      }
  }
  __syncthreads();
  float amx = 0.f, asum = 0.f, acnt = 0.f;
  for (int o = tid; o < 7 * 15 * 16; o += 512) {
    const int c4 = o & 15, q = (o >> 4) % 15, j = (o >> 4) / 15;
    const int py = py0 + j, px = px0 + q;
    if (py >= p.Hp || px >= p.Wp) continue;
    const f32x4* const row = (const f32x4*)(hv + (j * 32 + 2 * q) * 64) + c4;
    const f32x4 t0 = row[0], t1 = row[16], t2 = row[32];
    f32x4 m;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      m[e] = fmaxf(fmaxf(t0[e], t1[e]), t2[e]);
      amx = fmaxf(amx, m[e]);
      asum += m[e];
    }
    acnt += 4.f;
    *(f32x4*)(p.y + (((long)n * p.Hp + py) * p.Wp + px) * 64 + c4 * 4) = m;
  }
  if (p.amax_out) {
    __syncthreads();
    float* const red = lds;
    const bool stats = p.amax_stats && (blockIdx.x & 63) == 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amx = fmaxf(amx, __shfl_xor(amx, o, 64));
    if (stats) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { asum += __shfl_xor(asum, o, 64); acnt += __shfl_xor(acnt, o, 64); }
    }
    if (lane == 0) { red[wave] = amx; red[16 + wave] = asum; red[32 + wave] = acnt; }
    __syncthreads();
    if (tid == 0) {
      float m = red[0], sm_ = red[16], cn = red[32];
      for (int i = 1; i < 8; i++) { m = fmaxf(m, red[i]); sm_ += red[16 + i]; cn += red[32 + i]; }
      const unsigned bits = __builtin_bit_cast(unsigned, m);
      if (m > 0.f && bits > __hip_atomic_load(p.amax_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p.amax_out, bits);
      if (stats && cn > 0.f) {
        const int k = (blockIdx.x >> 6) & 15;
        atomicAdd((float*)p.amax_out + 1 + k, sm_);
        atomicAdd((float*)p.amax_out + 17 + k, cn);
      }
    }
  }
}


// ------------------------------------------------------------------------------------ 3x3, 64 -> 64 channels (layer1's conv2)
// The 3x3 convolutions of layer1 (backbone/resnet.py:254-274 with 64 bottleneck channels, frozen: forward only, the teacher's
// 8 x 256^2 and the student's 4 x 256^2 maps) ran on the tiled kernel's 128 x 64 tile at 3.5 x their HBM time (188 us for 268 MB):
// K = 576 is 36 steps, each re-fetching its rows' pixels through the L2 -> LDS path nine times over, behind a per-tile prologue.
// Same recipe as the stem: a block owns 8 x 16 output pixels, gathers their 10 x 18 input patch ONCE (fp32, 16-byte loads,
// coalesced), scales and splits it into the two fp16 terms on the way into LDS ([16-channel slab][pixel][32 B] per plane), and the
// nine taps read their fragments from the patch at pixel offset 18 kh + kw.  The weight planes stream through two 16 KB buffers,
// one tap (four steps) ahead.  4 waves (2 output rows x 16 columns x 64 channels each), 80 KB of LDS: two blocks per CU.
// Same products, same order as the tiled kernel: bit-identical (tests/test_stem_gpu.py).
//
// FUSE: conv3 (1x1, 64 -> 256 channels + FrozenBN + residual + ReLU) of the same bottleneck behind it, in the same launch.  A frozen
// layer1 saves nothing for a backward pass, and o2 = the 3x3's output is read by conv3 alone: its round trip through HBM (34 MB per
// image and block) and one launch per block go.  A 1x1 convolution is per pixel, so the tile needs no halo: every wave keeps its own
// 32 pixels.  After the tap loop the wave's o2 (FrozenBN + ReLU in registers, exactly the values the un-fused launch stores) is
// split into its two fp16 terms and transposed through the wave's 8 KB of the patch region (dead by then) into conv3's A fragments
// (four k16 steps, kept in registers for all of Cout); W3's packed planes stream through the weight ring in four panels of 64
// channels (16 KB each, one panel ahead); each panel's epilogue is the row-resident 1x1 kernel's (affine, residual, ReLU, fp32 store,
// statistics), its residual values requested one panel ahead (panel 0's behind the last tap).  Same k order and product order as
// conv1x1_rows_kernel: with the same scale of o2 the result is bit-identical to the two launches (tests/test_layer1_fused_gpu.py).
// Measured: the launch takes about the sum of its two phases minus o2's round trip -- inside a block the matrix
// phase (nine taps, each behind a full drain of the memory queue) and the memory phase (four panels) do not overlap; what overlap
// there is comes from the other block resident on the CU.
// FUSE == 2: conv1 of the NEXT bottleneck (1x1, 256 -> 64) behind that, still in the same launch: inside layer1 `out` is read again at
// once by the next block's conv1, and the launch holds it in 64-channel panels for its own pixels.  Each finished panel (the values
// just stored) is split with the scale of `out` as an operand, transposed through the wave's same 8 KB -- conv3's fragments sit in
// registers by then -- and multiplied as K steps 4 pn .. 4 pn + 3 into a second 32 x 64 accumulator per wave; W1's 16 KB chunk of
// the panel is copied into the 16 KB of the patch region the tail leaves free, behind one more barrier per panel.  One set of
// residual registers instead of two pays for the accumulator (requested when the set is consumed; the waits are counted in the
// panel code): 224 registers.  The epilogue stores o1_next and records its statistics -- the next launch's x_slot; the next block
// starts at its 3x3.  Same k order and product order as conv1x1_rows_kernel<16>: bit-identical to the three launches at their
// scales.  The range test of `out` is per WAVE (its 32 pixels x 256 channels, known after the last panel): a wave that fails
// computes its o1_next with fp32 FMAs from the `out` it stored.
// The scale of o2 cannot be its own maximum -- that is known when the launch is over.  It is the producing site's lagged scale
// (round 6: the largest |o2| of the previous step with 2 x head-room, folded by mmt_rb_scales_update from the pending maximum this
// launch records), and the range test is made per TILE on the tile's own o2: a tile that leaves the fp16 range at that scale (or
// whose mean falls below the low term's range) computes its 1x1 products with fp32 FMAs -- the exact path of the other kernels,
// decided per tile.
struct C64Tail {
  const unsigned short* w3pl; long w3pl_stride;   // packed fp16 planes of conv3's weight: [4 steps][8 blocks of 32 channels][32][16]
  const float* w3;                                // the same weight in fp32 ([256][64]): exact path
  const float* scale; const float* shift;         // conv3's folded FrozenBN
  const float* res;                               // residual [M][256]
  float* out;                                     // [M][256]
  const float* s_w3;                              // scale of the w3 planes
  const float* s_o2; int s_o2_amax;               // the scale of o2 (s_o2_amax: *s_o2 is a maximum of |o2| to derive it from; no range test)
  unsigned* o2_amax_next;                         // pending maximum of the producing site of o2, or null
  unsigned* amax_out;                             // statistics slot of out (max, sampled sums and counts), or null
  unsigned* out_amax_next;                        // pending maximum of the site of `out` as the next conv1's operand, or null
  // FUSE == 2: conv1 of the NEXT block (1x1, 256 -> 64, FrozenBN, ReLU) behind conv3 -- every finished 64-channel panel of `out` is one
  // K chunk of it.  W1's packed planes [16 steps][2 blocks of 32 channels][32][16], its fp32 form [64][256] (exact path), affine,
  // s_out: the scale of `out` as an operand (lagged like s_o2, or a maximum under s_o2_amax), o1n [M][64], its statistics slot
  const unsigned short* w1pl; long w1pl_stride; const float* w1; const float* scale1; const float* shift1; const float* s_w1;
  const float* s_out; float* o1n; unsigned* amax_o1n;
};
constexpr int C64_PW = 18, C64_PIX = 180, C64_SLAB = 192 * 32, C64_PL = 4 * C64_SLAB, C64_BOFF = 2 * C64_PL;
constexpr int C64_RED = 32768;   // FUSE: behind the four waves' transposes, floats for block-wide reductions
constexpr int C64_W1B = 32768;   // FUSE == 2: the 16 KB the tail leaves free in the patch region hold W1's chunk of the current panel

__device__ __forceinline__ void c64_dma16(const void* g, void* l) {   // 16 bytes per lane into LDS, hidden from the compiler's wait counts
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(__attribute__((address_space(3))) char*)l);
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(la) : "m0", "memory");
#endif
}

// FUSE, exact path: out for the block's 128 pixels from o2 in fp32 ([wave][32 pixels][64 channels] at the start of LDS), fp32 FMAs in
// ascending k like conv_slow_tile; lane = channel (4 x 64), the wave's 32 pixels in turn
__device__ __forceinline__ void c64_tail_exact(const ConvP& p, const C64Tail& t, const float* lds, const int img, const int oy0, const int ox0,
                                               const int wave, const int lane, float& amx, float& asum, float& acnt) {
  const float* const o2 = lds + wave * 2048;
  for (int j = 0; j < 4; j++) {
    const int c = lane + 64 * j;
    const float* const wr = t.w3 + c * 64;
    const float sc = t.scale ? t.scale[c] : 1.f, sh = t.shift ? t.shift[c] : 0.f;
    for (int i = 0; i < 32; i++) {
      const int oy = oy0 + 2 * wave + (i >> 4), ox = ox0 + (i & 15);
      if (oy >= p.Ho || ox >= p.Wo) continue;
      float acc = 0.f;
      for (int k = 0; k < 64; k++) acc = fmaf(o2[i * 64 + k], wr[k], acc);
      const long o = ((long)(img * p.Ho + oy) * p.Wo + ox) * 256 + c;
      float v = acc * sc + sh;
      if (t.res) v += t.res[o];
      v = max_nan(v, 0.f);
      t.out[o] = v;
      amx = max_nan(amx, v); asum += v; acnt += 1.f;
    }
  }
}

// FUSE, the input's own range guard failed (uniform over the grid): the wave's o2 with exact fp32 products in conv_slow_tile's order,
// into the same place; lane = channel.  -> the lane's largest o2
__device__ __forceinline__ float c64_o2_exact(const ConvP& p, float* lds, const int img, const int oy0, const int ox0, const int wave,
                                              const int lane) {
  float* const o2 = lds + wave * 2048;
  const float sc = p.scale ? p.scale[lane] : 1.f, sh = p.shift ? p.shift[lane] : 0.f;
  float amx = 0.f;
  for (int i = 0; i < 32; i++) {
    const int oy = oy0 + 2 * wave + (i >> 4), ox = ox0 + (i & 15);
    float v = 0.f;
    if (oy < p.Ho && ox < p.Wo) {
      float acc = 0.f;
      for (int kh = 0; kh < 3; kh++) {
        const int ih = oy - 1 + kh;
        if ((unsigned)ih >= (unsigned)p.H) continue;
        for (int kw = 0; kw < 3; kw++) {
          const int iw = ox - 1 + kw;
          if ((unsigned)iw >= (unsigned)p.W) continue;
          const float* xr = p.x + ((long)(img * p.H + ih) * p.W + iw) * 64;
          const float* wr = p.w + ((lane * 3 + kh) * 3 + kw) * 64;
          for (int ci = 0; ci < 64; ci++) acc = fmaf(xr[ci], wr[ci], acc);
        }
      }
      v = acc * sc + sh;
      if (p.relu) v = max_nan(v, 0.f);
      amx = max_nan(amx, fabsf(v));
    }
    o2[i * 64 + lane] = v;
  }
  return amx;
}

// statistics of what a block stored: the maximum (conditional atomic), sums and counts from every 64th block; `red`: 48 free floats
__device__ __forceinline__ void c64_commit(unsigned* const slot, const bool stats_on, float amx, float asum, float acnt, float* const red,
                                           const int wave, const int lane, const int tid, unsigned* const next = nullptr) {
  const bool stats = stats_on && (blockIdx.x & 63) == 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amx = max_nan(amx, __shfl_xor(amx, o, 64));
  if (stats) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { asum += __shfl_xor(asum, o, 64); acnt += __shfl_xor(acnt, o, 64); }
  }
  if (lane == 0) { red[wave] = amx; red[16 + wave] = asum; red[32 + wave] = acnt; }
  __syncthreads();
  if (tid == 0) {
    float m = red[0], sm_ = red[16], cn = red[32];
    for (int i = 1; i < 4; i++) { m = max_nan(m, red[i]); sm_ += red[16 + i]; cn += red[32 + i]; }
    const unsigned bits = __builtin_bit_cast(unsigned, m);
    if (bits > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, bits);
    if (next && bits > __hip_atomic_load(next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(next, bits);
    if (stats && cn > 0.f) {
      const int k = (blockIdx.x >> 6) & 15;
      atomicAdd((float*)slot + 1 + k, sm_);
      atomicAdd((float*)slot + 17 + k, cn);
    }
  }
}

// FUSE == 2, exact path of the next conv1 for one wave's 32 pixels: from `out` as this wave just stored it (its own stores, waited
// for), fp32 FMAs in ascending k; lane = channel
__device__ __forceinline__ void c64_next_exact(const ConvP& p, const C64Tail& t, const int img, const int oy0, const int ox0, const int wave,
                                               const int lane, float& amx, float& asum, float& acnt) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const float* const wr = t.w1 + lane * 256;
  const float sc = t.scale1 ? t.scale1[lane] : 1.f, sh = t.shift1 ? t.shift1[lane] : 0.f;
  for (int i = 0; i < 32; i++) {
    const int oy = oy0 + 2 * wave + (i >> 4), ox = ox0 + (i & 15);
    if (oy >= p.Ho || ox >= p.Wo) continue;
    const long m = (long)(img * p.Ho + oy) * p.Wo + ox;
    const float* const xr = t.out + m * 256;
    float acc = 0.f;
    for (int k = 0; k < 256; k++) acc = fmaf(__hip_atomic_load(xr + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), wr[k], acc);   // (past this CU's L1)
    const float v = max_nan(acc * sc + sh, 0.f);
    t.o1n[m * 64 + lane] = v;
    amx = max_nan(amx, v); asum += v; acnt += 1.f;
  }
}

template <int FUSE>
__global__ __launch_bounds__(256, 2) void conv3x3_c64_kernel(const ConvP p, const C64Tail t) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* const sm = (char*)lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_x = (p.Wo + 15) >> 4, tiles_y = (p.Ho + 7) >> 3;
  int bid = blockIdx.x;
  const int tx = bid % tiles_x; bid /= tiles_x;
  const int ty = bid % tiles_y;
  const int img = bid / tiles_y;
  const int oy0 = ty * 8, ox0 = tx * 16;
  const F16Guard guard = f16_guard_load(p.guard_x);
  const float sx = f16_scale_of(*p.f16_sx);
  if (f16_guard_bad(guard)) {   // (uniform over the grid) exact fp32 products; pixels of a ragged tile that wrap are written twice
    if constexpr (FUSE) {       // both convolutions exact, o2 through LDS
      float m = c64_o2_exact(p, lds, img, oy0, ox0, wave, lane);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = max_nan(m, __shfl_xor(m, o, 64));
      if (t.o2_amax_next && lane == 0 && __builtin_bit_cast(unsigned, m) != 0u) atomicMax(t.o2_amax_next, __builtin_bit_cast(unsigned, m));
      __syncthreads();
      float amx = 0.f, asum = 0.f, acnt = 0.f;
      c64_tail_exact(p, t, lds, img, oy0, ox0, wave, lane, amx, asum, acnt);
      float nmx = 0.f, nsum = 0.f, ncnt = 0.f;
      if constexpr (FUSE == 2) c64_next_exact(p, t, img, oy0, ox0, wave, lane, nmx, nsum, ncnt);
      if (t.amax_out) {
        __syncthreads();
        c64_commit(t.amax_out, true, amx, asum, acnt, lds + C64_RED / 4, wave, lane, tid, t.out_amax_next);
      }
      if (FUSE == 2 && t.amax_o1n) c64_commit(t.amax_o1n, true, nmx, nsum, ncnt, lds + C64_RED / 4 + 64, wave, lane, tid);
    } else {
      conv_slow_tile((img * p.Ho + oy0) * p.Wo + ox0, 16, p.Wo, 128, 0, 64, nullptr, false, tid, 256, blockIdx.x);
    }
    return;
  }
  const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)p.wpl, 0, 0x7ffffff0, 0x00020000);
  auto copy_chunk = [&](int t, int buf) {   // the weight planes of tap t: 4 steps x 2 planes x 2 blocks of 1 KiB, four per wave
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int item = wave * 4 + i, st = item >> 2, q = (item >> 1) & 1, blk = item & 1;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b, (lds_ptr_t)(sm + C64_BOFF + buf * 16384 + ((st * 2 + q) * 2 + blk) * 1024), 16,
                                               (int)((q * p.wpl_stride + (long)((t * 4 + st) * 2 + blk) * 512 + lane * 8) * 2), 0, 0, 0);
    }
  };
  copy_chunk(0, 0);
  // ---- the patch: item = (pixel, 4-channel quad): one 16-byte load, two 8-byte LDS stores (h, l)
  {
    f32x4 v[12];
#pragma unroll
    for (int rnd = 0; rnd < 12; rnd++) {
      const int item = tid + 256 * rnd;
      const int pix = item >> 4, cq = item & 15;
      const int pr = pix / C64_PW, pc = pix - pr * C64_PW;
      const int iy = oy0 - 1 + pr, ix = ox0 - 1 + pc;
      const bool ok = pix < C64_PIX && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      v[rnd] = ok ? ldg4(p.x + (((long)img * p.H + iy) * p.W + ix) * 64 + cq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int rnd = 0; rnd < 12; rnd++) {
      const int item = tid + 256 * rnd;
      const int pix = item >> 4, cq = item & 15;
      if (pix < C64_PIX) {
        uint2 o[2];
        split4h(v[rnd], sx, o);
        char* const dst = sm + (cq >> 2) * C64_SLAB + pix * 32 + (((((cq & 3) >> 1) ^ (pix >> 3)) & 1) << 4) + (cq & 1) * 8;
        *(uint2*)dst = o[0];
        *(uint2*)(dst + C64_PL) = o[1];
      }
    }
  }
  // ---- main loop.  Wave w: output rows 2 w, 2 w + 1 of the tile; MFMA row i = (i / 16, i % 16); 2 column tiles of 32 channels
  const int lr = lane & 31, kh2 = lane >> 5;
  const int prow = 2 * wave + (lr >> 4), pcol = lr & 15;
  const int boff = C64_BOFF + lr * 32 + (((kh2 ^ (lr >> 3)) & 1) << 4);
  f32x16 acc[2];
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[b][r] = 0.f;
#pragma unroll 1
  for (int t = 0; t < 9; t++) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // tap t's planes (and, first time, the patch) are in LDS
    __syncthreads();
    if (t + 1 < 9) copy_chunk(t + 1, (t + 1) & 1);                // into the buffer everybody finished reading before this barrier
    const int kh = t / 3, kw = t - kh * 3;
    const int pidx = (prow + kh) * C64_PW + pcol + kw;
    const char* const pa = sm + pidx * 32 + (((kh2 ^ (pidx >> 3)) & 1) << 4);
    const char* const pb = sm + boff + (t & 1) * 16384;
#pragma unroll
    for (int st = 0; st < 4; st++) {
      f16x8 fa[2], fb[2][2];
      fa[0] = *(const f16x8*)(pa + st * C64_SLAB);
      fa[1] = *(const f16x8*)(pa + st * C64_SLAB + C64_PL);
#pragma unroll
      for (int q = 0; q < 2; q++)
#pragma unroll
        for (int b = 0; b < 2; b++) fb[q][b] = *(const f16x8*)(pb + ((st * 2 + q) * 2 + b) * 1024);
#pragma unroll
      for (int pr = 0; pr < 3; pr++) {   // products (h, l), (l, h), (h, h): the tiled kernel's order
        const int qa = pr == 1 ? 1 : 0, qb = pr == 0 ? 1 : 0;
#pragma unroll
        for (int b = 0; b < 2; b++) acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[qa], fb[qb][b], acc[b], 0, 0, 0);
      }
    }
  }
  if constexpr (FUSE) {
    // ---- o2 in registers (the un-fused epilogue's expressions), the tile's statistics, then conv3 on the wave's own 32 pixels
    const int col_l = lane & 31, rq = lane >> 5;
    const float inv2 = 1.f / (sx * *p.f16_sw);
    float o2v[2][16];
    unsigned po[16];   // byte offset of (pixel of accumulator register r, channel lane % 32) in out / res; outside the image: beyond every
                       // bound.  The panel's and the block's channel offset ride in the instructions' scalar offset: one register per row
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int i = 8 * (r >> 2) + (r & 3) + 4 * rq;
      const int oy = oy0 + 2 * wave + (i >> 4), ox = ox0 + (i & 15);
      po[r] = (oy < p.Ho && ox < p.Wo) ? (unsigned)((img * p.Ho + oy) * p.Wo + ox) * 1024u + (unsigned)col_l * 4u : 0x80000000u;
    }
    float m2 = 0.f, s2 = 0.f, c2 = 0.f;
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const float sc = (p.scale ? p.scale[b * 32 + col_l] : 1.f) * inv2, sh = p.shift ? p.shift[b * 32 + col_l] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float v = acc[b][r] * sc + sh;
        if (p.relu) v = max_nan(v, 0.f);
        o2v[b][r] = v;
        const float av = po[r] != 0x80000000u ? fabsf(v) : 0.f;
        m2 = max_nan(m2, av);
        s2 += av;
        c2 += av > 0.f ? 1.f : 0.f;
      }
    }
    float sc3[4][2], sh3[4][2];   // conv3's affine for this lane's channels of the four panels: every vector load of the tail that is
#pragma unroll                    // not counted below is issued here
    for (int pn = 0; pn < 4; pn++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
        sc3[pn][b] = t.scale ? t.scale[pn * 64 + b * 32 + col_l] : 1.f;
        sh3[pn][b] = t.shift ? t.shift[pn * 64 + b * 32 + col_l] : 0.f;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      m2 = max_nan(m2, __shfl_xor(m2, o, 64));
      s2 += __shfl_xor(s2, o, 64);
      c2 += __shfl_xor(c2, o, 64);
    }
    // (the patch is still being read by waves inside the last tap: the 384 bytes behind the 180 pixels of its last slab are not)
    float* const red0 = (float*)(sm + C64_BOFF - 384);
    if (lane == 0) { red0[wave] = m2; red0[4 + wave] = s2; red0[8 + wave] = c2; }
    const int obytes = (int)((long)p.M * 1024);
    const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc((void*)t.res, 0, obytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((void*)t.out, 0, obytes, 0x00020000);
    float ur[2][2][16];
    auto request = [&](auto pnc) {   // the residual values of panel pn, into register set pn % 2 (FUSE == 2: the one set)
      constexpr int pn = decltype(pnc)::value;
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 16; r++)
          ur[FUSE == 2 ? 0 : (pn & 1)][b][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rres, (int)po[r], (pn * 64 + b * 32) * 4, 0));
    };
    auto copy_w3 = [&](int pn) {     // W3's planes of panel pn (channels 64 pn ..): 4 steps x 2 planes x 2 blocks of 1 KiB, four per wave
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int item = wave * 4 + i, st = item >> 2, q = (item >> 1) & 1, blk = item & 1;
        c64_dma16(t.w3pl + q * t.w3pl_stride + (long)(st * 8 + pn * 2 + blk) * 512 + lane * 8,
                  sm + C64_BOFF + ((pn + 1) & 1) * 16384 + ((st * 2 + q) * 2 + blk) * 1024);
      }
    };
    asm volatile("" ::: "memory");
    request(std::integral_constant<int, 0>{});
    asm volatile("" ::: "memory");
    copy_w3(0);   // into the buffer of tap 7: everybody left it before the barrier of tap 8
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the patch and tap 8's planes are dead from here on
    const float tmax = max_nan(max_nan(red0[0], red0[1]), max_nan(red0[2], red0[3]));
    const float ttot = (red0[4] + red0[5]) + (red0[6] + red0[7]), tcnt = (red0[8] + red0[9]) + (red0[10] + red0[11]);
    const float s_o2 = t.s_o2_amax ? f16_scale_of(*t.s_o2) : *t.s_o2;
    if (tid == 0 && t.o2_amax_next &&
        __builtin_bit_cast(unsigned, tmax) > __hip_atomic_load(t.o2_amax_next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(t.o2_amax_next, __builtin_bit_cast(unsigned, tmax));
    // the tile's own range test at the scale it was given (f16_guard_bad_lag's, on the tile's non-zero values): uniform over the block
    const bool exact = !t.s_o2_amax && (!(tmax <= 3.0e38f) || !(s_o2 > 0.f) || tmax * s_o2 > 60000.f || (ttot > 0.f && tcnt > ttot * s_o2 * 32.f));
    float amx = 0.f, asum = 0.f, acnt = 0.f;
    float nmx = 0.f, nsum = 0.f, ncnt = 0.f;   // FUSE == 2: statistics of o1_next
    constexpr bool NEXT = FUSE == 2;
    if (exact) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the copy in flight lands in a buffer nobody reads)
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) lds[wave * 2048 + (8 * (r >> 2) + (r & 3) + 4 * rq) * 64 + b * 32 + col_l] = o2v[b][r];
      __syncthreads();
      c64_tail_exact(p, t, lds, img, oy0, ox0, wave, lane, amx, asum, acnt);
      if constexpr (NEXT) c64_next_exact(p, t, img, oy0, ox0, wave, lane, nmx, nsum, ncnt);
    } else {
      // the wave's o2 as A fragments: [plane][k16 step][pixel][32 B], half ^= (pixel >> 3) & 1.  After the 4 x 4 transpose inside a quad
      // of lanes, lane k holds the quad's four channels of pixel 8 j + k + 4 (lane / 32): 8 bytes per plane
      char* const tw = sm + wave * 8192;
      auto to_frags = [&](const auto& v, const float s) {   // v[b][r]: the wave's 32 pixels x 64 channels in the accumulator layout
#pragma unroll
        for (int b = 0; b < 2; b++) {
          const int cq = (b * 32 + col_l) & ~3;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            unsigned w4[4] = {rb_split1(v[b][4 * j], s), rb_split1(v[b][4 * j + 1], s), rb_split1(v[b][4 * j + 2], s), rb_split1(v[b][4 * j + 3], s)};
            quad_transpose(w4, lane);
            const int i = 8 * j + (lane & 3) + 4 * rq;
            char* const d = tw + (cq >> 4) * 1024 + i * 32 + (((((cq >> 3) ^ (i >> 3)) & 1)) << 4) + (cq & 7) * 2;
            *(uint2*)d = uint2{__builtin_amdgcn_perm(w4[1], w4[0], 0x05040100u), __builtin_amdgcn_perm(w4[3], w4[2], 0x05040100u)};
            *(uint2*)(d + 4096) = uint2{__builtin_amdgcn_perm(w4[1], w4[0], 0x07060302u), __builtin_amdgcn_perm(w4[3], w4[2], 0x07060302u)};
          }
        }
      };
      to_frags(o2v, s_o2);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // panel 0's planes, its residual values, the fragments
      f16x8 fa3[4][2];
      {
        const char* const ta = tw + (lane & 31) * 32 + (((kh2 ^ ((lane & 31) >> 3)) & 1) << 4);
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
#pragma unroll
          for (int q = 0; q < 2; q++) fa3[kt][q] = *(const f16x8*)(ta + q * 4096 + kt * 1024);
      }
      const float inv3 = 1.f / (s_o2 * *t.s_w3);
      // FUSE == 2.  W1's planes of the K chunk that panel pn of `out` is (steps 4 pn ..): 4 steps x 2 planes x 2 blocks, four per wave
      const float s_out = NEXT ? (t.s_o2_amax ? f16_scale_of(*t.s_out) : *t.s_out) : 1.f;
      auto copy_w1 = [&](int pn) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int item = wave * 4 + i, st = item >> 2, q = (item >> 1) & 1, blk = item & 1;
          c64_dma16(t.w1pl + q * t.w1pl_stride + (long)((pn * 4 + st) * 2 + blk) * 512 + lane * 8,
                    sm + C64_W1B + ((st * 2 + q) * 2 + blk) * 1024);
        }
      };
      f32x16 acc1[2];
      float cnz = 0.f;   // non-zero values of `out` this lane stored (the wave's range test of `out` as an operand)
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc1[b][r] = 0.f;
      auto panel = [&](auto pnc) {
        constexpr int pn = decltype(pnc)::value;
        constexpr int US = NEXT ? 0 : (pn & 1);   // FUSE == 2 has one set of residual registers, requested when the set is consumed
        // planes of panel pn: issued a panel ago, with nothing but that panel's 32 stores behind them (vector memory operations
        // retire in order; the residual values of this panel were requested BEFORE the copy, so they are here as well)
        if constexpr (!NEXT) {
          if constexpr (pn > 0) asm volatile("s_waitcnt vmcnt(32)\n\ts_barrier" ::: "memory");
          if constexpr (pn + 1 < 4) {
            request(std::integral_constant<int, pn + 1>{});
            asm volatile("" ::: "memory");
            copy_w3(pn + 1);   // into the buffer everybody finished reading before this barrier
          }
        } else {
          // FUSE == 2: W3's planes of this panel landed before the barrier in the middle of the previous panel (they were issued before
          // W1's chunk, which that barrier waited for); this barrier frees W3's other buffer and W1's chunk buffer
          if constexpr (pn > 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
          if constexpr (pn + 1 < 4) copy_w3(pn + 1);
          copy_w1(pn);
        }
        f32x16 a3[2];
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
          for (int r = 0; r < 16; r++) a3[b][r] = 0.f;
        const char* const pb = sm + boff + ((pn + 1) & 1) * 16384;
#pragma unroll
        for (int kt = 0; kt < 4; kt++) {
          f16x8 fb[2][2];
#pragma unroll
          for (int q = 0; q < 2; q++)
#pragma unroll
            for (int b = 0; b < 2; b++) fb[q][b] = *(const f16x8*)(pb + ((kt * 2 + q) * 2 + b) * 1024);
#pragma unroll
          for (int pr = 0; pr < 3; pr++) {   // (h, l), (l, h), (h, h): the row-resident kernel's order
            const int qa = pr == 1 ? 1 : 0, qb = pr == 0 ? 1 : 0;
#pragma unroll
            for (int b = 0; b < 2; b++) a3[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa3[kt][qa], fb[qb][b], a3[b], 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);   // (left alone the compiler hoists the fragment reads of all steps, and spills)
        }
#pragma unroll
        for (int b = 0; b < 2; b++) {
          float sc = sc3[pn][b];
          sc *= inv3;   // operands were scaled by powers of two: exact rescale of the accumulated sum
          const float sh = sh3[pn][b];
#pragma unroll
          for (int r = 0; r < 16; r++) {   // same expressions as conv1x1_rows_kernel
            float v = a3[b][r] * sc + sh;
            v += ur[US][b][r];
            v = max_nan(v, 0.f);
            const bool ok = po[r] != 0x80000000u;
            const float av = ok ? fabsf(v) : 0.f;
            amx = max_nan(amx, av);
            asum += av;
            acnt += ok ? 1.f : 0.f;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, (int)po[r], (pn * 64 + b * 32) * 4, 0);
            if constexpr (NEXT) { a3[b][r] = v; cnz += av > 0.f ? 1.f : 0.f; }
          }
        }
        if constexpr (NEXT) {
          if constexpr (pn + 1 < 4) {   // the next panel's residual values, into the registers just consumed
            asm volatile("" ::: "memory");
            request(std::integral_constant<int, pn + 1>{});
            asm volatile("" ::: "memory");
          }
          to_frags(a3, s_out);   // this panel of `out` as A fragments of K steps 4 pn .., through the wave's own 8 KB
          // W1's chunk: behind its four copies (and W3's four before them) came 32 stores and, before the last panel, 32 requests --
          // with at most 63 (32) operations left, all eight copies have landed (vector memory operations retire in order)
          if constexpr (pn + 1 < 4) asm volatile("s_waitcnt vmcnt(63) lgkmcnt(0)\n\ts_barrier" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(32) lgkmcnt(0)\n\ts_barrier" ::: "memory");
          const char* const ta = tw + (lane & 31) * 32 + (((kh2 ^ ((lane & 31) >> 3)) & 1) << 4);
          const char* const pb1 = sm + C64_W1B + (boff - C64_BOFF);
#pragma unroll
          for (int kt = 0; kt < 4; kt++) {
            f16x8 fa[2], fb[2][2];
#pragma unroll
            for (int q = 0; q < 2; q++) fa[q] = *(const f16x8*)(ta + q * 4096 + kt * 1024);
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
              for (int b = 0; b < 2; b++) fb[q][b] = *(const f16x8*)(pb1 + ((kt * 2 + q) * 2 + b) * 1024);
#pragma unroll
            for (int pr = 0; pr < 3; pr++) {
              const int qa = pr == 1 ? 1 : 0, qb = pr == 0 ? 1 : 0;
#pragma unroll
              for (int b = 0; b < 2; b++) acc1[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[qa], fb[qb][b], acc1[b], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      };
      panel(std::integral_constant<int, 0>{});
      panel(std::integral_constant<int, 1>{});
      panel(std::integral_constant<int, 2>{});
      panel(std::integral_constant<int, 3>{});
      if constexpr (NEXT) {
        // the wave's own range test of `out` at the scale it was split with (its 32 pixels x 256 channels): wave-uniform
        float wm = amx, ws = asum, wc = cnz;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          wm = max_nan(wm, __shfl_xor(wm, o, 64));
          ws += __shfl_xor(ws, o, 64);
          wc += __shfl_xor(wc, o, 64);
        }
        const bool bad = !t.s_o2_amax && (!(wm <= 3.0e38f) || !(s_out > 0.f) || wm * s_out > 60000.f || (ws > 0.f && wc > ws * s_out * 32.f));
        if (bad) {
          c64_next_exact(p, t, img, oy0, ox0, wave, lane, nmx, nsum, ncnt);
        } else {
          const float inv1 = 1.f / (s_out * *t.s_w1);
          const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc((void*)t.o1n, 0, (int)((long)p.M * 256), 0x00020000);
#pragma unroll
          for (int b = 0; b < 2; b++) {
            float sc = t.scale1 ? t.scale1[b * 32 + col_l] : 1.f;
            sc *= inv1;
            const float sh = t.shift1 ? t.shift1[b * 32 + col_l] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
              float v = acc1[b][r] * sc + sh;
              v = max_nan(v, 0.f);
              const bool ok = po[r] != 0x80000000u;
              const float av = ok ? fabsf(v) : 0.f;
              nmx = max_nan(nmx, av);
              nsum += av;
              ncnt += ok ? 1.f : 0.f;
              const unsigned o = ok ? ((po[r] - (unsigned)col_l * 4u) >> 2) + (unsigned)col_l * 4u : 0x80000000u;
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rn, (int)o, b * 32 * 4, 0);
            }
          }
        }
      }
    }
    if (t.amax_out) {
      __syncthreads();
      c64_commit(t.amax_out, true, amx, asum, acnt, lds + C64_RED / 4, wave, lane, tid, t.out_amax_next);
    }
    if (FUSE == 2 && t.amax_o1n) {
      if (!t.amax_out) __syncthreads();
      c64_commit(t.amax_o1n, true, nmx, nsum, ncnt, lds + C64_RED / 4 + 64, wave, lane, tid);
    }
    return;
  }
  // ---- epilogue from the registers: acc[b][r] = MFMA row i = 8 (r / 4) + r % 4 + 4 (lane / 32), channel 32 b + lane % 32
  const int col_l = lane & 31, rq = lane >> 5;
  const float inv = 1.f / (sx * *p.f16_sw);
  const int ybytes = (int)((long)p.M * 64 * 4);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)p.y, 0, ybytes, 0x00020000);
  float amx = 0.f, asum = 0.f, acnt = 0.f;
#pragma unroll
  for (int b = 0; b < 2; b++) {
    const float sc = (p.scale ? p.scale[b * 32 + col_l] : 1.f) * inv, sh = p.shift ? p.shift[b * 32 + col_l] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int i = 8 * (r >> 2) + (r & 3) + 4 * rq;
      const int oy = oy0 + 2 * wave + (i >> 4), ox = ox0 + (i & 15);
      float v = acc[b][r] * sc + sh;
      if (p.relu) v = max_nan(v, 0.f);
      const bool ok = oy < p.Ho && ox < p.Wo;
      const float av = ok ? fabsf(v) : 0.f;
      amx = max_nan(amx, av);
      asum += av;
      acnt += ok ? 1.f : 0.f;
      const unsigned off = ok ? (unsigned)(((img * p.Ho + oy) * p.Wo + ox) * 64 + b * 32 + col_l) * 4u : 0x80000000u;
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, (int)off, 0, 0);
    }
  }
  if (p.amax_out) {
    __syncthreads();
    float* const red = lds;
    const bool stats = p.amax_stats && (blockIdx.x & 63) == 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amx = max_nan(amx, __shfl_xor(amx, o, 64));
    if (stats) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { asum += __shfl_xor(asum, o, 64); acnt += __shfl_xor(acnt, o, 64); }
    }
    if (lane == 0) { red[wave] = amx; red[16 + wave] = asum; red[32 + wave] = acnt; }
    __syncthreads();
    if (tid == 0) {
      float m = red[0], sm_ = red[16], cn = red[32];
      for (int i = 1; i < 4; i++) { m = max_nan(m, red[i]); sm_ += red[16 + i]; cn += red[32 + i]; }
      const unsigned bits = __builtin_bit_cast(unsigned, m);
      if (bits > __hip_atomic_load(p.amax_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p.amax_out, bits);
      // (the producing site's pending maximum: what the fused launch's scale of o2 is folded from while the two launches still run)
      if (p.amax_next && bits > __hip_atomic_load(p.amax_next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p.amax_next, bits);
      if (stats && cn > 0.f) {
        const int k = (blockIdx.x >> 6) & 15;
        atomicAdd((float*)p.amax_out + 1 + k, sm_);
        atomicAdd((float*)p.amax_out + 17 + k, cn);
      }
    }
  }
}


}  // namespace

namespace mmtconv {
// one launch of a form of the kernel (0: the 3x3 alone, 1: + conv3, 2: + the next block's conv1)
template <int FUSE>
static int launch_c64_form(const ConvP& p, const C64Tail& t, hipStream_t s) {
  constexpr int LDS = C64_BOFF + 2 * 16384;
  static bool done = false;
  if (!done) {
    const hipError_t e = hipFuncSetAttribute((const void*)conv3x3_c64_kernel<FUSE>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    if (e != hipSuccess) return (int)e;
    done = true;
  }
  const int tiles = p.N * ((p.Ho + 7) >> 3) * ((p.Wo + 15) >> 4);
  hipLaunchKernelGGL(conv3x3_c64_kernel<FUSE>, dim3(tiles), dim3(256), LDS, s, p, t);
  MMT_LAUNCH_CHECK();
  return 0;
}

int launch_c64(const ConvP& p, hipStream_t s) { return launch_c64_form<0>(p, C64Tail{}, s); }
}  // namespace mmtconv

extern "C" int mmt_c64_conv3_fused(const float* x, int N, int H, int W, const float* w2, const void* w2_planes, long w2_plane_stride,
                                   const float* s_w2, const float* scale2, const float* shift2, const float* x_slot, const float* w3,
                                   const void* w3_planes, long w3_plane_stride, const float* s_w3, const float* scale3,
                                   const float* shift3, const float* res, float* out, float* out_slot, const float* o2_scale,
                                   int o2_scale_is_amax, float* o2_amax_next, float* out_amax_next, const float* w1,
                                   const void* w1_planes, long w1_plane_stride, const float* s_w1, const float* scale1,
                                   const float* shift1, const float* out_scale, float* o1_next, float* o1_next_slot, void* stream) {
  if (!x || !w2 || !w2_planes || !s_w2 || !x_slot || !w3 || !w3_planes || !s_w3 || !res || !out || !o2_scale || N <= 0 || H <= 0 || W <= 0 ||
      (((size_t)w2_planes | (size_t)w3_planes | (size_t)x) & 15) || ((w2_plane_stride | w3_plane_stride) & 7) ||
      (((size_t)res | (size_t)out) & 3) || precision() != 3)
    return MMT_EINVAL;
  if (w1_planes && (!w1 || !s_w1 || !out_scale || !o1_next || ((size_t)w1_planes & 15) || (w1_plane_stride & 7) || ((size_t)o1_next & 3) ||
                    (const void*)res == (const void*)out))
    return MMT_EINVAL;
  if ((long)N * H * W * 1024 >= (1L << 31)) return MMT_EINVAL;   // 32-bit byte offsets into out / res
  ConvP p = {};
  p.x = x; p.w = w2; p.scale = scale2; p.shift = shift2;
  p.N = N; p.H = p.Ho = H; p.W = p.Wo = W; p.Cin = p.Cout = 64; p.KH = p.KW = 3; p.stride = 1; p.pad = 1;
  p.relu = 1; p.out_stride = 1; p.M = N * H * W; p.K = 576; p.cin32 = p.cin4 = 1;
  p.wpl = (const unsigned short*)w2_planes; p.wpl_stride = w2_plane_stride;
  p.f16_sx = x_slot; p.f16_ax = 1; p.f16_sw = s_w2; p.guard_x = x_slot;
  C64Tail t = {};
  t.w3pl = (const unsigned short*)w3_planes; t.w3pl_stride = w3_plane_stride; t.w3 = w3; t.scale = scale3; t.shift = shift3;
  t.res = res; t.out = out; t.s_w3 = s_w3; t.s_o2 = o2_scale; t.s_o2_amax = o2_scale_is_amax ? 1 : 0;
  t.o2_amax_next = (unsigned*)o2_amax_next; t.amax_out = (unsigned*)out_slot; t.out_amax_next = (unsigned*)out_amax_next;
  if (!w1_planes) return launch_c64_form<1>(p, t, (hipStream_t)stream);
  t.w1pl = (const unsigned short*)w1_planes; t.w1pl_stride = w1_plane_stride; t.w1 = w1; t.scale1 = scale1; t.shift1 = shift1;
  t.s_w1 = s_w1; t.s_out = out_scale; t.o1n = o1_next; t.amax_o1n = (unsigned*)o1_next_slot;
  return launch_c64_form<2>(p, t, (hipStream_t)stream);
}

extern "C" int mmt_stem_fused(const float* x, int N, int H, int W, const float* w_s2d, const void* w_planes, long w_plane_stride,
                              const float* s_w, const float* scale, const float* shift, const float* x_slot, float* y, float* y_slot,
                              void* stream) {
  if (!x || !w_s2d || !w_planes || !s_w || !scale || !shift || !x_slot || !y || N <= 0 || H < 8 || W < 8 || (H & 3) || (W & 3) ||
      ((size_t)w_planes & 15) || (w_plane_stride & 7) || ((size_t)x & 7) || ((size_t)y & 15) || precision() != 3)
    return MMT_EINVAL;
  if ((long)N * 3 * H * W >= (1L << 31)) return MMT_EINVAL;
  StemP p;
  p.x = x; p.wpl = (const unsigned short*)w_planes; p.wpl_stride = w_plane_stride; p.w = w_s2d;
  p.scale = scale; p.shift = shift; p.y = y; p.x_slot = x_slot; p.s_w = s_w;
  p.amax_out = (unsigned*)y_slot; p.amax_stats = y_slot ? 1 : 0;
  p.N = N; p.H = H; p.W = W; p.Hc = H / 2; p.Wc = W / 2; p.Hp = H / 4; p.Wp = W / 4;
  p.tiles_y = mmt_cdiv(p.Hp, 7); p.tiles_x = mmt_cdiv(p.Wp, 15);
  static bool done = false;
  if (!done) {
    const hipError_t e = hipFuncSetAttribute((const void*)stem_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, STEM_LDS);
    if (e != hipSuccess) return (int)e;
    done = true;
  }
  hipLaunchKernelGGL(stem_fused_kernel, dim3(N * p.tiles_y * p.tiles_x), dim3(512), STEM_LDS, (hipStream_t)stream, p);
  MMT_LAUNCH_CHECK();
  return 0;
}
