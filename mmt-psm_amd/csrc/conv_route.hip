// Which kernel a convolution call runs on: the ONE owner of that decision (include/mmtpsm.h: mmt_conv_route; the weight gradient:
// mmt_conv_wgrad_route, wgrad_route below).  Host code only.
// mmt_conv_forward, mmt_conv_forward_f16x2, mmt_conv3x3_strip_f16x2 and mmt_conv_forward_pg compute route() and switch on it; the
// host side asks mmt_conv_route with the same block.  Every shape test, tuned threshold and forward switch of the environment lives
// in this file and is private to it; the tuned values are those of profiles/r04_dispatch_sweep.txt unless a comment says otherwise.
#include "conv_shared.h"

namespace {
using namespace mmtconv;

// the six forward switches and the weight gradient's two (A/B timing, parity tests): read per route, i.e. per call -- the tests flip
// them between launches
bool on(const char* name) {
  const char* e = getenv(name);
  return !(e && atoi(e) == 0);
}
int read_switches() {
  return (on("MMT_SPLITK") ? MMT_SW_SPLITK : 0) | (on("MMT_STRIP") ? MMT_SW_STRIP : 0) | (on("MMT_ROWS") ? MMT_SW_ROWS : 0) |
         (on("MMT_PG") ? MMT_SW_PG : 0) | (on("MMT_C64") ? MMT_SW_C64 : 0) | (on("MMT_DIRECT_EPI") ? MMT_SW_DIRECT_EPI : 0) |
         wgrad_switches();
}

// operands that are in the block or promised by the caller (promised planes are promised aligned)
struct Have { bool w, wpl, xpl, f16; };

// tile variant of the tiled kernels: 0 = 128 x 32 (Cout <= 32: fp32 MFMA only), 1 = 128 x 128, 2 = 64 x 64, 3 = 128 x 64
int pick_variant(const ConvP& p) {
  if (p.Cout <= 32) return 0;
  // K <= 256 (the 1x1 layers of layer1/layer2/FPN laterals): 2-8 k-tiles per output tile, so prologue and epilogue
  // dominate; the 64x64 configuration keeps ~4x more blocks resident to overlap them (measured +10..25 %)
  constexpr int lowk = 256, lowv = 3;
  if (p.K <= lowk) return (p.Cout >= 64 && (long)mmt_cdiv(p.M, 128) * mmt_cdiv(p.Cout, 64) >= 768) ? lowv : 2;
  // enough 128x128 tiles to fill 256 CUs (2 resident blocks each) -> 128x128; else 128x64 (twice the blocks, A tile
  // still reused across 64 output channels); else 64x64 (4x the blocks)
  const long t128 = (long)mmt_cdiv(p.M, 128) * mmt_cdiv(p.Cout, 128);
  constexpr int t128min = 256;
  if (t128 >= t128min && p.Cout > 64) return 1;
  const long t12864 = (long)mmt_cdiv(p.M, 128) * mmt_cdiv(p.Cout, 64);
  if (t12864 >= 256 && p.Cout >= 64) return 3;
  return 2;
}

// number of K ranges for the 128 x 128 kernel: fill the 512 resident block slots when the tiles alone do not, keeping
// at least 32 steps per range
int pick_ksplit(const ConvP& p, int sw) {
  if (!(sw & MMT_SW_SPLITK) || p.Cout < 128) return 1;
  const long t128 = (long)mmt_cdiv(p.M, 128) * mmt_cdiv(p.Cout, 128);
  const int nkt = p.K >> 4;
  constexpr int tmax = 512, kmin = 128;
  if (t128 >= tmax || nkt < kmin) return 1;  // K >= 2048: shorter sums lose more in the second launch than they gain
  int ks = (int)(512 / t128);
  if (ks > nkt / 32) ks = nkt / 32;
  if (ks > 16) ks = 16;
  return ks < 2 ? 1 : ks;
}

// K ranges for the tap-strip kernel: 1 when its 256 x 128 tiles fill the chip (one 512-thread block per CU), else enough
// ranges to do so -- possible when a tile's pixels are consecutive in memory (Wo == TW: the finish kernel's row mapping),
// Cout is a multiple of 128 and every range keeps >= 6 super-steps; 0 = not a shape for this kernel
int strip_ksplit(const ConvP& p, int tw, int sw) {
  const long tiles = (long)p.N * (p.Ho * p.Wo / 256) * mmt_cdiv(p.Cout, 128);
  if (tiles >= 256) return 1;
  // fp32 tensors (the split arithmetics): a few-tile shape is NOT taken -- this kernel needs its input as pre-split planes, a pass
  // of its own over the tensor (~9 us on the student's N = 2 maps) that the tiled kernel, which splits in registers, does not; with
  // equal kernel times (profiles/r04_dispatch_sweep.txt: 35.07 vs 35.12-35.23 ms) the pass is what counts: 32 fewer launches per
  // step, 35.55 -> 35.34 ms in three same-box alternations (round 4).  bf16-stored tensors ARE their plane: split form kept.
  if (!(p.io & IO_X)) return 0;
  if (!(sw & MMT_SW_SPLITK) || p.Wo != tw || (p.Cout & 127) || tiles < 32) return 0;
  int ks = (int)((256 + tiles - 1) / tiles);
  const int pairs = 3 * (p.Cin >> 4) / 2;
  if (ks > pairs / 3) ks = pairs / 3;
  if (ks > 8) ks = 8;
  if (tiles * ks > 512) ks = (int)(512 / tiles);
  return ks >= 2 ? ks : 0;
}

// K order of the tap-strip kernel (bits 24-30 of its ksplit argument = slabs per group, 0 = kh outermost as in rounds 2-5): groups
// of 4 slabs, fewer where Cin / 16 is not a multiple of 4 (profiles/r06_strip_korder.txt): the fabric reads of 1 (141 MB per launch
// instead of 278) at the cycle count of 0 -- every change of kh recomputes the copy slots' row offsets, which costs 7 % of the
// kernel's cycles when it happens every super-step and 1 % every fourth
int strip_korder(const ConvP& p) {
  int g = 4;
  while (g > 1 && ((p.Cin >> 4) % g) != 0) g >>= 1;
  return g << 24;
}

// 3x3 / stride 1 / pad 1 with both operands as planes: which strip width (0 = not taken)
int strip_tw(const ConvP& p, const Have& h, int sw) {
  if (!h.xpl || !h.wpl || p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1 || p.out_stride != 1 || p.Ho != p.H || p.Wo != p.W ||
      (p.Cin & 31) || p.Cout <= 32 || ((size_t)p.xpl & 15) || (p.xpl_stride & 7) || !(sw & MMT_SW_STRIP))
    return 0;
  int tw = 0;
  if (p.Wo % 128 == 0 && p.Ho % 2 == 0) tw = 128;   // 2 image rows x 128 pixels per tile; 4 x 64 where Wo % 128 != 0
  else if (p.Wo % 64 == 0 && p.Ho % 4 == 0) tw = 64;
  constexpr int minc = 128;
  if (!tw || p.Cin < minc) return 0;  // K = 576 (the 64-channel layer1 convs): 12 super-steps do not amortise the fill
  return strip_ksplit(p, tw, sw) ? tw : 0;
}

// panels per block of the row-resident 1x1 kernel: all of them when the row blocks alone fill the chip (>= 512 resident
// slots), else column groups so that about 512 blocks exist (256 / 1024 / 2048 measured slower: profiles/r04_rows_epilogue.txt)
int rows_ppb(const ConvP& p) {
  const int tiles_m = mmt_cdiv(p.M, 128), npanel = mmt_cdiv(p.Cout, 32);
  if (tiles_m >= 512) return npanel;
  int groups = mmt_cdiv(512, tiles_m);
  if (groups > npanel) groups = npanel;
  return mmt_cdiv(npanel, groups);
}

// is this call one for the row-resident 1x1 kernel?  (K = 64 / 128 in every split mode; K = 256 on the fp16 split only)
bool rows_shape(const ConvP& p, bool f16, int sw) {
  constexpr int rows_min = 256;   // blocks of 128 rows (bf16 split)
  constexpr int rows_min16 = 16;
  if (!(sw & MMT_SW_ROWS) || p.io || p.KH != 1 || p.KW != 1 || p.stride != 1 || p.pad != 0 || p.Cout < 64 || (p.Cout & 3) ||
      p.res_mode > 2 || p.mul || p.out_stride != 1 || (long)p.M * p.Cin * 4 >= (1L << 31) || (long)p.M * p.Cout * 4 >= (1L << 31) ||
      (p.res_mode == 2 && (p.Wo & 7)))
    return false;
  if (f16) return (p.Cin == 64 || p.Cin == 128 || p.Cin == 256) && p.M >= 128 * rows_min16;
  return !p.mask && p.res_mode <= 1 && (p.Cin == 64 || p.Cin == 128) && p.M >= 128 * rows_min;
}

// 3x3 / stride 1 / pad 1 with 64 input and 64 output channels on fp32 tensors, plain affine (+ ReLU) epilogue: layer1's conv2
bool c64_shape(const ConvP& p, const Have& h, int sw) {
  return (sw & MMT_SW_C64) && p.Cin == 64 && p.Cout == 64 && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Ho == p.H &&
         p.Wo == p.W && !p.io && !p.ypl && !p.mul && !p.mask && p.res_mode == 0 && p.out_stride == 1 && h.wpl && h.w && h.f16 &&
         (long)p.M * 64 * 4 < (1L << 31);
}

// is this call one the plane-fed kernel takes?  (shape / epilogue form only)
bool pg_shape(const ConvP& p, const Have& h) {
  return h.xpl && h.wpl && !p.io && !p.ypl && !p.mul && p.out_stride == 1 && p.res_mode <= 1 && (p.Cin & 15) == 0 && p.Cout > 32 &&
         (long)p.N * p.H * p.W * p.Cin < (1L << 29) && (long)p.M * p.Cout * 4 < (1L << 31) && ((size_t)p.xpl & 15) == 0 &&
         (p.xpl_stride & 7) == 0 && ((size_t)p.wpl & 15) == 0 && (p.wpl_stride & 7) == 0;
}

// tile height (64 / 128 / 256 rows: 4 / 2 / 1 K groups inside the block) and K ranges across blocks.  Every block is 8 waves and
// takes a CU for itself: the tallest tile that still gives (nearly) every CU a block; K ranges across blocks only when even the
// 64-row tiles leave half the chip empty and K is long
void pg_plan(const ConvP& p, int sw, int& rows, int& ksplit) {
  const long tn = mmt_cdiv(p.Cout, 128);
  const long t256 = (long)mmt_cdiv(p.M, 256) * tn, t128 = (long)mmt_cdiv(p.M, 128) * tn, t64 = (long)mmt_cdiv(p.M, 64) * tn;
  const int nkt = p.K >> 4;
  rows = t256 >= 448 ? 256 : (t128 >= 224 ? 128 : 64);
  ksplit = 1;
  if (rows == 64 && t64 > 0 && t64 <= 128 && (sw & MMT_SW_SPLITK)) {
    int ks = (int)(256 / t64);
    if (ks > nkt / 64) ks = nkt / 64;     // >= 16 steps per group and range
    if (ks > 8) ks = 8;
    if (ks >= 2) ksplit = ks;
  }
}

// would the launch write row-blocked planes of y from its epilogue (mmt_conv_args.y_rb)?  The register-direct, LDS-staged,
// split-K-finish and row-resident epilogues do; the patch kernel (layer1's 3x3) does not
bool rb_epilogue_ok(const ConvP& p) {
  return !((p.Cout & 15) || p.out_stride > 1 || (p.io & IO_Y) || p.mul || (long)p.M * p.Cout >= (1L << 30));
}

void tile_of_variant(Route& r, int variant) {
  r.bm = variant == 2 ? 64 : 128;
  r.bn = variant == 0 ? 32 : (variant == 1 ? 128 : 64);
}

// the tiled DMA-fed kernels: the split-K form runs on the 128 x 128 kernel whatever the tile variant would have been
void take_tiled(Route& r, int family, int variant, int ksplit) {
  r.family = family;
  r.ksplit = ksplit;
  r.tag = ksplit > 1 ? 1 : variant;
  tile_of_variant(r, r.tag);
}

void take_rows(Route& r, const ConvP& p, int variant) {
  r.family = MMT_ROUTE_ROWS; r.tag = variant; r.bm = 128; r.bn = 32; r.panels = rows_ppb(p);
}

void take_strip(Route& r, int x_form) {
  r.family = MMT_ROUTE_STRIP; r.tag = 4; r.bm = 256; r.bn = 128; r.ksplit = r.strip_ksplit; r.x_form = x_form;
}

// ---- the weight gradient

// pixel ranges of the register-fed kernels: `want` of them, each at least 512 pixels (32 k-tiles per block) and a multiple of 32
void wg_ranges(int M, long want, int& splits, int& mps) {
  constexpr int min_px = 512;   // (tuned: profiles/r04_dispatch_sweep.txt; in the step: profiles/r04_history.md)
  if (want > mmt_cdiv(M, min_px)) want = mmt_cdiv(M, min_px);
  if (want < 1) want = 1;
  mps = (mmt_cdiv(M, (int)want) + 31) / 32 * 32;
  splits = mmt_cdiv(M, mps);
}

// pixel ranges across blocks of the plane-fed kernel, 0: not one of its layers.  T: the 32-pixel super-steps of the reduction
int wgpl_ranges(const ConvP& p, int mode, int sw, long& T) {
  T = ((long)p.N * p.H * p.W) >> 5;
  if (mode != 3 || !(sw & MMT_SW_WGRAD_PLANES) || p.stride != 1 || p.Ho != p.H || p.Wo != p.W || (p.W & 31) || (p.Cin & 127) ||
      (p.Cout & 127) || p.KH != p.KW || p.pad != (p.KH - 1) / 2 || !(p.KH & 1) || p.io || T < 2 ||
      (long)p.N * p.H * p.W * (p.Cin > p.Cout ? p.Cin : p.Cout) >= (1L << 29))
    return 0;
  // blocks per launch the pixel ranges aim at: profiles/r06_history.md.  The three-tap form has a third of the tiles and blocks that
  // multiply three times as much per super-step: the same target gives it three times the ranges and blocks of the same duration
  // (sweep of 128 / 192 / 256 / 384, isolated and in the step: profiles/wgrad_kw3_ab.txt)
  constexpr long target = 256;
  long ks = target / ((long)(p.Cout >> 7) * wg_tiles_n(p.KH, p.KW, p.Cin));
  if (ks > T / 8) ks = T / 8;     // >= 4 super-steps per group and range (one tap); >= 8 per range behind the ring's three (three taps)
  return ks < 1 ? 1 : (int)ks;
}

}  // namespace

namespace mmtconv {

int wgrad_switches() { return (on("MMT_WGRAD_PLANES") ? MMT_SW_WGRAD_PLANES : 0) | (on("MMT_WGRAD_GROUP") ? MMT_SW_WGRAD_GROUP : 0); }

WgradRoute wgrad_route(const ConvP& p, int mode, int have, int sw) {
  WgradRoute r = {};
  r.switches = sw;
  r.splits = r.group_splits = 1;
  if (p.M == 0 || p.Cout == 0) return r;   // nothing to launch
  // Pixel ranges per job inside a group: 1 / WG_DIV of what the job would use ALONE.  Measured in the step (profiles/r06_history.md
  // section 7): filling the chip as a group makes blocks that own a CU for ~150 us and hold up the step stream's latency-bound chain
  // (+2 ms); the jobs' own ranges only save launches and reduces (-0.3 ms); a quarter of them is the optimum (-0.5 ... -0.75 ms):
  // blocks four times as long, a quarter of the slab traffic, still short
  // (WG_DIV_PL: the plane-fed jobs' divisor.  The three-tap form has a third of the tiles and three times the ranges of the one-tap
  // form at equal block duration; swept again in the step with it, 2 / 4 / 8 are not separable: profiles/wgrad_kw3_ab.txt)
  constexpr int WG_DIV = 4, WG_DIV_PL = 4;
  const bool group = (sw & MMT_SW_WGRAD_GROUP) != 0;
  long T;
  const int ks = (have & MMT_WG_HAVE_PLANES) ? wgpl_ranges(p, mode, sw, T) : 0;
  if (ks) {
    r.family = p.KW == 3 ? MMT_WGRAD_PLANES_3 : MMT_WGRAD_PLANES_1;
    r.terms = 2; r.splits = ks; r.lds_bytes = WGPL_LDS; r.dbias_in_kernel = 1;
    r.ws_floats = ks > 1 ? (long)ks * p.Cout * p.K : 0;
    long gs = (ks + WG_DIV_PL - 1) / WG_DIV_PL;
    if (gs > T / 8) gs = T / 8;
    r.group_splits = gs < 1 ? 1 : (int)gs;
    r.group_kind = group ? 1 : 0;
  } else {
    // all blocks of a launch run equally long: fill the 512 resident slots (256 CUs x 2 blocks) ONCE.  (640 = 1.25
    // rounds cost a second, 20 %-full round: 92 -> 105 TFLOP/s fp32, 103 -> 136 split-bf16 on the FPN 3x3 shapes)
    constexpr int slots = 512;    // (tuned: profiles/r04_dispatch_sweep.txt; in the step: r04 / r06 history)
    const long tiles = (long)mmt_cdiv(p.K, 128) * mmt_cdiv(p.Cout, 128);
    wg_ranges(p.M, tiles >= slots ? 1 : slots / tiles, r.splits, r.mps);
    r.ws_floats = r.splits > 1 ? (long)r.splits * p.Cout * p.K : 0;
    wg_ranges(p.M, (r.splits + WG_DIV - 1) / WG_DIV, r.group_splits, r.group_mps);
    r.decode = !(p.Wo >= 8 && p.Ho >= 8) ? 0 : ((p.Wo & 3) == 0 ? 2 : 1);
    r.vec4 = (p.Cout & 3) == 0;
    r.bf = ((p.io & IO_X) ? 1 : 0) | ((p.io & IO_DY) ? 2 : 0);   // bf16 storage of x / dy: mode 1, the pipelined kernel with 4-channel loads only
    // the pipelined kernel addresses both operands with 32-bit byte offsets (buffer loads)
    const bool small = (long)p.N * p.H * p.W * p.Cin * 4 < (1L << 31) && (long)p.M * p.Cout * 4 < (1L << 31);
    r.lds_bytes = 65536;   // the 64 KB epilogue tile (>= 3 stages of 16 KB); fp32: 4 stages of 4096 floats
    r.dbias_in_kernel = 1;
    const bool f16 = (have & MMT_WG_HAVE_MAXIMA) != 0;   // the two-term fp16 split: mode 3, fp32 tensors
    if (!p.cin4 || (f16 ? !(mode == 3 && !r.bf && r.vec4 && small) : (r.bf && !(mode == 1 && r.vec4 && small)))) return r;   // no kernel
    if (f16) {
      r.family = MMT_WGRAD_PIPE_F16; r.terms = 2;
      r.group_kind = group && !p.io ? 2 + r.decode : 0;
    } else if (mode > 0 && small) {
      r.family = MMT_WGRAD_PIPE; r.terms = mode;
      if (mode >= 3) r.lds_bytes = 73728;            // the three operand stages of the 3-term split (3 x 24 KB)
    } else if (mode > 0 && r.vec4) { r.family = MMT_WGRAD_SPLIT; r.terms = mode; }
    else { r.family = r.vec4 && r.decode ? MMT_WGRAD_FP32_FAST : MMT_WGRAD_FP32_SLOW; r.dbias_in_kernel = 0; }
  }
  return r;
}

Route route(const ConvP& p, int mode, int entry, int assume) {
  Route r = {};
  r.kgroups = r.ksplit = 1;
  const int sw = r.switches = read_switches();
  const Have h = {p.w || (assume & MMT_ASSUME_W), p.wpl || (assume & MMT_ASSUME_W_PLANES),
                  p.xpl || (assume & MMT_ASSUME_X_PLANES) || ((p.io & IO_X) && (assume & MMT_ASSUME_X)),
                  (p.f16_sx && p.f16_sw) || (assume & MMT_ASSUME_F16_SCALARS)};
  const int v = pick_variant(p);
  auto plan_strip = [&] {
    r.strip_tw = strip_tw(p, h, sw);
    if (r.strip_tw) { r.strip_ksplit = strip_ksplit(p, r.strip_tw, sw); r.strip_korder = strip_korder(p); }
    return r.strip_tw != 0;
  };
  if (entry == MMT_ENTRY_F16) {
    // the two-term fp16 split: mode 3, fp32 tensors, no bf16 planes of y (all three entry points refuse the rest)
    if (mode != 3 || p.io || p.ypl) return r;
    const bool c64 = c64_shape(p, h, sw);
    r.writes_rb = rb_epilogue_ok(p) && !c64;
    plan_strip();
    if (pg_shape(p, h)) pg_plan(p, sw, r.pg_rows, r.pg_ksplit);
    // the plane-fed kernel is WANTED (with a plane-split pass of x in front) for the 3x3 and larger convolutions the tap-strip kernel
    // does not take; not for 1x1 / fc, whose inputs are large against their work -- the split pass costs what the leaner loop returns
    // (profiles/r05_bench_pg.txt); Cout = 64: half of every 128-column tile would be zeros
    const bool strip = r.strip_tw && !p.mul, pg = r.pg_rows && (sw & MMT_SW_PG) && p.M > 0 && p.Cout >= 96 && p.KH * p.KW >= 4;
    const bool tiled = v != 0 && (p.Cin & 15) == 0 && h.wpl;   // any convolution the DMA-fed kernel takes
    const bool rows = tiled && rows_shape(p, true, sw);
    r.wanted = (strip ? 1 << MMT_ROUTE_STRIP : 0) | (pg ? 1 << MMT_ROUTE_PG : 0) | (tiled && c64 ? 1 << MMT_ROUTE_C64 : 0) |
               (rows ? 1 << MMT_ROUTE_ROWS : 0) | (tiled ? 1 << MMT_ROUTE_DMA : 0);
    if (strip) take_strip(r, MMT_X_F16_PLANES);
    else if (pg) { r.family = MMT_ROUTE_PG; r.tag = 5; r.bm = r.pg_rows; r.bn = 128; r.kgroups = 256 / r.pg_rows; r.ksplit = r.pg_ksplit;
                   r.x_form = MMT_X_F16_PLANES; }
    else if (!tiled) r.tag = v;
    else if (c64) { r.family = MMT_ROUTE_C64; r.tag = v; }
    else if (rows) take_rows(r, p, v);   // 1x1 layers with K = 64 / 128 / 256: rows resident in registers as fp16 fragments
    else take_tiled(r, MMT_ROUTE_DMA, v, pick_ksplit(p, sw));
    return r;
  }
  // the library's own dispatch: packed weight planes -> the DMA-fed kernels (row-resident, tap-strip, tiled); a split mode without
  // them -> operands split in registers; mode 0 and the shapes the split kernels do not cover -> fp32-input MFMA
  if (mode > 0 && v != 0 && (p.Cin & 15) == 0 && h.wpl) {
    if (rows_shape(p, false, sw)) take_rows(r, p, v);   // 1x1 / stride 1 with K = 64 or 128 and many rows
    else if ((mode == 3 || (mode == 1 && (p.io & IO_X))) && plan_strip())   // mode 3 with x_planes given, mode 1 with x stored as bf16
      take_strip(r, (p.io & IO_X) ? MMT_X_AS_IS : MMT_X_BF16_PLANES);
    else take_tiled(r, (p.io & IO_X) ? MMT_ROUTE_DMA_BF16X : MMT_ROUTE_DMA, v, pick_ksplit(p, sw));
  } else {
    r.family = mode > 0 && v != 0 && (p.Cin & 15) == 0 ? MMT_ROUTE_SPLIT : MMT_ROUTE_FP32;
    r.tag = v;
    tile_of_variant(r, v);
  }
  r.wanted = 1 << r.family;
  return r;
}

}  // namespace mmtconv

extern "C" int mmt_conv_route(const mmt_conv_args* a, int entry, int assume, mmt_conv_route_t* out) {
  ConvP p;
  if (!out || (entry != MMT_ENTRY_LIB && entry != MMT_ENTRY_F16)) return MMT_EINVAL;
  const int e = fill(p, a, (assume & MMT_ASSUME_X) != 0);
  if (e) return e;
  *out = route(p, precision(), entry, assume);
  return 0;
}

extern "C" int mmt_conv_wgrad_route(const mmt_conv_args* a, int have, mmt_conv_wgrad_route_t* out) {
  ConvP p;
  if (!out) return MMT_EINVAL;
  const int e = fill(p, a, true);
  if (e) return e;
  *out = wgrad_route(p, precision(), have | (a->f16_x_amax && a->f16_dy_amax ? MMT_WG_HAVE_MAXIMA : 0), read_switches());
  return 0;
}

extern "C" int mmt_conv_switches(void) { return read_switches(); }
