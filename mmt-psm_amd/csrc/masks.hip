// On-device replacements for the two per-ROI CPU Python loops of the reference step:
//
//   paste_masks      <- mask_head/inference.py:29-65 (sigmoid, pick the predicted class),
//                       :120-206 (expand_masks / expand_boxes / paste_mask_in_image), :209-246 (Masker)
//                       and detector/generalized_rcnn.py:129-132 (sum over detections) -- the teacher's
//                       integral pseudo-mask, built with int atomics instead of D x (H,W) canvases.
//   polygon_targets  <- mask_head/loss.py:37-75 (project_masks_on_boxes),
//                       structures/segmentation_mask.py:96-133 (crop / resize / convert) and the
//                       rasteriser pycoco/maskApi.c:166-206 (rleFrPoly) + :53-74 (union merge).
//
// Built with -ffp-contract=off: thresholds (> 0.5) and floor/ceil decisions must round like the CPU code.
#include "common.h"

// ------------------------------------------------------------------------------------ paste
// The geometry and the bilinear value live in two functions that every paste kernel calls (the integral map, the byte stack and
// the mask words), so the forms cannot drift apart by a bit.
struct PasteGeom {
  int x0, y0;                  // the expanded integer box's corner (may lie outside the canvas)
  int cx0, cx1, cy0, cy1;      // the box clipped to the canvas, half open
  float sx, sy;                // source pixels per destination pixel
};

// expand_boxes (inference.py:120-135) with scale = (M+2)/M, then .to(int32) (truncation); false: nothing lands on the canvas
__device__ __forceinline__ bool paste_geom(const float* __restrict__ box, int M, int IH, int IW, PasteGeom& g) {
  const int P = M + 2;
  const float scale = (float)(M + 2) / (float)M;
  const float bx0 = box[0], by0 = box[1], bx1 = box[2], by1 = box[3];
  float wh = (bx1 - bx0) * .5f, hh = (by1 - by0) * .5f;
  const float xc = (bx1 + bx0) * .5f, yc = (by1 + by0) * .5f;
  wh *= scale; hh *= scale;
  const int x0 = (int)(xc - wh), x1 = (int)(xc + wh), y0 = (int)(yc - hh), y1 = (int)(yc + hh);
  const int w = max(x1 - x0 + 1, 1), h = max(y1 - y0 + 1, 1);
  g.x0 = x0; g.y0 = y0;
  g.cx0 = max(x0, 0); g.cx1 = min(x1 + 1, IW); g.cy0 = max(y0, 0); g.cy1 = min(y1 + 1, IH);
  // F.interpolate(bilinear, align_corners=False): src = (dst+0.5)*in/out - 0.5 clamped at 0
  g.sy = (float)P / (float)h; g.sx = (float)P / (float)w;
  return g.cx1 - g.cx0 > 0 && g.cy1 - g.cy0 > 0;
}

// the resized probability at canvas pixel (xx, yy) of the clipped box; pm = the (M+2)^2 padded probabilities
__device__ __forceinline__ float paste_value(const float* pm, int P, const PasteGeom& g, int xx, int yy) {
  const int dy = yy - g.y0, dx = xx - g.x0;
  float fy = g.sy * ((float)dy + 0.5f) - 0.5f;
  if (fy < 0.f) fy = 0.f;
  float fx = g.sx * ((float)dx + 0.5f) - 0.5f;
  if (fx < 0.f) fx = 0.f;
  // inside the box fy, fx < P - 0.5; the min only keeps a box of non-finite or overflowing corners inside pm
  const int iy0 = min((int)fy, P - 1), ix0 = min((int)fx, P - 1);
  const int iy1 = iy0 + (iy0 < P - 1 ? 1 : 0), ix1 = ix0 + (ix0 < P - 1 ? 1 : 0);
  const float ly1 = fy - (float)iy0, ly0 = 1.f - ly1, lx1 = fx - (float)ix0, lx0 = 1.f - lx1;
  return ly0 * (lx0 * pm[iy0 * P + ix0] + lx1 * pm[iy0 * P + ix1]) +
         ly1 * (lx0 * pm[iy1 * P + ix0] + lx1 * pm[iy1 * P + ix1]);
}

// detection d's M x M plane, zero-padded by one, into LDS; PROB: the input holds probabilities already (one class)
template <bool PROB>
__device__ __forceinline__ void paste_fill(float* pm, const float* __restrict__ logits, int d, int M, int NC, int lab) {
  const int P = M + 2;
  for (int i = threadIdx.x; i < P * P; i += 256) {
    const int y = i / P, x = i - y * P;
    float v = 0.f;
    if (y >= 1 && y <= M && x >= 1 && x <= M) {
      const float z = logits[(((long)d * M + (y - 1)) * M + (x - 1)) * NC + lab];
      v = PROB ? z : 1.f / (1.f + expf(-z));
    }
    pm[i] = v;
  }
}

// STACK: the evaluator's form (mask_head/inference.py:209-246 as pap_eval.py:107-109 calls it): the input holds the
// PROBABILITIES of the predicted class ((D, 1, M, M): MaskPostProcessor's `mask` field), and every detection gets its own
// binary canvas stack[d] (bytes) instead of a vote in the integral map of its image.
template <bool STACK>
__global__ __launch_bounds__(256) void paste_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                    const float* __restrict__ boxes, const int* __restrict__ img,
                                                    int M, int NC, int IH, int IW, float thresh,
                                                    int* __restrict__ seg, unsigned char* __restrict__ stack) {
  extern __shared__ float pm[];  // (M+2)^2 padded probabilities
  const int d = blockIdx.x;
  if (!STACK && img[d] < 0) return;   // a row behind its image's count in a fixed-capacity detection list: no vote
  const int P = M + 2;
  paste_fill<STACK>(pm, logits, d, M, NC, STACK ? 0 : labels[d]);
  __syncthreads();
  PasteGeom g;
  if (!paste_geom(boxes + d * 4, M, IH, IW, g)) return;
  const int cw = g.cx1 - g.cx0, ch = g.cy1 - g.cy0;
  int* out = STACK ? nullptr : seg + (long)img[d] * IH * IW;
  unsigned char* outb = STACK ? stack + (long)d * IH * IW : nullptr;
  for (int i = threadIdx.x; i < cw * ch; i += 256) {
    const int yy = g.cy0 + i / cw, xx = g.cx0 + i % cw;
    if (paste_value(pm, P, g, xx, yy) > thresh) {
      if (STACK) outb[(long)yy * IW + xx] = 1;
      else atomicAdd(out + (long)yy * IW + xx, 1);
    }
  }
}

// WORDS: the same paste written straight into the run-length codec's mask words (csrc/maskeval.hip: bit k = pixel
// (y = k % IH, x = k / IH), tail bits zero) -- what mmt_paste_mask_stack into a zeroed stack followed by mmt_mask_pack gives,
// without the bytes.  A thread owns one word and stores it, zero or not, so the caller clears nothing and no two threads meet.
// Most words lie in columns the box does not reach: a block of such words never fills the LDS.  The few words that do hold
// pixels of the clipped box are evaluated by their whole wave, one word at a time: lane = bit, one bilinear value per lane, and
// a ballot is the word (a thread that walked its own 64 bits would keep the 63 lanes beside it waiting).
__global__ __launch_bounds__(256) void paste_words_kernel(const float* __restrict__ prob, const float* __restrict__ boxes, int M,
                                                          int IH, int IW, long nw, float thresh,
                                                          unsigned long long* __restrict__ words) {
  extern __shared__ float pm[];  // (M+2)^2 padded probabilities
  const int d = blockIdx.y, P = M + 2;
  const long hw = (long)IH * IW;
  PasteGeom g;
  const bool some = paste_geom(boxes + d * 4, M, IH, IW, g);
  // columns [cx0, cx1) are positions [p0, p1) of the flattening; everything before and behind them is zero.  The block's words
  // cover positions [b0, b1) (block-uniform), a thread's word [kw, ke): compared as positions, so that the great majority of
  // threads, whose word is a plain zero, never divide
  const long p0 = (long)g.cx0 * IH, p1 = (long)g.cx1 * IH;
  const long b0 = blockIdx.x * 256L * 64, b1 = min(b0 + 256L * 64, hw);
  const bool hit = some && b0 < p1 && b1 > p0;
  const long j = blockIdx.x * 256L + threadIdx.x;
  const long kw = j * 64, ke = min(kw + 64, hw);
  unsigned long long w = 0;
  if (hit) {   // whole blocks, so every wave below is complete for its ballots and shuffles
    paste_fill<true>(pm, prob, d, M, 1, 0);
    __syncthreads();
    // does this thread's word hold a pixel of the clipped box?  Its first pixel is (x0, y0)
    int x0 = 0, y0 = 0;
    bool mine = false;
    if (kw < p1 && ke > p0) {   // (ke > p0 >= 0 leaves out the threads behind the last word)
      x0 = (int)((unsigned)kw / (unsigned)IH); y0 = (int)(kw - (long)x0 * IH);   // (kw < IH * IW < 2^31)
      int x = x0, y = y0;
      for (long k = kw; k < ke && x < g.cx1 && !mine;) {   // the word column by column: rows [y, y + len) of column x
        const int len = (int)min((long)(IH - y), ke - k);
        mine = x >= g.cx0 && max(y, g.cy0) < min(y + len, g.cy1);
        k += len; x++; y = 0;
      }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(mine);   // wave-uniform
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      // lane b is bit b of lane src's word: position kw_src + b = pixel (xx, yy)
      int xx = __shfl(x0, src, 64), yy = __shfl(y0, src, 64) + lane;
      if (yy >= IH) {
        if (IH >= 64) { yy -= IH; xx++; }   // (yy < IH + 64: one column further at the most)
        else { const int q = yy / IH; xx += q; yy -= q * IH; }
      }
      // (a position behind the last pixel has xx >= IW >= cx1: the tail bits stay zero)
      const bool in = xx >= g.cx0 && xx < g.cx1 && yy >= g.cy0 && yy < g.cy1;
      const unsigned long long bits = __ballot(in && paste_value(pm, P, g, xx, yy) > thresh);
      if (lane == src) w = bits;
    }
  }
  if (j < nw) words[(long)d * nw + j] = w;
}

extern "C" int mmt_paste_masks(const float* logits, const int32_t* labels, const float* boxes, const int32_t* img,
                               int D, int M, int NC, int IH, int IW, float thresh, int32_t* seg, void* stream) {
  if (D <= 0) return 0;
  const size_t lds = (size_t)(M + 2) * (M + 2) * sizeof(float);
  hipLaunchKernelGGL(paste_kernel<false>, dim3(D), dim3(256), lds, (hipStream_t)stream, logits, labels, boxes, img, M, NC, IH,
                     IW, thresh, seg, (unsigned char*)nullptr);
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmt_paste_mask_stack(const float* prob, const float* boxes, int D, int M, int IH, int IW, float thresh,
                                    uint8_t* stack, void* stream) {
  if (D <= 0) return 0;
  if (!prob || !boxes || !stack || M <= 0 || IH <= 0 || IW <= 0) return MMT_EINVAL;
  const size_t lds = (size_t)(M + 2) * (M + 2) * sizeof(float);
  hipLaunchKernelGGL(paste_kernel<true>, dim3(D), dim3(256), lds, (hipStream_t)stream, prob, (const int*)nullptr, boxes,
                     (const int*)nullptr, M, 1, IH, IW, thresh, (int*)nullptr, stack);
  MMT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmt_paste_mask_words(const float* prob, const float* boxes, int D, int M, int IH, int IW, float thresh,
                                    uint64_t* words, int32_t* rec, void* stream) {
  const long P = (long)M + 2;
  if (D < 0 || D > 65535 || M <= 0 || P * P * (long)sizeof(float) > 65536 || IH <= 0 || IW <= 0 ||
      (long)IH * (long)IW >= (1L << 31))
    return MMT_EINVAL;
  if (D == 0) return 0;
  if (!prob || !boxes || !words || !rec) return MMT_EINVAL;
  const long nw = ((long)IH * IW + 63) >> 6;
  hipLaunchKernelGGL(paste_words_kernel, dim3(mmt_cdiv(nw, 256), D), dim3(256), (size_t)(P * P) * sizeof(float),
                     (hipStream_t)stream, prob, boxes, M, IH, IW, nw, thresh, (unsigned long long*)words);
  MMT_LAUNCH_CHECK();
  return mmt_mask_records(words, D, IH, IW, rec, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ polygons
// rleFrPoly builds, from the x5-upsampled dense boundary walk, the sorted list of column crossings
// a_j = x*h + y and emits alternating run lengths; zero-length runs are folded.  That is exactly
//   mask[q] = (#{j : a_j <= q}) mod 2     (q = column-major pixel index)
// so the sort + run-length stage is replaced by a parity count over an (unsorted) crossing list kept
// in LDS.  One wave per ROI; lanes own polygon edges for the boundary walk and pixels for the fill.
//
// The list cannot fill.  Parity adds over any partition of the edges, so a polygon's edges are walked in passes of
// POLY_PASS = 64, one edge per lane, and every pass XORs its own parities into the polygon's.  Along one edge the walk's
// column u never turns back, and a crossing is recorded only where u steps over the centre of one of the M pixel
// columns: at most M per edge, 64 * M per pass -- 8 KB at the largest M the entry point takes (32).
#define POLY_PASS 64
#define POLY_MAX_M 32   // M * M <= 16 pixels per lane x 64 lanes

__global__ __launch_bounds__(64) void polygon_kernel(const float* __restrict__ xy, const int* __restrict__ poly_off,
                                                     const int* __restrict__ roi_poly, const float* __restrict__ boxes,
                                                     int M, float* __restrict__ out, int* __restrict__ overflow) {
  __shared__ unsigned cross[POLY_PASS * POLY_MAX_M];
  __shared__ int ncross;
  const int p = blockIdx.x, lane = threadIdx.x;
  const int h = M, w = M;
  const int cap = POLY_PASS * M;
  if (p == 0 && lane == 0 && overflow) *overflow = 0;   // kept in the ABI; nothing can overflow
  // crop + resize of structures/segmentation_mask.py:96-120 in float32, ratio cast like `tensor * python_float`
  const float b0 = boxes[p * 4 + 0], b1 = boxes[p * 4 + 1], b2 = boxes[p * 4 + 2], b3 = boxes[p * 4 + 3];
  float bw = b2 - b0, bh = b3 - b1;
  if (!(bw >= 1.f)) bw = 1.f;  // max(w, 1)
  if (!(bh >= 1.f)) bh = 1.f;
  const float rw = (float)((double)M / (double)bw), rh = (float)((double)M / (double)bh);
  const int npix = h * w;
  // accumulated mask (union over polygons): bit i of a lane is pixel q = lane + 64 * i (column-major), i < 16
  unsigned acc = 0;

  for (int pi = roi_poly[2 * p]; pi < roi_poly[2 * p + 1]; pi++) {
    const int v0 = poly_off[pi], k = poly_off[pi + 1] - v0;
    unsigned par = 0;   // this polygon's parities, pass by pass
    const double scale = 5;
    for (int j0 = 0; j0 < k; j0 += POLY_PASS) {
      if (lane == 0) ncross = 0;
      __syncthreads();
      const int j = j0 + lane;
      if (j < k) {
        const int j1 = (j + 1 == k) ? 0 : j + 1;
        const float fxs = (xy[(v0 + j) * 2 + 0] - b0) * rw, fys = (xy[(v0 + j) * 2 + 1] - b1) * rh;
        const float fxe = (xy[(v0 + j1) * 2 + 0] - b0) * rw, fye = (xy[(v0 + j1) * 2 + 1] - b1) * rh;
        int xs = (int)(scale * (double)fxs + .5), ys = (int)(scale * (double)fys + .5);
        int xe = (int)(scale * (double)fxe + .5), ye = (int)(scale * (double)fye + .5);
        const int dx = abs(xe - xs), dy = abs(ys - ye);
        const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
        if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
        const double s = dx >= dy ? (double)(ye - ys) / dx : (double)(xe - xs) / dy;
        const int n = (dx >= dy ? dx : dy);
        int pu = 0, pv = 0;
        for (int d = 0; d <= n; d++) {
          const int t = flip ? n - d : d;
          int u, v;
          if (dx >= dy) { u = t + xs; v = (int)(ys + s * t + .5); }
          else { v = t + ys; u = (int)(xs + s * t + .5); }
          if (d > 0 && u != pu) {
            double xd = (double)(u < pu ? u : u - 1);
            xd = (xd + .5) / scale - .5;
            if (!(floor(xd) != xd || xd < 0 || xd > w - 1)) {
              double yd = (double)(v < pv ? v : pv);
              yd = (yd + .5) / scale - .5;
              if (yd < 0) yd = 0; else if (yd > h) yd = h;
              yd = ceil(yd);
              const int slot = atomicAdd(&ncross, 1);
              if (slot < cap) cross[slot] = (unsigned)((int)xd * h + (int)yd);   // (always: see above)
            }
          }
          pu = u; pv = v;
        }
      }
      __syncthreads();
      const int nc = min(ncross, cap);
      for (int c = 0; c < nc; c++) {
        const unsigned a = cross[c];
#pragma unroll
        for (int i = 0; i < 16; i++) par ^= (a <= (unsigned)(lane + 64 * i) ? 1u : 0u) << i;
      }
      __syncthreads();
    }
    acc |= par;
  }
  for (int i = 0; i < 16; i++) {
    const int q = lane + 64 * i;
    if (q >= npix) break;
    const int x = q / h, y = q - x * h;
    out[((long)p * h + y) * w + x] = ((acc >> i) & 1u) ? 1.f : 0.f;
  }
}

extern "C" int mmt_polygon_targets(const float* poly_xy, const int32_t* poly_off, const int32_t* roi_poly,
                                   const float* boxes, int P, int M, float* out, int32_t* overflow, void* stream) {
  if (P <= 0) return 0;
  if (M < 1 || M > POLY_MAX_M) return MMT_EINVAL;
  hipLaunchKernelGGL(polygon_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, poly_xy, poly_off, roi_poly, boxes, M,
                     out, overflow);
  MMT_LAUNCH_CHECK();
  return 0;
}
