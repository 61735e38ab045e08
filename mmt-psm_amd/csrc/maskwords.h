// What the kernels over mask words share (csrc/maskeval.hip, csrc/masknms.hip): the layout of include/mmtpsm.h, "mask work of the
// PAP evaluator" -- bit k of a mask is pixel (y = k % H, x = k / H), ceil(H*W/64) words per mask, one integer record per mask.
#pragma once
#include "common.h"

typedef unsigned long long u64;

#define REC MMT_MASK_REC_INTS   // area, xmin, xmax, ymin, ymax, wrap, 0, 0

static inline bool bad_size(int H, int W) { return H <= 0 || W <= 0 || (long)H * (long)W >= (1L << 31); }
static inline long words_of(int H, int W) { return ((long)H * W + 63) >> 6; }

// the box of a record by rleToBbox's rule (pycoco/maskApi.c:135-151): an empty mask is [0, 0, 0, 0], a mask that wraps from the
// bottom of one column to the top of the next reports the full height
__device__ __forceinline__ void box_of(const int* __restrict__ r, int H, int& x, int& y, int& w, int& h) {
  if (r[0] == 0) { x = y = w = h = 0; return; }
  x = r[1]; w = r[2] - r[1] + 1;
  if (r[5]) { y = 0; h = H; } else { y = r[3]; h = r[4] - r[3] + 1; }
}
