"""The convolution grid: every cell of the routing code (csrc/conv_route.hip: route, wgrad_route) with the smallest shape that reaches it
and still hangs over its tile, every epilogue form the cell's shape predicate admits, and the fp64 references the GPU test
(tests/test_conv_grid_gpu.py) holds the kernels to element by element.  Plain Python and torch on the CPU: nothing here imports the
library; tests/test_conv_grid_cases.py asks the library's route whether every case reaches the cell it names.

THE CELLS are written by hand from conv_route.hip (CELLS, WCELLS below): a cell is what the launch switches on -- family, tile, K
ranges, K groups, strip width, the form of x, plane-fed tile height (forward); family, pixel decode, 4-channel loads, bf16 storage
bits, pixel ranges (weight gradient) -- in one arithmetic.  A cell lists its shape and the neighbouring cell one step below its threshold (`below`); admitted(cell)
gives the forms its predicate admits, edges(cell) the edges its shape exercises (the host test asserts both).

THE FORMS (FORMS): plain | affine_relu (scale, shift, ReLU) | res1 (same pixels) | res2 (the coarser map of the FPN top-down add,
parent pixel (h >> 1, w >> 1)) | res3 (the four finer pixels) | mask (mask > 0 ? v * mask_scale : 0) | mul | scatter (out_stride 2 into
a (2 Ho - 1) x (2 Wo - 1) destination, with a mask over the destination) | bf16_io (mode 1: x, res, mask and y stored as bf16) |
dgrad_mask, dgrad_res (the weight exists only as the packed planes of the flipped, row-scaled forward weight: layers.fused._dgrad).

THE INPUTS (operands, wgrad_operands): seeded randn, activations post-ReLU, weights randn / sqrt(K).  In every case the last image,
the first 16-channel slab of x and the last 32-channel block of the output channels are scaled down by 2^-6 (a power of two: nothing
else about the numbers changes): an error there is 64 times below the tensor's maximum, invisible to a max-norm, and as visible as any
other to the per-element magnitude B.

THE REFERENCE: conv_ref gives, per output element, the fp64 result with its epilogue and B = (|scale| sum |x||w| + |shift| + |res|)
times the mask and mul factors; wgrad_ref the same with B = |rowscale| sum |x||dy| (+ |dw| it accumulates into).  A kernel is held to
|y - ref| <= bound * max(B, 2^-126), bound = bound_of(arithmetic, K): TWICE the coefficient c(arithmetic, K) that
tests/test_conv_grid_cases.py derives by emulating the arithmetic on the grid's own inputs: the operands split as
tests/operand_prep_reference.py splits them (fp16 two-term, bf16 two- and three-term, plain bf16), the kept products (3 of the
two-term splits, 6 of the three-term split, 1 of plain bf16 and of fp32) added into ONE fp32 accumulator per output element, one
MFMA step of the reduction at a time (16 elements; fp32 operands: 2), the sum inside a step exact -- which is how every kernel of
the family accumulates.  The factor two covers another order of the steps, split-K partial sums included.  The project's own 3e-6
(tests/test_stem_gpu.py, tests/test_f16x2_gpu.py) is used instead wherever it is the tighter of the two.
(A first version let torch's fp32 CPU convolution stand in for the accumulator, one call per product: its blocked sums are three
times more accurate than any chain of MFMA steps at K = 576 ... 12544 (c = 9e-8 ... 2e-8 where the chain gives 2e-7 ... 4e-7), and
adding each product's sum separately hides that the small products are rounded at the size of the large one; every 3x3 and long-K
case then missed 2 c by factors of 1.1 to 2.5 on kernels that are right.  The chain is also the same on every machine.)

COEFF / WCOEFF, the derived tables -- c(arithmetic, K): the worst |emulated - fp64| / sum |x||w| over the emulated elements, rounded up
to two digits (the host test re-derives every entry and fails when its measurement is more than a quarter above or a half below the
table's).  Every entry is measured on 2048 or more output pixels (512 at K = 12544), whatever the cell's own size: at most 2048
pixels per image of a larger map, further images drawn the same way for a smaller one -- the worst of a few hundred elements says
little.  Measured (forward: K = KH KW Cin; weight gradient: "M", the N Ho Wo pixels summed over):

  arithmetic  products kept                     measured c
  fp32        1, fp32 operands                  K 64: 1.95e-7  216: 2.36e-7  280: 2.88e-7  576: 2.23e-7;  M 105: 1.87e-7  1104: 2.98e-7
  bf16        1 (mode 1; x, dy stored as bf16)  K 576: 1.66e-3  1152: 6.2e-4  2048: 3.7e-4;  M 1104: 8.3e-4
  bf16x2      3 of 4                            K 576: 3.03e-6;  M 1104: 1.92e-6
  bf16x3      6 of 9                            K 16: 2.30e-7  64: 2.88e-7  272: 2.59e-7  576: 4.48e-7  1152: 3.20e-7  2048: 2.35e-7  12544: 1.92e-7;
                                                M 105: 2.63e-7  540: 3.34e-7  1104: 2.63e-7
  f16x2       3 of 4, both tensors scaled by    K 16: 3.10e-7  128: 2.76e-7  256: 1.85e-7  272: 2.14e-7  288: 3.09e-7  576: 2.10e-7  1152: 2.52e-7
              the power of two of their maximum 2048: 1.63e-7  2160: 2.53e-7  12544: 1.52e-7;  M 105: 2.16e-7  256: 2.28e-7  512: 2.52e-7
                                                540: 1.81e-7  1104: 1.78e-7  1150: 2.04e-7
The same with the stand-in the issue named (one call of torch's fp32 CPU convolution / matmul per kept product, the sums added in
fp32), kept on record beside the chain's values -- the chain is 1 to 8 times larger, most at long K:
  fp32    K 64: 1.61e-7  216: 1.96e-7  280: 2.97e-7  576: 8.5e-8;  M 105: 2.73e-7  1104: 4.40e-7
  bf16    K 576: 1.25e-3  1152: 6.6e-4  2048: 3.7e-4;  M 1104: 8.3e-4
  bf16x2  K 576: 2.20e-6;  M 1104: 1.90e-6
  bf16x3  K 16: 2.25e-7  64: 2.35e-7  272: 2.21e-7  576: 8.9e-8  1152: 8.9e-8  2048: 3.7e-8  12544: 2.3e-8;  M 105: 2.57e-7  540: 2.84e-7  1104: 6.16e-7
  f16x2   K 16: 2.97e-7  128: 2.61e-7  256: 3.45e-7  272: 2.95e-7  288: 3.21e-7  576: 1.01e-7  1152: 8.5e-8  2048: 5.0e-8  2160: 5.1e-8
          12544: 2.4e-8;  M 105: 3.46e-7  256: 2.53e-7  512: 3.23e-7  540: 3.58e-7  1104: 4.61e-7  1150: 4.20e-7
(the 1x1 cells, K 16 ... 280, go through a matmul and agree with the chain; the 3x3 and long-K cells go through a blocked convolution.)
(c hardly moves with K: with products of random sign the chain's rounding errors and sum |x||w| both grow like K.)
Which cases need more than the project's 3e-6: the one-term bf16 cases (mode 1, bf16-stored x / dy: the operands' rounding alone is
2^-9 each) and the two-term bf16 split at K = 576 (c = 3.03e-6, from the dropped x1 w1 product and the second terms' rounding:
held to 2 c = 6.2e-6; at M = 1104 its c is 1.9e-6 and 3e-6 is used).  Every fp32, bf16x3 and f16x2 case is held to 2 c, which is
below 1e-6 throughout.  K = 12544 (the fc shape) needs no more than the others: 1.5e-7 and 1.9e-7.
"""
import math

import torch
import torch.nn.functional as F

TINY = 2.0 ** -126
DOWN = 2.0 ** -6
PROJECT_BOUND = 3e-6

# include/mmtpsm.h: MMT_ROUTE_*, MMT_X_*, MMT_WGRAD_*
FP32, SPLIT, DMA, DMA_BF16X, ROWS, STRIP, PG, C64 = 1, 2, 3, 4, 5, 6, 7, 8
X_AS_IS, X_BF16_PLANES, X_F16_PLANES = 0, 1, 2
WG_FP32_FAST, WG_FP32_SLOW, WG_SPLIT, WG_PIPE, WG_PIPE_F16, WG_PLANES_1, WG_PLANES_3 = 1, 2, 3, 4, 5, 6, 7

FORMS = ("plain", "affine_relu", "res1", "res2", "res3", "mask", "mul", "scatter", "bf16_io", "dgrad_mask", "dgrad_res")
TILED_FORMS = ("plain", "affine_relu", "res1", "res2", "res3", "mask", "mul", "scatter")   # the tiled kernels' staged epilogue takes all
DGRAD = ("dgrad_mask", "dgrad_res")
ROUTE_FIELDS = ("family", "tag", "bm", "bn", "ksplit", "kgroups", "strip_tw", "x_form", "pg_rows")
WROUTE_FIELDS = ("family", "terms", "decode", "vec4", "bf", "splits")


def _cell(entry, mode, shape, route, x_bf16=False, below=None, panels=None, no_planes=False, note=""):
    """entry: "lib" (mmt_conv_forward's dispatch in `mode`) or "f16" (the two-term fp16 split, mode 3); shape: (N, Cin, H, W, Cout, k,
    stride, pad); route: ROUTE_FIELDS; below: (shape one step under the cell's threshold, the cell it lands on)"""
    return dict(entry=entry, mode=mode, shape=shape, route=dict(zip(ROUTE_FIELDS, route)), x_bf16=x_bf16, below=below,
                panels=panels, no_planes=no_planes, note=note)


# ---- forward and data gradient.  Shapes: M = N Ho Wo; "t128" = ceil(M / 128) ceil(Cout / 128) as in pick_variant
_S33 = (2, 64, 10, 12, 72, 3, 1, 1)         # M = 240 = 3 * 64 + 48, Cout = 64 + 8; image 0 ends at pixel 119, inside the second 64-row tile
_V1 = (2, 272, 46, 178, 136, 1, 1, 0)       # M = 16376: 128 row tiles x 2 column tiles = 256 = t128min; K = 272 > 256; M % 128 = 120
_V3 = (2, 272, 90, 90, 136, 1, 1, 0)        # M = 16200: 127 x 2 = 254 < 256 tiles of 128 x 128, 127 x 3 = 381 of 128 x 64
_KS = (2, 2048, 10, 12, 136, 1, 1, 0)       # K = 2048 = 128 steps, 4 tiles: 4 ranges of 32 steps
_FC = (70, 12544, 1, 1, 136, 1, 1, 0)       # the fc shape: 784 steps over 16 ranges; every "image" is one row
_ROWS_G = (2, 64, 34, 488, 68, 1, 1, 0)     # M = 33184 >= 128 * 256: 260 row blocks -> 2 column groups of 2 and 1 panels
_ROWS_A = (2, 64, 34, 968, 68, 1, 1, 0)     # M = 65824: 515 >= 512 row blocks, all 3 panels in one block
_ROWS_F = (2, 128, 34, 32, 68, 1, 1, 0)     # M = 2176 >= 128 * 16 (fp16 split): 17 row blocks, one panel per block
_ROWS_FA = (2, 256, 34, 968, 68, 1, 1, 0)   # K = 256: the fp16 split only
_ST128 = (2, 128, 128, 128, 136, 3, 1, 1)   # 2 * 64 * 2 = 256 strip tiles (the fp32 tensors' minimum), Cout = 128 + 8
_ST64 = (2, 128, 256, 64, 136, 3, 1, 1)     # Wo % 128 != 0: 4 rows x 64
_STK128 = (2, 128, 32, 128, 128, 3, 1, 1)   # bf16 x: 32 tiles (the minimum) -> 4 K ranges of 3 tap pairs; Cout % 128 == 0 is demanded
_STK64 = (2, 128, 64, 64, 128, 3, 1, 1)
_PG64 = (2, 32, 9, 13, 136, 3, 1, 1)        # M = 234 = 3 * 64 + 42
_PG64K = (2, 240, 9, 13, 136, 3, 1, 1)      # K = 2160 = 135 steps: 2 ranges of >= 64
_PG128 = (2, 32, 77, 93, 136, 3, 1, 1)      # M = 14322: 112 x 2 = 224 tiles of 128 rows
_PG256 = (2, 32, 147, 195, 136, 3, 1, 1)    # M = 57330: 224 x 2 = 448 tiles of 256 rows
_STRIP_FORMS = ("plain", "affine_relu", "res1", "res2", "res3", "mask")
_PG_FORMS = ("plain", "affine_relu", "res1", "mask")

CELLS = {
    # the fp32-input MFMA kernel: whatever the mode where Cin % 16 != 0 or Cout <= 32 (variant 0, 128 x 32), and mode 0
    "fp32_cin24": _cell("lib", 3, (2, 24, 6, 8, 40, 3, 1, 1), (FP32, 2, 64, 64, 1, 1, 0, 0, 0)),
    "fp32_v0": _cell("lib", 3, (2, 64, 10, 12, 12, 1, 1, 0), (FP32, 0, 128, 32, 1, 1, 0, 0, 0)),
    "fp32_v1": _cell("lib", 3, (2, 280, 46, 178, 136, 1, 1, 0), (FP32, 1, 128, 128, 1, 1, 0, 0, 0)),
    "fp32_v3": _cell("lib", 3, (2, 280, 90, 90, 136, 1, 1, 0), (FP32, 3, 128, 64, 1, 1, 0, 0, 0)),
    "fp32_mode0": _cell("lib", 0, _S33, (FP32, 2, 64, 64, 1, 1, 0, 0, 0)),
    # operands split in registers: a split mode without packed weight planes.  The binding always packs them, so no call of the product
    # reaches this cell; the GPU test launches it through the library's C entry point
    "split_m3": _cell("lib", 3, _S33, (SPLIT, 2, 64, 64, 1, 1, 0, 0, 0), no_planes=True),
    "split_m2": _cell("lib", 2, _S33, (SPLIT, 2, 64, 64, 1, 1, 0, 0, 0), no_planes=True),
    "split_m1": _cell("lib", 1, _S33, (SPLIT, 2, 64, 64, 1, 1, 0, 0, 0), no_planes=True),
    # the tiled DMA-fed kernels on the bf16 splits (the library's dispatch)
    "dma_v2_m3": _cell("lib", 3, _S33, (DMA, 2, 64, 64, 1, 1, 0, 0, 0)),
    "dma_v2_m2": _cell("lib", 2, _S33, (DMA, 2, 64, 64, 1, 1, 0, 0, 0)),
    "dma_v2_m1": _cell("lib", 1, _S33, (DMA, 2, 64, 64, 1, 1, 0, 0, 0)),
    "dma_k16": _cell("lib", 3, (2, 16, 10, 12, 72, 1, 1, 0), (DMA, 2, 64, 64, 1, 1, 0, 0, 0)),   # K: ONE 16-channel step
    "dma_1x1map": _cell("lib", 3, (3, 64, 1, 1, 72, 3, 1, 1), (DMA, 2, 64, 64, 1, 1, 0, 0, 0)),     # a 1 x 1 map under a 3x3
    "dma_v1_m3": _cell("lib", 3, _V1, (DMA, 1, 128, 128, 1, 1, 0, 0, 0), below=(_V3, "dma_v3_m3")),
    "dma_v3_m3": _cell("lib", 3, _V3, (DMA, 3, 128, 64, 1, 1, 0, 0, 0)),
    "dma_ksplit_m3": _cell("lib", 3, _KS, (DMA, 1, 128, 128, 4, 1, 0, 0, 0),
                           below=((2, 2032, 10, 12, 136, 1, 1, 0), "dma_v2_m3")),
    "dma_fc_m3": _cell("lib", 3, _FC, (DMA, 1, 128, 128, 16, 1, 0, 0, 0)),
    # x stored as bf16 (mode 1): its own plane
    "dma_bf16x": _cell("lib", 1, _S33, (DMA_BF16X, 2, 64, 64, 1, 1, 0, 0, 0), x_bf16=True),
    "dma_bf16x_ksplit": _cell("lib", 1, _KS, (DMA_BF16X, 1, 128, 128, 4, 1, 0, 0, 0), x_bf16=True),
    # the row-resident 1x1 kernel, bf16 split: K = 64 / 128, >= 128 * 256 rows, res_mode <= 1 and no mask
    "rows_groups_m3": _cell("lib", 3, _ROWS_G, (ROWS, 2, 128, 32, 1, 1, 0, 0, 0), panels=2,
                            below=((2, 64, 34, 480, 68, 1, 1, 0), "dma_v2_m3")),
    "rows_all_m3": _cell("lib", 3, _ROWS_A, (ROWS, 3, 128, 32, 1, 1, 0, 0, 0), panels=3),
    # the tap-strip kernel on three bf16 planes of x (mode 3 without the fp16 split) and on bf16-stored x (mode 1)
    "strip128_m3": _cell("lib", 3, _ST128, (STRIP, 4, 256, 128, 1, 1, 128, X_BF16_PLANES, 0),
                         below=((2, 128, 126, 128, 136, 3, 1, 1), "dma_v1_m3")),
    "strip64_m3": _cell("lib", 3, _ST64, (STRIP, 4, 256, 128, 1, 1, 64, X_BF16_PLANES, 0)),
    "strip128_bf16x": _cell("lib", 1, _ST128, (STRIP, 4, 256, 128, 1, 1, 128, X_AS_IS, 0), x_bf16=True),
    "strip64_bf16x": _cell("lib", 1, _ST64, (STRIP, 4, 256, 128, 1, 1, 64, X_AS_IS, 0), x_bf16=True),
    "strip128_ksplit": _cell("lib", 1, _STK128, (STRIP, 4, 256, 128, 4, 1, 128, X_AS_IS, 0),
                             x_bf16=True, below=((2, 128, 30, 128, 128, 3, 1, 1), "dma_bf16x")),
    "strip64_ksplit": _cell("lib", 1, _STK64, (STRIP, 4, 256, 128, 4, 1, 64, X_AS_IS, 0), x_bf16=True),
    # ---- the two-term fp16 split (the default arithmetic)
    "f16_dma_v2": _cell("f16", 3, _S33, (DMA, 2, 64, 64, 1, 1, 0, 0, 0)),
    "f16_dma_k16": _cell("f16", 3, (2, 16, 10, 12, 72, 1, 1, 0), (DMA, 2, 64, 64, 1, 1, 0, 0, 0)),
    "f16_dma_v1": _cell("f16", 3, _V1, (DMA, 1, 128, 128, 1, 1, 0, 0, 0),
                        below=(_V3, "f16_dma_v3")),
    "f16_dma_v3": _cell("f16", 3, _V3, (DMA, 3, 128, 64, 1, 1, 0, 0, 0)),
    "f16_dma_ksplit": _cell("f16", 3, _KS, (DMA, 1, 128, 128, 4, 1, 0, 0, 0)),
    "f16_dma_fc": _cell("f16", 3, _FC, (DMA, 1, 128, 128, 16, 1, 0, 0, 0)),
    "f16_rows_groups": _cell("f16", 3, _ROWS_F, (ROWS, 2, 128, 32, 1, 1, 0, 0, 0),
                             panels=1, below=((2, 128, 31, 33, 68, 1, 1, 0), "f16_dma_v2")),
    "f16_rows_all": _cell("f16", 3, _ROWS_FA, (ROWS, 3, 128, 32, 1, 1, 0, 0, 0), panels=3),
    "f16_c64": _cell("f16", 3, (2, 64, 10, 12, 64, 3, 1, 1), (C64, 2, 0, 0, 1, 1, 0, 0, 0)),
    "f16_strip128": _cell("f16", 3, _ST128, (STRIP, 4, 256, 128, 1, 1, 128, X_F16_PLANES, 0),
                          below=((2, 128, 126, 128, 136, 3, 1, 1), "f16_pg128")),
    "f16_strip64": _cell("f16", 3, _ST64, (STRIP, 4, 256, 128, 1, 1, 64, X_F16_PLANES, 0),
                         below=((2, 128, 252, 64, 136, 3, 1, 1), "f16_pg128")),
    "f16_pg64": _cell("f16", 3, _PG64, (PG, 5, 64, 128, 1, 4, 0, X_F16_PLANES, 64)),
    "f16_pg64_ksplit": _cell("f16", 3, _PG64K, (PG, 5, 64, 128, 2, 4, 0, X_F16_PLANES, 64)),
    "f16_pg128": _cell("f16", 3, _PG128, (PG, 5, 128, 128, 1, 2, 0, X_F16_PLANES, 128),
                       below=((2, 32, 77, 92, 136, 3, 1, 1), "f16_pg64")),
    "f16_pg256": _cell("f16", 3, _PG256, (PG, 5, 256, 128, 1, 1, 0, X_F16_PLANES, 256),
                       below=((2, 32, 147, 194, 136, 3, 1, 1), "f16_pg128")),
}

def admitted(cell):
    """the epilogue forms the cell's shape predicate admits, written from conv_route.hip and the launchers (tests/test_conv_grid_cases.py
    asks the route the same question form by form and compares).  Every admitted form has a numeric case (cases()).
      fp32, split          the staged epilogue takes every operand; no planes-only weight (a data gradient there materialises the
                           flipped weight and is a plain call), no bf16-stored x
      tiled DMA-fed        everything, on either arithmetic; bf16 storage where x is stored as bf16 (mode 1)
      row-resident         res_mode <= 2 (2: Wo % 8 == 0), no mul, no scatter; on the bf16 splits res_mode <= 1 and no mask
      patch kernel         the plain affine (+ ReLU) epilogue, fp32 weight in the block
      tap-strip            no scatter; the fp16 split hands `mul` to the tiled kernel, the library's dispatch keeps it
      plane-fed            res_mode <= 1, no mul, no scatter
    res2 needs a map with a parent pixel for every pixel (even Ho, Wo): the 1 x 1 maps (fc rows, the 1x1-map cell) have none"""
    c = CELLS[cell]
    fam, f16 = c["route"]["family"], c["entry"] == "f16"
    if fam in (FP32, SPLIT):
        forms = TILED_FORMS
    elif fam == DMA:
        forms = TILED_FORMS + DGRAD
    elif fam == DMA_BF16X:
        forms = TILED_FORMS + DGRAD + ("bf16_io",)
    elif fam == ROWS:
        forms = ("plain", "affine_relu", "res1", "res2", "mask") + DGRAD if f16 else ("plain", "affine_relu", "res1", "dgrad_res")
    elif fam == C64:
        forms = ("plain", "affine_relu")
    elif fam == STRIP:
        forms = _STRIP_FORMS + DGRAD + (() if f16 else ("mul",)) + (("bf16_io",) if c["x_bf16"] else ())
    else:
        forms = _PG_FORMS + DGRAD
    Ho, Wo = out_hw(c["shape"])
    if Ho % 2 or Wo % 2:
        forms = tuple(f for f in forms if f != "res2")
    return forms


def arithmetic(cell):
    c = CELLS[cell]
    if c["route"]["family"] == FP32:
        return "fp32"
    return "f16x2" if c["entry"] == "f16" else ("fp32", "bf16", "bf16x2", "bf16x3")[c["mode"]]


def out_hw(shape):
    N, Cin, H, W, Cout, k, s, p = shape
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def cases():
    """[(cell, form)] in a fixed order, the cell's forms together (the GPU test keeps one cell's products at a time)"""
    return [(c, f) for c in CELLS for f in admitted(c)]


def edges(cell):
    """the edges a cell's shape exercises, as data"""
    c = CELLS[cell]
    N, Cin, H, W, Cout, k, s, p = c["shape"]
    Ho, Wo = out_hw(c["shape"])
    M, r = N * Ho * Wo, c["route"]
    bm, bn = (r["bm"], r["bn"]) if r["family"] != C64 else (0, 0)
    e = {"M": M, "K": k * k * Cin, "m_overhang": M % bm if bm else None, "n_overhang": Cout % bn if bn else None}
    # a tile that starts in one image and ends in the next / starts in one image row and ends in another (row-major pixels)
    e["tile_crosses_image"] = bool(bm) and N >= 2 and (Ho * Wo) % bm != 0
    e["last_tile_spans_rows"] = bool(bm) and ((M - 1) // bm * bm) // Wo != (M - 1) // Wo
    e["single_k_step"] = k * k * Cin == 16
    e["map_1x1"] = (H, W) == (1, 1) and k == 3
    return e


# ------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


def scale_down(x, w):
    """the last image, the first 16-channel slab of x and the last 32-channel block of w's output channels times 2^-6, in place"""
    x[-1] *= DOWN
    x[:, :16] *= DOWN
    w[-(((w.shape[0] - 1) % 32) + 1):] *= DOWN


def operands(cell, form):
    """the tensors of a case on the CPU, NCHW-shaped fp32 (bf16 where the form stores them so): dict with x, w (the weight the launch
    multiplies with: for a dgrad form the flipped, row-scaled data-gradient weight; `w_fwd`, `rowscale`: what layers.fused._dgrad is
    given), scale, shift, relu, res, res_mode, mask, mask_scale, mul, out_stride, out_hw"""
    c = CELLS[cell]
    N, Cin, H, W, Cout, k, s, p = c["shape"]
    Ho, Wo = out_hw(c["shape"])
    g = _gen(repr(c["shape"]))                 # (cells of one shape share x and w: one set of fp64 products serves them)
    x = torch.randn(N, Cin, H, W, generator=g).relu()
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    if form in DGRAD:
        x = torch.randn(N, Cin, H, W, generator=g) * 1e-2            # a gradient: both signs, small
    scale_down(x, w)
    o = dict(x=x, w=w, scale=None, shift=None, relu=False, res=None, res_mode=0, mask=None, mask_scale=1.0, mul=None, out_stride=1,
             out_hw=None, y_dtype=torch.float32)
    g = _gen(cell + "/" + form)
    if form in DGRAD:
        g = _gen(cell + "/dgrad")                                     # (one row scale for both dgrad forms of a cell: they share the products)
        # forward layer: Cout channels -> Cin channels, weight (Cin, Cout, k, k), row scale per forward output channel (= this conv's input)
        o["rowscale"] = torch.rand(Cin, generator=g) + 0.5
        o["w_fwd"] = w.flip(2, 3).transpose(0, 1).contiguous()        # so that the flipped, transposed forward weight is w ...
        o["w"] = (o["w_fwd"] * o["rowscale"].view(-1, 1, 1, 1)).flip(2, 3).transpose(0, 1).contiguous()   # ... times the scale, rounded once
        g = _gen(cell + "/" + form)
    if form == "affine_relu":
        o["scale"], o["shift"], o["relu"] = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1, True
    elif form in ("res1", "dgrad_res", "bf16_io"):
        o["res"], o["res_mode"] = torch.randn(N, Cout, Ho, Wo, generator=g) * (1e-2 if form == "dgrad_res" else 1.0), 1   # (a gradient's size)
    elif form == "res2":
        o["res"], o["res_mode"] = torch.randn(N, Cout, Ho >> 1, Wo >> 1, generator=g), 2
    elif form == "res3":
        o["res"], o["res_mode"] = torch.randn(N, Cout, 2 * Ho, 2 * Wo, generator=g), 3
    elif form == "mul":
        o["mul"], o["relu"] = torch.rand(N, Cout, Ho, Wo, generator=g), True
    elif form == "scatter":
        o["out_stride"], o["out_hw"] = 2, (2 * Ho - 1, 2 * Wo - 1)
    if form in ("mask", "dgrad_mask", "bf16_io", "scatter"):
        oh, ow = o["out_hw"] or (Ho, Wo)
        o["mask"], o["mask_scale"] = torch.randn(N, Cout, oh, ow, generator=g), 1.5
    if c["x_bf16"]:
        o["x"] = o["x"].bfloat16()
    if form == "bf16_io":
        o["res"], o["mask"], o["y_dtype"] = o["res"].bfloat16(), o["mask"].bfloat16(), torch.bfloat16
    return o


# ------------------------------------------------------------------------------------------ references
def products(x, w, stride, pad):
    """fp64 sum x w and sum |x||w| per output element, (N, Cout, Ho, Wo)"""
    xd, wd = x.double(), w.double()
    return F.conv2d(xd, wd, None, stride, pad), F.conv2d(xd.abs(), wd.abs(), None, stride, pad)


def products_unfold(x, w, stride, pad):
    """the same as fp64 unfold + matmul (runs on whatever device x and w are on)"""
    xd, wd = x.double(), w.double()
    N, Cout = x.shape[0], w.shape[0]
    Ho, Wo = out_hw((N, x.shape[1], x.shape[2], x.shape[3], Cout, w.shape[2], stride, pad))
    cols = F.unfold(xd, w.shape[2:], padding=pad, stride=stride)           # (N, Cin k k, Ho Wo)
    wm = wd.reshape(Cout, -1)
    return ((wm @ cols).reshape(N, Cout, Ho, Wo), (wm.abs() @ cols.abs()).reshape(N, Cout, Ho, Wo))


def conv_ref(x, w, o, stride, pad, prod=None):
    """-> (ref, B) fp64, shaped like the destination.  o: operands(); prod: products(x, w) if the caller kept them"""
    acc, mag = prod if prod is not None else products(x, w, stride, pad)
    one = lambda t: t.double().view(1, -1, 1, 1)   # noqa: E731
    v, B = acc, mag
    if o["scale"] is not None:
        v, B = v * one(o["scale"]), B * one(o["scale"]).abs()
    if o["shift"] is not None:
        v, B = v + one(o["shift"]), B + one(o["shift"]).abs()
    if o["res_mode"] == 1:
        r = o["res"].double()
    elif o["res_mode"] == 2:
        r = F.interpolate(o["res"].double(), scale_factor=2, mode="nearest")
    elif o["res_mode"] == 3:
        r = None
    if o["res_mode"] in (1, 2):
        v, B = v + r, B + r.abs()
    elif o["res_mode"] == 3:
        f = o["res"].double()
        v, B = v + F.avg_pool2d(f, 2) * 4, B + F.avg_pool2d(f.abs(), 2) * 4
    if o["relu"]:
        v = v.clamp_min(0)
    if o["out_stride"] > 1:
        oh, ow = o["out_hw"]
        vs, Bs = v.new_zeros(v.shape[0], v.shape[1], oh, ow), v.new_zeros(v.shape[0], v.shape[1], oh, ow)
        vs[:, :, ::o["out_stride"], ::o["out_stride"]], Bs[:, :, ::o["out_stride"], ::o["out_stride"]] = v, B
        v, B = vs, Bs
    if o["mask"] is not None:
        keep = (o["mask"].double() > 0).double() * o["mask_scale"]
        v, B = v * keep, B * keep
    if o["mul"] is not None:
        v, B = v * o["mul"].double(), B * o["mul"].double().abs()
    return v, B


# ------------------------------------------------------------------------------------------ the weight gradient
def _wcell(mode, have, shape, route, x_bf16=False, dy_bf16=False, note=""):
    """have: "" | "maxima" | "planes" (maxima and row-blocked planes of both operands); route: WROUTE_FIELDS"""
    return dict(mode=mode, have=have, shape=shape, route=dict(zip(WROUTE_FIELDS, route)), x_bf16=x_bf16, dy_bf16=dy_bf16, note=note)


_W1 = (2, 20, 23, 24, 36, 3, 1, 1)     # M = 1104: three pixel ranges of 384; Cin % 16 != 0, Cout % 32 != 0; Wo % 4 == 0 (decode 2)
_W1D1 = (2, 20, 23, 25, 36, 3, 1, 1)   # Wo % 4 != 0 (decode 1), M = 1150
_W1D0 = (3, 20, 5, 7, 36, 3, 1, 1)     # maps under 8 x 8 (decode 0), M = 105: one range
_WPL = (1, 128, 16, 32, 128)           # the plane-fed kernel's smallest layer with two pixel ranges
WCELLS = {
    "planes_3": _wcell(3, "planes", _WPL + (3, 1, 1), (WG_PLANES_3, 2, 0, 0, 0, 2)),
    "planes_1": _wcell(3, "planes", _WPL + (1, 1, 0), (WG_PLANES_1, 2, 0, 0, 0, 2)),
    "planes_3_one_range": _wcell(3, "planes", (1, 128, 8, 32, 128, 3, 1, 1), (WG_PLANES_3, 2, 0, 0, 0, 1)),
    "planes_3_two_images": _wcell(3, "planes", (2, 128, 8, 32, 128, 3, 1, 1), (WG_PLANES_3, 2, 0, 0, 0, 2)),   # ranges and halo rows across an image boundary
    "f16_decode2": _wcell(3, "maxima", _W1, (WG_PIPE_F16, 2, 2, 1, 0, 3)),
    "f16_decode1": _wcell(3, "maxima", _W1D1, (WG_PIPE_F16, 2, 1, 1, 0, 3)),
    "f16_decode0": _wcell(3, "maxima", _W1D0, (WG_PIPE_F16, 2, 0, 1, 0, 1)),
    "f16_rect": _wcell(3, "maxima", (2, 20, 9, 30, 36, 3, 1, 1), (WG_PIPE_F16, 2, 1, 1, 0, 2)),   # Ho = 9 against Wo = 30: a decode that swaps them lands elsewhere
    "pipe_m3": _wcell(3, "", _W1, (WG_PIPE, 3, 2, 1, 0, 3)),
    "pipe_m2": _wcell(2, "", _W1, (WG_PIPE, 2, 2, 1, 0, 3)),
    "pipe_m1": _wcell(1, "", _W1, (WG_PIPE, 1, 2, 1, 0, 3)),
    "pipe_m3_decode1": _wcell(3, "", (2, 20, 9, 30, 36, 3, 1, 1), (WG_PIPE, 3, 1, 1, 0, 2)),
    "pipe_m3_decode0": _wcell(3, "", _W1D0, (WG_PIPE, 3, 0, 1, 0, 1)),
    "pipe_vec4_off": _wcell(3, "", (2, 20, 23, 24, 38, 3, 1, 1), (WG_PIPE, 3, 2, 0, 0, 3)),
    "pipe_bf_x": _wcell(1, "", _W1, (WG_PIPE, 1, 2, 1, 1, 3), x_bf16=True),
    "pipe_bf_dy": _wcell(1, "", _W1, (WG_PIPE, 1, 2, 1, 2, 3), dy_bf16=True),
    "pipe_bf_x_dy": _wcell(1, "", _W1, (WG_PIPE, 1, 2, 1, 3, 3), x_bf16=True, dy_bf16=True),
    "fp32_fast": _wcell(0, "", _W1, (WG_FP32_FAST, 0, 2, 1, 0, 3)),
    "fp32_slow": _wcell(0, "", _W1D0, (WG_FP32_SLOW, 0, 0, 1, 0, 1)),
    "fp32_slow_vec4_off": _wcell(0, "", (2, 20, 23, 24, 38, 3, 1, 1), (WG_FP32_SLOW, 0, 2, 0, 0, 3)),
    # the register-splitting kernel takes operands of 2^31 bytes and more only: its route is pinned, no launch
    "split_beyond": _wcell(2, "", (1, 128, 2048, 2048, 128, 1, 1, 0), (WG_SPLIT, 2, 2, 1, 0, 512), note="route only"),
}
WNOT_RUN = {"split_beyond": "an operand of 2^31 bytes: tests/test_wgrad_route.py pins the route as well; no numeric case at a test's size"}


def warithmetic(cell):
    c = WCELLS[cell]
    if c["have"]:
        return "f16x2"
    if c["x_bf16"] or c["dy_bf16"]:
        return "bf16"
    return ("fp32", "bf16", "bf16x2", "bf16x3")[c["mode"]]


def edges_w(cell):
    c = WCELLS[cell]
    Ho, Wo = out_hw(c["shape"])
    return {"M": c["shape"][0] * Ho * Wo, "K": c["shape"][5] ** 2 * c["shape"][1]}


def wgrad_operands(cell):
    c = WCELLS[cell]
    N, Cin, H, W, Cout, k, s, p = c["shape"]
    Ho, Wo = out_hw(c["shape"])
    g = _gen("wgrad/" + cell)
    x = torch.randn(N, Cin, H, W, generator=g).relu()
    dy = torch.randn(N, Cout, Ho, Wo, generator=g) * 1e-2
    x[-1] *= DOWN                       # the last image (both operands: its pixels' products are 2^-12 of the others')
    dy[-1] *= DOWN
    x[:, :4] *= DOWN                    # a channel slab of x and a block of dy's channels: rows and columns of dw 64 times below the rest
    dy[:, -(((Cout - 1) % 32) + 1):] *= DOWN
    o = dict(x=x, dy=dy, rowscale=torch.rand(Cout, generator=g) + 0.5, dw0=torch.randn(Cout, Cin, k, k, generator=g) * 1e-3)
    if c["x_bf16"]:
        o["x"] = x.bfloat16()
    if c["dy_bf16"]:
        o["dy"] = dy.bfloat16()
    return o


def wgrad_ref(x, dy, rowscale, shape):
    """-> (dw, B, dbias, Bbias) fp64: dw = rowscale * sum x dy, B = |rowscale| sum |x||dy|; dbias = column sums of dy, bounded by sum |dy|"""
    N, Cin, H, W, Cout, k, s, p = shape
    xd, dd = x.double(), dy.double()
    rs = rowscale.double().view(-1, 1, 1, 1)
    dw = torch.nn.grad.conv2d_weight(xd, (Cout, Cin, k, k), dd, stride=s, padding=p) * rs
    B = torch.nn.grad.conv2d_weight(xd.abs(), (Cout, Cin, k, k), dd.abs(), stride=s, padding=p) * rs.abs()
    return dw, B, dd.sum((0, 2, 3)), dd.abs().sum((0, 2, 3))


# ------------------------------------------------------------------------------------------ the coefficients
# c(arithmetic, reduction length): derived by tests/test_conv_grid_cases.py (module docstring).  Forward: K = KH KW Cin; weight
# gradient: the pixels N Ho Wo.  Values: the measured emulation error rounded up to two digits
COEFF = {
    ("bf16", 576): 0.0017, ("bf16", 1152): 0.00063, ("bf16", 2048): 0.00038,
    ("bf16x2", 576): 3.1e-06,
    ("bf16x3", 16): 2.4e-07, ("bf16x3", 64): 2.9e-07, ("bf16x3", 272): 2.6e-07, ("bf16x3", 576): 4.5e-07, ("bf16x3", 1152): 3.2e-07, ("bf16x3", 2048): 2.4e-07, ("bf16x3", 12544): 2e-07,
    ("f16x2", 16): 3.2e-07, ("f16x2", 128): 2.8e-07, ("f16x2", 256): 1.9e-07, ("f16x2", 272): 2.2e-07, ("f16x2", 288): 3.1e-07, ("f16x2", 576): 2.2e-07, ("f16x2", 1152): 2.6e-07, ("f16x2", 2048): 1.7e-07, ("f16x2", 2160): 2.6e-07, ("f16x2", 12544): 1.6e-07,
    ("fp32", 64): 2e-07, ("fp32", 216): 2.4e-07, ("fp32", 280): 2.9e-07, ("fp32", 576): 2.3e-07,
}
WCOEFF = {
    ("bf16", 1104): 0.00084,
    ("bf16x2", 1104): 2e-06,
    ("bf16x3", 105): 2.7e-07, ("bf16x3", 540): 3.4e-07, ("bf16x3", 1104): 2.7e-07,
    ("f16x2", 105): 2.2e-07, ("f16x2", 256): 2.3e-07, ("f16x2", 512): 2.6e-07, ("f16x2", 540): 1.9e-07, ("f16x2", 1104): 1.8e-07, ("f16x2", 1150): 2.1e-07,
    ("fp32", 105): 1.9e-07, ("fp32", 1104): 3e-07,
}


def bound_of(arith, K):
    """what a kernel is held to, as a multiple of B: twice the derived coefficient, or the project's 3e-6 where that is the tighter"""
    return min(2.0 * COEFF[(arith, K)], PROJECT_BOUND) if COEFF[(arith, K)] <= PROJECT_BOUND else 2.0 * COEFF[(arith, K)]


def wbound_of(arith, M):
    c = WCOEFF[(arith, M)]
    return min(2.0 * c, PROJECT_BOUND) if c <= PROJECT_BOUND else 2.0 * c
