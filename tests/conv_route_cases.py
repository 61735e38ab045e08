"""The grid of convolution calls whose routing tests/golden/conv_routes.npz pins (tests/test_conv_route.py; recorded by
tests/golden/gen_golden_conv_routes.py): every convolution shape of the R-50-FPN and ResNeXt detectors at the benchmark's (1024) and the
test size (160), forward and data-gradient forms, the fc layers as 1x1, and for every threshold of the decision code one case just below
and one at it.  A case is (N, Cin, H, W, Cout, k, stride, pad, out_stride, dgrad, epi); `dgrad`: the weight exists only as packed planes;
`epi` (the launch filling only): 0 plain, 1 residual of the same pixels, 2 the coarser map of the FPN top-down add, 3 mask, 4 mul.
Every case runs in the arithmetic modes 0-3, with fp32 and with bf16-stored x, with all six forward switches on and each of them off
singly, in three fillings of the argument block (FILLINGS)."""
import itertools

MODES = (0, 1, 2, 3)
SWITCHES = ("MMT_SPLITK", "MMT_STRIP", "MMT_ROWS", "MMT_PG", "MMT_C64", "MMT_DIRECT_EPI")   # bit i of mmt_conv_switches()
SWITCH_LEGS = (None,) + SWITCHES          # all on, then each off singly
FILLINGS = ("shape", "kind", "launch")    # the shape alone / as _hip._conv_kind sees the block / every operand of the launch there
IO_X = 1
PLACEHOLDER = 0x10   # what the callers of the legacy queries put where a pointer had to be non-null


def _backbone(N, S, resnext):
    """(N, Cin, H, W, Cout, k, stride, pad) of the body, the FPN and the RPN head over an S x S batch"""
    out = [(N, 3, S, S, 64, 7, 2, 3)]
    h, cin = S // 4, 64
    for stage, (mid, cout, blocks) in enumerate(((64, 256, 3), (128, 512, 4), (256, 1024, 6), (512, 2048, 3))):
        if resnext:
            mid *= 4   # 32 groups x 8 channels per group at layer1, doubling per stage
        for b in range(blocks):
            s = 2 if (b == 0 and stage > 0) else 1
            ho = h // s
            if resnext:   # the stride sits in the (grouped) 3x3, which has kernels of its own
                out += [(N, cin, h, h, mid, 1, 1, 0), (N, mid, ho, ho, cout, 1, 1, 0)]
            else:
                out += [(N, cin, h, h, mid, 1, s, 0), (N, mid, ho, ho, mid, 3, 1, 1), (N, mid, ho, ho, cout, 1, 1, 0)]
            if b == 0:
                out.append((N, cin, h, h, cout, 1, s, 0))
            h, cin = ho, cout
    for lvl, c in enumerate((256, 512, 1024, 2048)):
        hl = S // (4 << lvl)
        out += [(N, c, hl, hl, 256, 1, 1, 0), (N, 256, hl, hl, 256, 3, 1, 1)]
    for lvl in range(5):
        hl = max(S // (4 << lvl), 1)
        out += [(N, 256, hl, hl, 256, 3, 1, 1), (N, 256, hl, hl, 3, 1, 1, 0), (N, 256, hl, hl, 12, 1, 1, 0)]
    return out


def _heads(R, Rm):
    """the box head's fc layers as 1x1 over R rows, the mask head over Rm regions (the deconvolution as its four strided taps)"""
    return [(R, 12544, 1, 1, 1024, 1, 1, 0), (R, 1024, 1, 1, 1024, 1, 1, 0), (R, 1024, 1, 1, 81, 1, 1, 0), (R, 1024, 1, 1, 324, 1, 1, 0),
            (Rm, 256, 14, 14, 256, 3, 1, 1), (Rm, 256, 28, 28, 81, 1, 1, 0)]


def _dgrad(c):
    """the data-gradient call of a forward shape: channels swapped over the output's pixels, stride 1, planes-only weight; a strided 1x1
    scatters through out_stride.  None: not a form of this family (strided 3x3 / 7x7)"""
    N, Cin, H, W, Cout, k, s, pad = c
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    if s == 1:
        return (N, Cout, Ho, Wo, Cin, k, 1, k - 1 - pad, 1, 1, 0)
    if k == 1:
        return (N, Cout, Ho, Wo, Cin, 1, 1, 0, s, 1, 0)
    return None


def _thresholds():
    t = []

    def c(N, Cin, H, W, Cout, k, epi=0):
        t.append((N, Cin, H, W, Cout, k, 1, k // 2, 1, 0, epi))
    for tiles in (255, 256):             # 128 x 128 tiles that fill the chip: the tile variant
        c(1, 512, tiles, 128, 128, 1)
        c(1, 512, tiles, 128, 256, 1)
    for tiles in (511, 512):             # ... and the K split of the 128 x 128 kernel
        c(1, 2048, tiles, 128, 128, 1)
    for H in (62, 64, 510, 512):         # tap-strip tiles 31 / 32 (bf16 x: K ranges) and 255 / 256
        c(1, 128, H, 128, 128, 3)
        c(1, 256, H, 128, 128, 3)
    for Cout in (32, 33, 64, 95, 96, 128):
        c(2, 128, 64, 64, Cout, 3)
        c(2, 128, 128, 128, Cout, 3)
        c(2, 64, 64, 64, Cout, 1)
        c(2, 64, 64, 64, Cout, 3)
    for Cin in (256, 272, 2032, 2048):   # K: the low-K tile rule, the shortest sum that is split
        c(1, Cin, 64, 128, 128, 1)
        c(1, Cin, 64, 128, 256, 1)
    for M in (128 * 16 - 1, 128 * 16, 128 * 256 - 1, 128 * 256):   # rows of the row-resident 1x1 kernel
        for Cin, Cout in ((64, 64), (64, 256), (128, 512), (256, 1024), (512, 128)):
            for epi in (0, 1, 3):
                c(1, Cin, 1, M, Cout, 1, epi)
    for epi in (2, 4):
        c(2, 64, 64, 64, 256, 1, epi)
        c(2, 64, 62, 62, 256, 1, epi)
    for H, W in ((128, 128), (128, 64), (128, 192), (128, 96), (126, 128), (127, 128), (130, 64), (132, 64)):   # Wo % 64, % 128; Ho
        c(2, 256, H, W, 256, 3)
    for epi in (1, 2, 3, 4):
        c(2, 256, 128, 128, 256, 3, epi)     # a tap-strip shape
        c(2, 256, 64, 64, 256, 3, epi)       # a plane-fed shape
    for W in (256 * 447, 256 * 448, 128 * 223, 128 * 224, 64 * 128, 64 * 129):   # plane-fed tile counts 448, 224, 128 (one image row)
        c(1, 256, 1, W, 128, 3)
    return t


def cases():
    seen, out = set(), []

    def add(c):
        if c is not None and c not in seen:
            seen.add(c)
            out.append(c)
    fwd = []
    for S, Ns, R, Rm in ((1024, (2, 4), 1024, 400), (160, (2,), 512, 100)):
        for N in Ns:
            for rx in (False, True):
                fwd += _backbone(N, S, rx)
        fwd += _heads(R, Rm)
    for c in fwd:
        add(c + (1, 0, 0))
        add(_dgrad(c))
    for c in fwd:                     # the mask head's deconvolution: four 1x1 taps into every other pixel
        if c[1:4] == (256, 14, 14) and c[5] == 3:
            add((c[0], 256, 14, 14, 256, 1, 1, 0, 2, 0, 0))
    for c in _thresholds():
        add(c)
    return out


def grid():
    """every (mode, bf16 x?, switch leg, case, filling) in the order of the table's rows"""
    return itertools.product(MODES, (0, 1), range(len(SWITCH_LEGS)), cases(), FILLINGS)


def _aligned(n, k):
    return 0x10000 * k + 0x100 * n   # distinct, 256-byte aligned, never dereferenced


def fill(ConvArgs, case, io_x, filling, placeholders):
    """the argument block of a case.  `placeholders` (the legacy queries only): the shape filling carries placeholder pointers for x
    and the weight planes, as its callers wrote it; without them the shape filling is the bare shape and the caller states the promise
    (mmt_conv_route's `assume`)"""
    N, Cin, H, W, Cout, k, s, pad, out_stride, dgrad, epi = case
    a = ConvArgs()
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, Cin, Cout, k, k, s, pad
    a.Ho, a.Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    a.out_stride, a.mask_scale = out_stride, 1.0
    if out_stride > 1:
        a.out_H, a.out_W = a.Ho * out_stride, a.Wo * out_stride
    a.io_bf16 = IO_X if io_x else 0
    if filling == "shape":
        if placeholders:
            a.x = a.w_planes = PLACEHOLDER
        return a
    a.x, a.y = _aligned(1, 1), _aligned(2, 1)
    a.w_planes, a.w_plane_stride = _aligned(3, 1), 8 * ((Cout * k * k * Cin + 7) // 8)
    if not dgrad:
        a.w = _aligned(4, 1)
    if filling == "kind":
        return a
    a.scale, a.shift, a.relu = _aligned(5, 1), _aligned(6, 1), 1
    a.y_amax, a.y_amax_stats, a.f16_guard_x = _aligned(7, 1), 1, _aligned(8, 1)
    if dgrad:
        a.w_src = _aligned(9, 1)
    if not io_x:
        a.x_planes, a.x_plane_stride = _aligned(10, 1), 8 * ((N * H * W * Cin + 7) // 8)
    if epi in (1, 2):
        a.res, a.res_mode = _aligned(11, 1), epi
    elif epi == 3:
        a.mask = _aligned(12, 1)
    elif epi == 4:
        a.mul = _aligned(13, 1)
    return a
