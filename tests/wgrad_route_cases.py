"""The grid of weight-gradient calls whose routing tests/golden/wgrad_routes.npz pins (tests/test_wgrad_route.py; recorded by
tests/golden/gen_golden_wgrad_routes.py): the convolution shapes of the R-50-FPN detector at the benchmark's (1024) and the test size
(160) and the heads, and for every threshold of the decision code one case on each side of it.  A case is (N, Cin, H, W, Cout, k,
stride, pad).  Every case runs in the arithmetic modes 0-3, with x / dy stored as fp32 or bf16 (IOS), with both weight-gradient
switches on and each of them off singly.  BATCHES: lists of jobs for the grouped launch's plan, (case, planes?, maxima?, dw id, dbias id)."""
import itertools

from conv_route_cases import _backbone, _heads

MODES = (0, 1, 2, 3)
IO_X, IO_DY = 1, 16
IOS = (0, IO_X, IO_DY, IO_X | IO_DY)
SWITCHES = ("MMT_WGRAD_PLANES", "MMT_WGRAD_GROUP")
SWITCH_LEGS = (None,) + SWITCHES          # all on, then each off singly


def _thresholds():
    t = []

    def c(N, Cin, H, W, Cout, k, s=1, pad=None):
        t.append((N, Cin, H, W, Cout, k, s, (k - 1) // 2 if pad is None else pad))
    for Cout in (6, 8, 126, 128):                 # Cout % 4: 4-channel loads, the fp16 split
        c(2, 64, 16, 16, Cout, 1)
        c(2, 64, 16, 16, Cout, 3)
    for Cin, Cout in itertools.product((64, 128, 192, 256), repeat=2):   # Cin, Cout % 128: the plane-fed kernel's tiles
        c(1, Cin, 16, 32, Cout, 3)
    for W in (16, 32, 48, 64):                    # W % 32: its super-steps
        c(1, 128, 16, W, 128, 3)
        c(1, 128, 16, W, 128, 1)
    for H, W in itertools.product((4, 7, 8), (4, 7, 8, 9, 10, 12)):      # Ho, Wo below and at 8; Wo % 4: the pixel decode
        c(64, 64, H, W, 64, 1)
    c(4, 64, 26, 10, 64, 1)
    for M in (511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049):        # pixel ranges of >= 512 pixels
        c(1, 64, 1, M, 64, 1)
        c(1, 64, 1, M, 64, 3)
    for W in (32, 64, 96, 224, 256, 288, 480, 512, 544, 1024, 2048):     # T = N H W / 32 around 2, 8 and 16: the plane-fed ranges
        c(1, 128, 1, W, 128, 3)
        c(1, 128, 1, W, 128, 1)
        c(1, 256, 1, W, 256, 3)
    for Cin in (1920, 2048, 2176):                # plane-fed tiles 240 / 256 / 272 (one-tap form), 16 x 16 super-steps
        c(1, Cin, 16, 32, 2048, 1)
    for Cin in (3968, 4096, 4224):                # tiles 496 / 512 / 528: the resident slots
        c(2, Cin, 16, 32, 2048, 1)
    for Cin in (640, 768):                        # three-tap form: 3 Cin / 128 x Cout / 128 tiles
        c(2, Cin, 32, 32, 2048, 3)
    c(2, 256, 32, 32, 512, 1, 2, 0)               # stride 2
    c(2, 128, 32, 32, 128, 3, 2, 1)
    c(2, 128, 32, 32, 128, 3, 1, 0)               # not "same"-padded
    for k, pad in ((2, 0), (2, 1), (4, 1), (4, 2), (5, 2), (7, 3)):      # even kernels; the one-tap form's odd ones
        c(2, 128, 16, 32, 128, k, 1, pad)
    # the 2^29-element / 2^31-byte limits (shapes only): x, then dy, then both with Cout % 4 != 0; the argument block's own limit
    for H in (2047, 2048):
        c(1, 128, H, 2048, 128, 1)
        c(1, 128, H, 2048, 128, 3)
        c(1, 4, H, 2048, 128, 1)
        c(1, 128, H, 2048, 6, 1)
        c(1, 4, H, 2048, 6, 1)
    c(1, 512, 2048, 2048, 128, 1)
    c(1, 512, 2047, 2048, 128, 1)
    return t


def cases():
    seen, out = set(), []
    for c in _backbone(2, 1024, False) + _heads(1024, 400) + _backbone(2, 160, False) + _heads(512, 100) + _thresholds():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def grid():
    """every (mode, io_bf16, switch leg, case) in the order of the table's rows"""
    return itertools.product(MODES, IOS, range(len(SWITCH_LEGS)), cases())


def _aligned(n, k):
    return 0x10000 * k + 0x100 * n   # distinct, 256-byte aligned, never dereferenced


def fill(a, case, io=0, maxima=False):
    """the argument block of a case, into `a` (a ConvArgs); maxima: both operands carry their recorded maximum (the fp16 split)"""
    N, Cin, H, W, Cout, k, s, pad = case
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, Cin, Cout, k, k, s, pad
    a.Ho, a.Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    a.out_stride, a.mask_scale, a.io_bf16 = 1, 1.0, io
    a.x = _aligned(1, 1)
    if maxima:
        a.f16_x_amax, a.f16_dy_amax = _aligned(2, 1), _aligned(3, 1)
    return a


# ---- batches of jobs.  A job: (case, planes?, maxima?, dw id, dbias id or 0)
_PL3, _PL1, _PL5 = (2, 128, 16, 32, 128, 3, 1, 1), (2, 256, 16, 32, 128, 1, 1, 0), (2, 128, 16, 32, 128, 5, 1, 2)
_PLBIG = (2, 128, 64, 64, 128, 3, 1, 1)
_P2, _P1, _P0 = (2, 64, 32, 32, 64, 1, 1, 0), (4, 64, 26, 10, 64, 1, 1, 0), (64, 64, 4, 4, 64, 1, 1, 0)
_P2BIG = (2, 256, 64, 64, 256, 1, 1, 0)
_NOT4, _S2 = (2, 64, 16, 16, 6, 1, 1, 0), (2, 256, 32, 32, 512, 1, 2, 0)


def _mixed():
    return [(_P0, 0, 1), (_PL3, 1, 1), (_P1, 0, 1), (_P2, 0, 1), (_NOT4, 0, 1), (_P2BIG, 0, 1), (_PLBIG, 1, 1), (_P0, 0, 1), (_P1, 0, 1),
            (_P2, 0, 0), (_S2, 0, 1), (_PL1, 1, 1), (_PL3, 1, 0), (_PL5, 1, 1), (_S2, 1, 1)]


def batches():
    def ids(jobs, dbias=()):
        return [j + (i + 1, (i + 1) if i in dbias else 0) for i, j in enumerate(jobs)]
    out = {
        "shared_dw": [(_PL3, 1, 1, 1, 0), (_PL3, 1, 1, 1, 0), (_PLBIG, 1, 1, 2, 0), (_P2, 0, 1, 3, 0), (_P2BIG, 0, 1, 3, 0), (_P2, 0, 1, 4, 0)],
        "shared_dbias": [(_PLBIG, 1, 1, 1, 9), (_PL1, 1, 1, 2, 9), (_PL3, 1, 1, 3, 0)],
        "single_member": ids([(_PLBIG, 1, 1), (_P2, 0, 1), (_P2BIG, 0, 1), (_P1, 0, 1)]),
        "planes_13": ids([(_PLBIG if i % 3 == 0 else (_PL1 if i % 3 == 1 else _PL3), 1, 1) for i in range(13)], dbias=(0, 5)),
        "pipe_7": ids([(_P2BIG if i % 2 else _P2, 0, 1) for i in range(7)], dbias=(1,)),
        "mixed": ids(_mixed(), dbias=(2, 6)),
        "batch_96": ids([_mixed()[i % 15] for i in range(96)]),
        "one": ids([(_PLBIG, 1, 1)]),
        "empty": [],
    }
    return out


def batch_grid():
    """every (mode, switch leg, batch name) in the order of the table's rows"""
    return itertools.product(MODES, range(len(SWITCH_LEGS)), sorted(batches()))


def fill_jobs(WgradJob, specs):
    """the mmt_wgrad_job array of a batch"""
    arr = (WgradJob * max(len(specs), 1))()
    for j, (case, planes, maxima, dw, dbias) in zip(arr, specs):
        fill(j.a, case, 0, bool(maxima))
        j.dy, j.dw = _aligned(4, 1), _aligned(dw, 2)
        if dbias:
            j.dbias = _aligned(dbias, 3)
        if planes:
            j.x_planes, j.dy_planes, j.s_x, j.s_dy = _aligned(5, 1), _aligned(6, 1), _aligned(7, 1), _aligned(8, 1)
            j.x_plane_stride = j.dy_plane_stride = 1 << 24
    return arr
