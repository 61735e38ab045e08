"""CIAM_Module.forward with the reference's normalisations (reference modeling/relation/mask_relation_module.py:199-242:
MODEL.RELATION_MASK.NORM 1 "sum channel", 2 "L2 norm", anything else none; PRE_NORM) as plain torch arithmetic, group by
group -- what the reference computes when it calls the module once per (image, class) slice.  Dtype follows the input (the tests
use float64 as the expected value and float32 on the CPU as the measure of an input's conditioning).  Pinned to the reference's own
module by tests/golden/ciam_norm.npz (tests/test_ciam_formulation.py).

Each normalisation's gradient term can be cut (`detach`), which is how the tests show that their inputs make every term visible:
  "instance_norm"   the 1 / ||x[i]|| factor of PRE_NORM
  "channel_weight"  w[c] of NORM 1 (the sum over the group and the quotient by the maximum)
  "l2_factor"       F[i][j] of NORM 2

Also the input builders shared by the CIAM tests."""
import torch

COMBOS = [(-1, False), (-1, True), (1, False), (1, True), (2, False), (2, True)]      # (NORM, PRE_NORM); the first is the default
VARIANTS = COMBOS[1:]
TERMS = ("instance_norm", "channel_weight", "l2_factor")
EPS = 1e-10
FWD_BAR, GRAD_BAR = 2e-5, 2e-4     # the project's bars for this module (tests/test_relation_kernels_gpu.py), of a tensor's largest magnitude


def terms_of(norm, pre_norm):
    """the gradient terms a combination has.  The instance norm under NORM 2 is left out: E / F does not change when an instance is
    rescaled, so that term is zero up to the 1e-10 in the denominator"""
    t = []
    if pre_norm and norm != 2:
        t.append("instance_norm")
    if norm == 1:
        t.append("channel_weight")
    if norm == 2:
        t.append("l2_factor")
    return t


def ciam_slice(gamma, x, norm, pre_norm, detach=()):
    """one (image, class) slice: x (n, C, H, W) -> gamma * attention(x) + x"""
    n, C, H, W = x.shape
    if pre_norm:
        nf = torch.norm(x.reshape(n, -1), 2, -1)
        if "instance_norm" in detach:
            nf = nf.detach()
        f = x / nf[:, None, None, None]
    else:
        f = x
    cw = f.permute(1, 0, 2, 3).reshape(C, n, -1)
    energy = torch.bmm(cw, cw.permute(0, 2, 1))
    if norm == 1:
        w = torch.abs(torch.sum(energy.reshape(C, -1), dim=1))
        w = w / torch.max(w)
        if "channel_weight" in detach:
            w = w.detach()
        ne = energy * w[:, None, None]
    elif norm == 2:
        fac = torch.sqrt(torch.sum(energy ** 2, dim=0))
        if "l2_factor" in detach:
            fac = fac.detach()
        ne = energy / (fac[None] + EPS)
    else:
        ne = energy
    ne = torch.max(ne, -1, keepdim=True)[0] - ne
    att = torch.softmax(torch.mean(ne, 0), dim=-1)
    out = torch.mm(att, x.reshape(n, -1)).view(n, C, H, W)
    return gamma * out + x


def ciam(gamma, x, sizes, norm, pre_norm, detach=()):
    """all slices of a batch: `sizes` = the lengths of the contiguous groups"""
    parts, st = [], 0
    for s in sizes:
        parts.append(ciam_slice(gamma, x[st:st + s], norm, pre_norm, detach))
        st += s
    assert st == x.shape[0]
    return torch.cat(parts)


def evaluate(x, gamma, gout, sizes, norm, pre_norm, detach=(), dtype=torch.float64):
    """-> (out - x, dx - dout, dgamma) in `dtype` on the CPU: the attention parts the tests compare (the identity path is exactly
    x forward and dout backward, several times larger, and would hide an error in them)"""
    xx = x.detach().to("cpu", dtype).requires_grad_(True)
    gg = torch.tensor(float(gamma), dtype=dtype, requires_grad=True)
    go = gout.detach().to("cpu", dtype)
    out = ciam(gg, xx, sizes, norm, pre_norm, detach)
    out.backward(go)
    return (out - xx).detach(), (xx.grad - go).detach(), gg.grad.detach().reshape(1)


def rel_dev(a, b):
    """largest deviation of a from b, relative to b's largest magnitude"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def sample_index(numel, k):
    """the fixed sample of a tensor's flat index range that tests/golden/ciam_norm.npz stores for slice k"""
    g = torch.Generator().manual_seed(4242 + k)
    return torch.randperm(numel, generator=g)[:1024].sort().values


# ---------------------------------------------------------------- inputs
GAMMA = 0.7
LAYOUTS = [([5, 1, 37, 70], 14), ([128], 14), ([1, 1, 1], 14), ([200, 56], 14), ([5, 9], 7)]     # (group sizes, H = W)


def group_ids(sizes):
    return torch.cat([torch.full((s,), 3 * i + 1, dtype=torch.int64) for i, s in enumerate(sizes)])


def gaussian_inputs(sizes, hw, seed, C=16):
    """ReLU'd Gaussian features at scale 0.3, as in tests/test_relation_kernels_gpu.py::test_ciam_vs_oracle"""
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    x = torch.relu(torch.randn(n, C, hw, hw, generator=g) * 0.3 + 0.1)
    gout = torch.randn(n, C, hw, hw, generator=g)
    return x, gout


def structured_inputs(sizes, hw, seed, C=16):
    """instances built from two shared spatial templates with random non-negative mixing weights, channel scales spread over 1.5
    decades and instance scales over one: instances that differ in norm and channels that differ in weight, so that the
    normalisations' own gradient terms are a visible part of dx (the Gaussian inputs above are nearly equal in both).  The output
    gradient has a part in the span of the same templates (three times the white part), which makes <dOut[i], x[j]> -- what drives
    the gradient through the softmax and the energies -- a sizeable share of the attention part of dx next to the mix term"""
    g = torch.Generator().manual_seed(seed)
    n, K = sum(sizes), 2
    tmpl = torch.relu(torch.randn(K, hw * hw, generator=g) + 0.3)
    mix = torch.rand(n, C, K, generator=g) ** 2
    x = torch.einsum("nck,kp->ncp", mix, tmpl) + 0.05 * torch.relu(torch.randn(n, C, hw * hw, generator=g))
    cs = 10.0 ** (-1.5 * torch.rand(C, generator=g))
    cs[0] = 1.0
    isc = 10.0 ** (torch.rand(n, generator=g) - 0.5)
    x = (x * cs[None, :, None] * isc[:, None, None]).view(n, C, hw, hw) * 0.1
    gm = torch.randn(n, C, K, generator=g)
    gout = 3.0 * torch.einsum("nck,kp->ncp", gm, tmpl).view(n, C, hw, hw) + torch.randn(n, C, hw, hw, generator=g)
    return x.contiguous(), gout


def inputs_for(norm, pre_norm, sizes, hw):
    """the input of a (combination, layout) case: the structured ones for every combination (tests/test_ciam_formulation.py holds
    them to the visibility and the conditioning condition; the Gaussian ones fail the first under PRE_NORM)"""
    return structured_inputs(sizes, hw, 1000 * len(sizes) + sizes[0] + hw)
