"""Checks of the attention block's fused projection front end (csrc/attn_proj.hip), written once for both executors: tests/test_attn_proj_gpu.py runs them on
the GPU, tests/test_attn_proj_cpu.py on the CPU interpreter (hipemu.fullemu.Installed). The reference of the forward is the path the kernel replaces (three
sg_conv2d_fwd launches through the small-K streaming kernel + two sg_maxpool2_fwd launches): bit for bit. The reference of the data gradient is fp64 torch."""
import os

import torch

from util import check

# (B, H, C, Dp, Cg, relu): the discriminator's and the generator's block of BigGAN-128 at ch 96 (12 theta / phi channels padded to 16), a k tail, ReLU on load
D_SHAPE = (2, 64, 96, 16, 48, False)
G_SHAPE = (1, 64, 192, 24, 96, False)
RELU_SHAPE = (2, 16, 96, 16, 48, True)
TAIL_SHAPE = (3, 8, 72, 16, 48, False)       # C = 72: zero-padded k tail; J = 192: a partial last wave stride
TINY_SHAPES = [(1, 8, 96, 16, 48, False), (1, 4, 192, 24, 96, True), (3, 4, 72, 16, 48, False)]
REJECTED = [(2, 16, 96, 16, 64), (2, 16, 256, 32, 128), (2, 12, 96, 16, 48), (2, 16, 100, 16, 48)]      # (B, H, C, Dp, Cg)


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def inputs(case, dev):
    B, H, C, Dp, Cg, relu = case
    x = _rnd((B, H, H, C), 11).to(dev)
    ws = [_rnd((Dp, C), 12, 0.1).to(dev), _rnd((Dp, C), 13, 0.1).to(dev), _rnd((Cg, C), 14, 0.1).to(dev)]
    return x, ws


def run_fwd(case, x, ws):
    from studiogan_amd import _lib as L
    B, H, C, Dp, Cg, relu = case
    HW4 = (H // 2) ** 2
    dev = x.device
    theta = torch.full((B, H, H, Dp), float("nan"), dtype=torch.bfloat16, device=dev)
    phi = torch.full((B, HW4, Dp), float("nan"), dtype=torch.bfloat16, device=dev)
    g = torch.full((B, HW4, Cg), float("nan"), dtype=torch.bfloat16, device=dev)
    iphi = torch.full((B, HW4, Dp), 255, dtype=torch.uint8, device=dev)
    ig = torch.full((B, HW4, Cg), 255, dtype=torch.uint8, device=dev)
    assert L.lib().sg_attn_proj_ok(B, H, H, C, C, Dp, Cg) == 1
    L.call("sg_attn_proj_fwd", L.ptr(x), C, L.ptr(ws[0]), L.ptr(ws[1]), L.ptr(ws[2]), L.ptr(theta), L.ptr(phi), L.ptr(g), L.ptr(iphi), L.ptr(ig),
           B, H, H, C, Dp, Cg, 1 if relu else 0, L.stream())
    return theta, phi, g, iphi, ig


def run_fwd_separate(case, x, ws):
    """the five launches the fused kernel replaces (the 1x1 launches forced onto the small-K streaming kernel whatever the problem size)"""
    from studiogan_amd import functional as F, _lib as L
    B, H, C, Dp, Cg, relu = case
    os.environ["SG_CONV_SK"] = "force"
    try:
        full = [F.conv2d_raw(x, w.data_ptr(), C, w.shape[0], 1, 1, pix_flags=L.PIX_RELU if relu else 0) for w in ws]
    finally:
        os.environ.pop("SG_CONV_SK", None)
    outs = [full[0]]
    idxs = []
    for t in full[1:]:
        Cc = t.shape[3]
        y = torch.empty((B, (H // 2) ** 2, Cc), dtype=t.dtype, device=t.device)
        idx = torch.empty((B, (H // 2) ** 2, Cc), dtype=torch.uint8, device=t.device)
        L.call("sg_maxpool2_fwd", L.dt(t), L.ptr(t), Cc, L.ptr(y), Cc, L.ptr(idx), B, H, H, Cc, L.stream())
        outs.append(y)
        idxs.append(idx)
    return outs[0], outs[1], outs[2], idxs[0], idxs[1]


def _bits(t):
    return t.cpu().view(torch.int16) if t.dtype == torch.bfloat16 else t.cpu()


def forward_case(case, dev):
    """theta, pooled phi / g and both argmax planes equal the separate launches' bit for bit; two runs give the same bits"""
    x, ws = inputs(case, dev)
    new = run_fwd(case, x, ws)
    old = run_fwd_separate(case, x, ws)
    for name, a, b in zip(("theta", "phi", "g", "idx_phi", "idx_g"), new, old):
        assert torch.equal(_bits(a), _bits(b)), f"{name} differs from the separate launches {case}"
    again = run_fwd(case, x, ws)
    for a, b in zip(new, again):
        assert torch.equal(_bits(a), _bits(b))
    return new


def unpool_ref(dy, idx, B, H):
    """fp64 [B,H,H,C]: the pooled gradient at each window's argmax position, zero elsewhere"""
    Cc = dy.shape[-1]
    dy = dy.double().cpu().reshape(B, H // 2, H // 2, Cc)
    idx = idx.cpu().reshape(B, H // 2, H // 2, Cc).long()
    full = torch.zeros((B, H, H, Cc), dtype=torch.float64)
    for pos in range(4):
        full[:, pos >> 1::2, pos & 1::2, :] = dy * (idx == pos)
    return full


def bwd_data_case(case, dev, with_res=True):
    """dx against fp64: res + dtheta W_theta + unpool(dphi) W_phi + unpool(dg) W_g (tolerance of the 1x1 layers in tests/test_conv_v2_gpu.py)"""
    from studiogan_amd import _lib as L
    B, H, C, Dp, Cg, relu = case
    x, ws = inputs(case, dev)
    _, _, _, iphi, ig = run_fwd(case, x, ws)
    HW4 = (H // 2) ** 2
    dtheta, dphi, dg = _rnd((B, H, H, Dp), 21).to(dev), _rnd((B, HW4, Dp), 22).to(dev), _rnd((B, HW4, Cg), 23).to(dev)
    res = _rnd((B, H, H, C), 24).to(dev) if with_res else None
    wd = [w.t().contiguous() for w in ws]      # data-gradient images [C][rows]
    outs = []
    for _ in range(2):
        dx = torch.full((B, H, H, C), float("nan"), dtype=torch.bfloat16, device=dev)
        L.call("sg_attn_proj_bwd_data", L.ptr(dtheta), L.ptr(dphi), L.ptr(dg), L.ptr(iphi), L.ptr(ig), L.ptr(wd[0]), L.ptr(wd[1]), L.ptr(wd[2]), L.ptr(res),
               L.ptr(dx), B, H, H, C, Dp, Cg, L.stream())
        outs.append(dx.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two runs differ"
    w64 = [w.double().cpu() for w in ws]
    ref = dtheta.double().cpu() @ w64[0] + unpool_ref(dphi, iphi, B, H) @ w64[1] + unpool_ref(dg, ig, B, H) @ w64[2]
    if with_res:
        ref = ref + res.double().cpu()
    check(f"attn proj dx {case} res={with_res}", outs[0].float(), ref, 4e-3)
