"""The attention block's fused projection front end (csrc/attn_proj.hip) on the GPU at BigGAN-128's two block shapes (discriminator 64x64x96 -> 16/16/48,
generator 64x64x192 -> 24/24/96; theta / phi carry their zero padding rows), with ReLU on load, with a zero-padded k tail and a partial last wave stride.
Kernel level: tests/attn_proj_checks.py (forward bit for bit against the five launches it replaces, data gradient against fp64). Network level: the
BigGAN-128 generator / discriminator pair at full width and a small batch, SG_ATTN_PROJ=1 against SG_ATTN_PROJ=0."""
import os

import pytest
import torch

import attn_proj_checks as AP
from util import Collector

pytestmark = pytest.mark.gpu

FWD_CASES = [AP.D_SHAPE, AP.G_SHAPE, AP.RELU_SHAPE, AP.TAIL_SHAPE]


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_equals_separate_launches(sg, case):
    AP.forward_case(case, torch.device("cuda:0"))


@pytest.mark.parametrize("case", [AP.D_SHAPE, AP.G_SHAPE, AP.TAIL_SHAPE])
@pytest.mark.parametrize("with_res", [True, False])
def test_data_gradient_matches_fp64(sg, case, with_res):
    AP.bwd_data_case(case, torch.device("cuda:0"), with_res)


def test_predicate_rejects_other_shapes(sg):
    lib = sg.lib()
    for B, H, C, Dp, Cg in AP.REJECTED:
        assert lib.sg_attn_proj_ok(B, H, H, C, C, Dp, Cg) == 0
    assert lib.sg_attn_proj_ok(2, 64, 64, 96, 96, 16, 48) == 1 and lib.sg_attn_proj_ok(2, 64, 64, 192, 192, 24, 96) == 1


class _MODEL:
    info_type = "N/A"


def _networks(dev):
    from studiogan_amd import ops
    from studiogan_amd.backbones import big_resnet
    MOD = ops.Modules(apply_g_sn=True, apply_d_sn=True, g_cond_mtd="cBN", backbone="big_resnet")
    torch.manual_seed(5)
    G = big_resnet.Generator(120, 128, 128, 96, True, [4], "cBN", 1000, "ortho", "N/A", True, MOD, _MODEL).to(dev)
    D = big_resnet.Discriminator(128, 96, True, True, [1], "PD", "W/O", "N/A", False, 1000, "ortho", "N/A", True, MOD, _MODEL).to(dev)
    with torch.no_grad():      # sigma = 0 at initialisation would switch the attention branch off
        for net in (G, D):
            for m in net.modules():
                if isinstance(m, ops.SelfAttention):
                    m.sigma.fill_(0.7)
    return G, D


def test_network_gradients_match_separate_launches(sg):
    """D(G(z)) at full width, batch 4: the fused front end is used by both attention blocks (the 1x1 data-gradient launches of the blocks disappear), images and
    logits are bit-identical to the separate launches' (the forward is), every gradient agrees to the bf16 rounding of the partial sums the chained launches made."""
    dev = torch.device("cuda:0")
    G, D = _networks(dev)
    sd = ({k: v.clone() for k, v in G.state_dict().items()}, {k: v.clone() for k, v in D.state_dict().items()})
    g = torch.Generator().manual_seed(9)
    z, lab = torch.randn((4, 120), generator=g), torch.randint(0, 1000, (4,), generator=g)
    got, fused_calls = {}, {}
    keep = os.environ.get("SG_ATTN_PROJ")
    try:
        for mode in ("0", "1"):
            os.environ["SG_ATTN_PROJ"] = mode
            n = [0]
            G.load_state_dict(sd[0]); D.load_state_dict(sd[1])      # same power-iteration and batch-norm state for both passes
            G.train(); D.train()
            for p in list(G.parameters()) + list(D.parameters()):
                p.grad = None
            zd = z.to(dev).requires_grad_(True)
            img = G(zd, lab.to(dev))
            out = D(img, lab.to(dev))["adv_output"]
            n[0] = sum(1 for fn in _walk(out.grad_fn) if type(fn).__name__ == "AttnProjFnBackward")
            out.sum().backward()
            torch.cuda.synchronize()
            fused_calls[mode] = n[0]
            got[mode] = {"img": img.detach().float().cpu(), "out": out.detach().float().cpu(), "dz": zd.grad.float().cpu(),
                         **{"G." + k: p.grad.float().cpu() for k, p in G.named_parameters() if p.grad is not None},
                         **{"D." + k: p.grad.float().cpu() for k, p in D.named_parameters() if p.grad is not None}}
    finally:
        if keep is None:
            os.environ.pop("SG_ATTN_PROJ", None)
        else:
            os.environ["SG_ATTN_PROJ"] = keep
    assert fused_calls == {"0": 0, "1": 2}, fused_calls
    assert torch.equal(got["0"]["img"], got["1"]["img"]) and torch.equal(got["0"]["out"], got["1"]["out"])
    assert set(got["0"]) == set(got["1"])
    C = Collector()
    for k in got["0"]:
        # (a generator block's convolution biases feed a batch norm: their gradient is analytically zero, what is left is rounding noise of either path)
        if k not in ("img", "out") and not (k.startswith("G.blocks.") and k.endswith(".bias") and ".conv2d" in k):
            C.check("fused vs separate: " + k, got["1"][k], got["0"][k], 2e-2, l2=True)
    C.finish()


def _walk(fn, seen=None):
    seen = set() if seen is None else seen
    stack = [fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        yield f
        stack.extend(nf for nf, _ in f.next_functions)
