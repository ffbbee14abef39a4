"""Outputs of the modulated convolution (csrc/modconv.hip through style_ops/modulated_conv2d.py) across two builds of the library, bit for bit.

    SG_LIBSGAMD=<other build> python tools/modconv_fold_check.py --save ref.pt
    python tools/modconv_fold_check.py --against ref.pt

Runs every case of MODCONV_CASES (tests/stylegan2_pl_checks.py) on its seeded inputs in fp32 and bf16, and cases g and d once more with the post_gain the
tests give them: the forward y, the first-order dx, ds, dw (and dnoise where the case has noise), then under second_order(generator=True) the four gradients
of <vx, dx> + <vs, ds> (d_gy, d_x, d_s, d_w) on the fused and on the composition route of the tangent. --against asserts torch.equal on every tensor and
that none is all zero."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

GAINS = {"g": 0.75, "d": 1.5}      # tests/test_stylegan2_pl_gpu.py test_modconv_second_order_with_post_gain


def run_case(tag, dtype, gain, dev):
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops import modulated_conv2d as MC
    import modconv_ref as R
    import stylegan2_pl_checks as K
    index = K.MODCONV_CASES.index(tag)
    N, C, Cout, H, k, up, demod, noise, flip = K.OP_CASES[tag]
    x, w, s, nz, gy = R.exact_inputs(6100 + index, N, C, Cout, H, k, up, None if gain is not None else noise)
    vx, vs = K.grid(6200 + index, *x.shape).to(dev, dtype), K.grid(6300 + index, *s.shape).to(dev, torch.float32)
    xd = x.to(dev, dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd, sd = w.to(dev, torch.float32).requires_grad_(True), s.to(dev, torch.float32).requires_grad_(True)
    nd = None if nz is None else nz.to(dev, torch.float32).requires_grad_(True)
    gyd = gy.to(dev, dtype).requires_grad_(True)
    if gain is None:
        y = MC.modulated_conv2d(xd, wd, sd, noise=nd, up=up, padding=k // 2, resample_filter=R.low_pass().to(dev), demodulate=demod, flip_weight=flip)
    else:
        y = MC._ModConvFn.apply(xd, wd, sd, None, 1, demod, flip, torch.tensor([gain], dtype=torch.float32, device=dev))
    leaves = [xd, sd, wd] + ([nd] if nd is not None else [])
    first = torch.autograd.grad(y, leaves, gyd, retain_graph=True)
    out = dict(zip(("y", "dx", "ds", "dw", "dnoise"), (y,) + first))
    for route in ("fused", "composition"):
        saved = MC.TANGENT_ROUTE[0]
        MC.TANGENT_ROUTE[0] = route
        try:
            with style_ops.second_order(generator=True):
                dx, ds = torch.autograd.grad(y, [xd, sd], gyd, create_graph=True)
            second = torch.autograd.grad((dx.float() * vx.float()).sum() + (ds * vs).sum(), [gyd, xd, sd, wd])
        finally:
            MC.TANGENT_ROUTE[0] = saved
        out.update(zip((f"{route} d_gy", f"{route} d_x", f"{route} d_s", f"{route} d_w"), second))
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}


def run():
    import stylegan2_pl_checks as K
    dev, outs = torch.device("cuda:0"), {}
    for tag in K.MODCONV_CASES:
        for dtype in (torch.float32, torch.bfloat16):
            for gain in (None, GAINS[tag]) if tag in GAINS else (None,):
                for what, t in run_case(tag, dtype, gain, dev).items():
                    outs[f"{tag} {K.dtype_name(dtype)}{'' if gain is None else f' gain={gain}'} {what}"] = t
    return outs


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--save")
    g.add_argument("--against")
    a = ap.parse_args()
    import studiogan_amd
    print("library:", studiogan_amd.LIB_PATH)
    outs = run()
    zero = [k for k, t in outs.items() if not float(t.abs().max()) > 0]
    assert not zero, f"all-zero (or non-finite) output: {zero}"
    if a.save:
        torch.save(outs, a.save)
        print(f"saved {len(outs)} tensors to {a.save}")
    else:
        ref = torch.load(a.against)
        assert ref.keys() == outs.keys(), "the two runs cover different cases"
        bad = [k for k, t in outs.items() if not (t.dtype == ref[k].dtype and torch.equal(t, ref[k]))]
        for k in outs:
            print(f"{k:40s} {'DIFFERS' if k in bad else 'equal'}")
        assert not bad, f"{len(bad)} of {len(outs)} tensors differ from {a.against}: {bad}"
        print(f"all {len(outs)} tensors bit-identical to {a.against}")
