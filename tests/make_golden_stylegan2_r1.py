"""Writes tests/golden/stylegan2_r1.npz: the lazy R1 regulariser through the StyleGAN2 discriminator (the REAL reference's Discriminator and
stylegan_cal_r1_reg, src/utils/losses.py:378-382) on the three full cases of tests/golden/stylegan2_dis.npz (their seeded state and labels, batch 4; their images where those pass the margin check below),
next to the fp64 expectation of tests/stylegan2_dis_ref.py:

    penalty = mean_b 0.5 || d sum(adv_output) / d img_b ||^2

Per case: <case>/penalty, <case>/r1_grads, <case>/dp/<parameter> (the penalty's gradient, fp64 values stored as float32 like the sibling fixture's; zero where
the penalty does not reach the parameter), and
    <case>/ref32_err/{penalty,r1_grads,dp/<parameter>}   the reference's own fp32 distance from them (max |ref - fp64| / max |fp64|). The script first asserts
                                that the restatement in fp32 agrees with the reference to fp32 rounding, as tests/make_golden_stylegan2_dis.py does.
    <case>/lowp/{penalty,r1_grads,dp/<parameter>}        fp64 with conv_clamp 256 (what a bf16 run is held against)
    <case>/bf16_floor           the restatement with bf16 storage in block b16 (conv_clamp 256), in both evaluation orders of the device (the larger), against
                                those: the largest of the penalty's relative error, max |r1_grads - expected| / max |expected| and the relative L2 distance of
                                every parameter gradient

The penalty's parameter gradient is DISCONTINUOUS where a pre-activation crosses 0 (the second-order pass multiplies by the leaky ReLU's slope twice), so the
fp32 bound max(2e-5, 4 ref32_err) only means something if no fp32 evaluation can land on another side than fp64. The script asserts it: every pre-activation of
the fp64 run is at least MARGIN = 4 times further from 0 than the fp32 run of the same statement is from the fp64 one anywhere in that tensor (and, with the
clamp, every activated value as far from +-256). An image that fails is replaced by the next seeded one (stylegan2_dis_ref.case_inputs(100 * attempt + case)),
never the bound; <case>/img, <case>/label and <case>/image_seed (the attempt; 0 = the sibling fixture's image) are stored. Margins found:
    orig    image 0, 6.7e+01 fp32 errors at the closest element      resnet  image 1, 3.8e+01 (image 0: b16.conv0 has a pre-activation of 1.0e-7, 0.06 errors)
    skip    image 0, 1.3e+01
bf16 storage does move sides; the script asserts that its emulation differs from fp64 on at most 0.5 % of the leaky ReLU sides of any layer (found: 0.18 %,
0.20 %, 0.20 %), each within the emulation's own error of the kink: the cap a device run is allowed. <case>/bf16_floor_of/<quantity> is each quantity's own
share of bf16_floor. (`orig` has a minibatch-std group of 2, behind which the second derivative of the statistic is the 1e-8 term alone: its bias gradients
are differences of nearly equal terms, 1e-5 and below, and both ref32_err and the bf16 floor of those tensors are large. They are kept as measured.)

    python tests/make_golden_stylegan2_r1.py      (needs the reference checkout: imported through oracle/ref_import.py)

Data only; TEST INFRASTRUCTURE ONLY."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import stylegan2_dis_ref as D                      # noqa: E402
import stylegan2_ref as S                          # noqa: E402
from make_golden_stylegan2_dis import err          # noqa: E402       (the seeding itself is reused through the stored state of stylegan2_dis.npz)

GOLDEN = os.path.join(HERE, "golden", "stylegan2_r1.npz")
BF = torch.bfloat16
FLIP_CAP = 0.005
MARGIN = 4.0        # a kink must be this many fp32 errors away (the factor of the max(2e-5, 4 ref32_err) rule: a device's fp32 error is not the CPU's)


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


class record_pre:
    """with record_pre() as pre: every leaky ReLU input and every clamp input of the restatement, in evaluation order"""

    def __enter__(self):
        self.saved = (D.lrelu, S.lrelu, D.clamp)
        self.lrelu, self.clamp = [], []

        def lrelu(x, mask=None):
            self.lrelu.append(x.detach())
            return self.saved[0](x, mask)

        def clamp(x, c):
            if c is not None:
                self.clamp.append((x.detach(), c))
            return self.saved[2](x, c)

        D.lrelu = S.lrelu = lrelu
        D.clamp = clamp
        return self

    def __exit__(self, *a):
        D.lrelu, S.lrelu, D.clamp = self.saved


def r1(sd, cfg, img, label, pkeys, **kw):
    """(penalty, r1_grads, {parameter: d penalty}) of the restatement by double backward, in the dtype of the arguments"""
    img = img.clone().requires_grad_(True)
    sd = dict(sd)
    for k in pkeys:
        sd[k] = sd[k].clone().requires_grad_(True)
    adv = D.discriminator(sd, cfg, img, label, **kw)["adv_output"]
    (g,) = torch.autograd.grad(adv.sum(), img, create_graph=True)
    penalty = (g.square().sum([1, 2, 3]) / 2).mean()
    dp = torch.autograd.grad(penalty, [sd[k] for k in pkeys], allow_unused=True)
    return penalty.detach(), g.detach(), {k: (torch.zeros_like(sd[k]) if d is None else d) for k, d in zip(pkeys, dp)}


def kink_margin(sd, sd32, cfg, img, label, pkeys, **kw):
    """min over the leaky ReLU inputs (and clamp inputs) of |distance of the fp64 value from the kink| / (largest fp32 error in that tensor)"""
    with record_pre() as p64:
        r1(sd, cfg, img, label, pkeys, **kw)
    with record_pre() as p32:
        r1(sd32, cfg, img.float(), label, pkeys, **kw)
    margin = float("inf")
    assert len(p64.lrelu) == len(p32.lrelu) > 0 and len(p64.clamp) == len(p32.clamp)
    for a, b in zip(p64.lrelu, p32.lrelu):
        e = max(float((a - b.double()).abs().max()), 1e-30)
        margin = min(margin, float(a.abs().min()) / e)
    for (a, c), (b, _) in zip(p64.clamp, p32.clamp):
        e = max(float((a - b.double()).abs().max()), 1e-30)
        margin = min(margin, float((a.abs() - c).abs().min()) / e)
    return margin


def bf16_sides(sd, cfg, img, label, pkeys, fused):
    """the share of leaky ReLU sides on which the bf16 emulation differs from fp64 (largest over the layers); asserts the cap and that every difference is
    within the emulation's own error of the kink"""
    with record_pre() as p64:
        r1(sd, cfg, img, label, pkeys, **D.LOWP)
    with record_pre() as pbf:
        r1(sd, cfg, img, label, pkeys, act_dtype=BF, fused=fused, **D.LOWP)
    worst = 0.0
    for a, b in zip(p64.lrelu, pbf.lrelu):
        flip = (a > 0) != (b > 0)
        worst = max(worst, float(flip.double().mean()))
        if bool(flip.any()):
            assert float(a[flip].abs().max()) <= float((a - b).abs().max()), "a side differs away from the kink"
    assert worst <= FLIP_CAP, f"the bf16 emulation alone differs from fp64 on {worst:.2%} of a layer's sides (cap {FLIP_CAP:.1%}): change the seed"
    return worst


def compute():
    from oracle import ref_import as RI
    RI._prepare()
    sg2 = importlib.import_module("models.stylegan2")
    ref_losses = importlib.import_module("utils.losses")
    dis = {k: (torch.from_numpy(v) if v.dtype.kind in "fi" else v) for k, v in D.load_golden().items()}
    fix = {}
    for tag in D.FULL_CASES:
        cfg = D.CASES[tag]
        keys = [str(k) for k in dis[f"{tag}/keys"]]
        sd32 = {k: dis[f"{tag}/sd/{k}"].float() for k in keys}
        sd = {k: v.double() for k, v in sd32.items()}
        label = dis[f"{tag}/label"]
        pkeys = [k[len(tag) + 4:] for k in dis if k.startswith(f"{tag}/dp/")]
        for attempt in range(20):       # the sibling fixture's image, unless a pre-activation of it sits on a kink: then the next seeded image that has none
            img = dis[f"{tag}/img"].double() if attempt == 0 else D.case_inputs(100 * attempt + D.FULL_CASES.index(tag), cfg)[0]
            margin, margin_lowp = (kink_margin(sd, sd32, cfg, img, label, pkeys, **kw) for kw in ({}, D.LOWP))
            if min(margin, margin_lowp) >= MARGIN:
                break
            print(f"{tag}: image {attempt} has a pre-activation within {min(margin, margin_lowp):.2f} x the fp32 error of a kink; taking the next seed")
        assert min(margin, margin_lowp) >= MARGIN
        fix[f"{tag}/img"], fix[f"{tag}/label"], fix[f"{tag}/image_seed"] = img.float().numpy(), label.numpy(), np.int64(attempt)
        Dn = sg2.Discriminator(**D.kwargs_of(cfg))
        Dn.load_state_dict(sd32, strict=True)
        params = dict(Dn.named_parameters())
        assert pkeys == list(params)
        # the reference (fp32), the restatement in fp32 and in fp64
        il = img.float().requires_grad_(True)
        pen_ref = ref_losses.stylegan_cal_r1_reg(adv_output=Dn(il, label)["adv_output"], images=il)
        (g_ref,) = torch.autograd.grad(pen_ref, il, retain_graph=True)      # (not stored: only shows that the penalty's graph reaches the image)
        assert bool(torch.isfinite(g_ref).all())
        (r1_ref,) = torch.autograd.grad(Dn(il, label)["adv_output"].sum(), il)
        dp_ref = torch.autograd.grad(pen_ref, list(params.values()), allow_unused=True)
        p32, g32, dp32 = r1(sd32, cfg, img.float(), label, pkeys)
        pen, g, dp = r1(sd, cfg, img, label, pkeys)
        assert err(p32, pen_ref.detach()) <= 2e-6 and err(g32, r1_ref) <= 2e-6, (tag, err(p32, pen_ref.detach()), err(g32, r1_ref))
        fix[f"{tag}/penalty"], fix[f"{tag}/r1_grads"] = pen.numpy(), g.numpy()
        fix[f"{tag}/ref32_err/penalty"] = np.float64(err(pen_ref.detach(), pen))
        fix[f"{tag}/ref32_err/r1_grads"] = np.float64(err(r1_ref, g))
        for k, gk in zip(pkeys, dp_ref):
            fix[f"{tag}/dp/{k}"] = dp[k].float().numpy()
            gk = torch.zeros_like(params[k]) if gk is None else gk
            if float(dp[k].abs().max()) > 0:
                fix[f"{tag}/ref32_err/dp/{k}"] = np.float64(err(gk, dp[k]))
                # (two fp32 evaluations of a gradient that, behind a group of 2, is a difference of nearly equal terms: held to the bound the device is held to)
                assert err(dp32[k], gk) <= max(2e-5, 4 * err(gk, dp[k])), (tag, k, err(dp32[k], gk), err(gk, dp[k]))
            else:
                assert float(gk.abs().max()) == 0, (tag, k)
        # low precision: fp64 with the clamp, and the same with bf16 storage in b16, in both evaluation orders of the device
        lp, lg, ldp = r1(sd, cfg, img, label, pkeys, **D.LOWP)
        fix[f"{tag}/lowp/penalty"], fix[f"{tag}/lowp/r1_grads"] = lp.numpy(), lg.numpy()
        for k in pkeys:
            fix[f"{tag}/lowp/dp/{k}"] = ldp[k].float().numpy()
        floors, sides = {}, 0.0
        for fused in (True, False):
            ep, eg, edp = r1(sd, cfg, img, label, pkeys, act_dtype=BF, fused=fused, **D.LOWP)
            got = {"penalty": err(ep, lp), "r1_grads": err(eg, lg)}
            got.update({f"dp/{k}": rel_l2(edp[k], ldp[k]) for k in pkeys if float(ldp[k].abs().max()) > 0})
            floors = {k: max(v, floors.get(k, 0.0)) for k, v in got.items()}
            sides = max(sides, bf16_sides(sd, cfg, img, label, pkeys, fused))
        floor = max(floors.values())
        fix[f"{tag}/bf16_floor"] = np.float64(floor)
        for k, v in floors.items():     # (each quantity's own share of the floor: none is larger than bf16_floor, so holding a quantity to its own asks no less)
            fix[f"{tag}/bf16_floor_of/{k}"] = np.float64(v)
        worst = max(float(v) for k, v in fix.items() if k.startswith(f"{tag}/ref32_err/"))
        print("   ", ", ".join(f"{k} {v:.1e}" for k, v in floors.items()))
        print(f"{tag}: image {attempt}, penalty {float(pen):.4e}, worst ref32_err {worst:.2e}, kink margin {margin:.1e} (with the clamp {margin_lowp:.1e}), bf16_floor {floor:.2e}, "
              f"bf16 sides differing {sides:.3%}")
    return fix


if __name__ == "__main__":
    fix = compute()
    np.savez_compressed(GOLDEN, **fix)
    print(f"wrote {GOLDEN}: {len(fix)} arrays, {os.path.getsize(GOLDEN)} bytes")
    assert os.path.getsize(GOLDEN) < (1 << 20)
