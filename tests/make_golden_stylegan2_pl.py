"""Writes tests/golden/stylegan2_pl.npz: path-length regularisation through the StyleGAN2 generator (the REAL reference's Generator and PathLengthRegularizer,
src/utils/losses.py:168-186) on the three architectures of tests/golden/stylegan2_gen.npz (their seeded state, batch 4, seeded latents and pl_noise,
noise_mode 'const'), next to the fp64 expectation of tests/stylegan2_ref.py:

    pl_grads   = d <img, pl_noise> / d ws                 pl_lengths = sqrt( mean_rows sum_w pl_grads^2 )
    pl_mean    = lerp(0, mean(pl_lengths), 0.01)          loss = mean( (pl_lengths - pl_mean)^2 * 2 )              (pl_mean stays in the graph, as in the reference)

The reference is run the way its worker runs it: TRAINING mode, where a SynthesisBlock passes fused_modconv=False. (In eval mode its fused route carries the
styles in per-sample weights, and under no_weight_gradients(True) -- pl_no_weight_grad, which the worker sets for stylegan2 -- that route yields no gradient for
ws at all.) Both pl_no_weight_grad settings are run and agree.

Per case: <case>/{z,c,pl_noise}, <case>/pl_lengths, <case>/loss, <case>/pl_mean (after the step), <case>/dp/<parameter> (the loss's gradient for every
generator parameter, mapping network included; fp64 values stored as float32; zero where the loss does not reach the parameter), and
    <case>/ref32_err/{pl_lengths,loss,pl_mean,dp/<parameter>}   the reference's own fp32 distance from them (max |ref - fp64| / max |fp64|). The script first
                                asserts that the restatement in fp32 agrees with the reference to fp32 rounding.
For `skip` also the run with bf16 blocks (b8 and b16 in low precision, conv_clamp 256):
    skip/lowp/{pl_lengths,loss,pl_mean,dp/<parameter>}          fp64 with the clamp (what a bf16 run is held against)
    skip/bf16_floor, skip/bf16_floor_of/<quantity>              the restatement with bf16 storage in those blocks against them: relative error of loss and
                                pl_mean, max |pl_lengths - expected| / max |expected|, relative L2 distance of every parameter gradient; the largest, and each

The loss's parameter gradient is DISCONTINUOUS where a leaky-ReLU input crosses 0 or a clamp binds (the second-order pass multiplies by the slope twice), so
the fp32 bound max(2e-5, 4 ref32_err) only means something if no fp32 evaluation can land on another side than fp64. The script asserts it: every
pre-activation of the fp64 run is at least MARGIN = 4 times further from 0 than the fp32 run of the same statement is from the fp64 one anywhere in that tensor
(and, with the clamp, every activated value as far from +-256). A latent batch that fails is replaced by the next seeded one, never the bound; <case>/z_seed is
the attempt. A bias behind which nothing but a piecewise-linear activation and linear layers lead to the image gets an EXACT zero from the loss: the gradient for
ws depends on it only through sides. In these networks that is every ToRGB bias and nothing else (a synthesis layer's bias and noise strength move the
activation the next layer's style gradient is a sum over, so theirs is not zero); the script asserts that the reference's are exactly zero where the
restatement's are, and that the set is that one.
Margins found:
    skip    latents 1, 1.5e+01 fp32 errors at the closest element, the same with the clamp (latents 0: a pre-activation at 0.40 errors)
    resnet  latents 0, 3.0e+01
    orig    latents 0, 2.8e+01
bf16 storage does move sides; the script asserts that its emulation differs from fp64 on at most 0.5 % of the leaky-ReLU sides of any layer (found: 0.11 %),
each within the emulation's own error of the kink: the cap of tests/make_golden_stylegan2_r1.py.

    python tests/make_golden_stylegan2_pl.py      (needs the reference checkout: imported through oracle/ref_import.py)

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
import stylegan2_ref as S                          # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "stylegan2_pl.npz")
BF = torch.bfloat16
BATCH = 4
PL_DECAY, PL_WEIGHT = 0.01, 2
FLIP_CAP = 0.005
MARGIN = 4.0        # a kink must be this many fp32 errors away (the factor of the max(2e-5, 4 ref32_err) rule: a device's fp32 error is not the CPU's)
LOWP_CASE = "skip"
BUFFERS = ("resample_filter", "noise_const", "w_avg")


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def err(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def param_keys(sd):
    return [k for k in sd if k.split(".")[-1] not in BUFFERS]


def inputs(case, cfg, attempt=0):
    """seeded (z, c, pl_noise) of a case, fp64 on grids fp32 holds: pl_noise = N(0, 1) / sqrt(H W) rounded to 2^-10"""
    g = torch.Generator().manual_seed(7000 + 100 * attempt + case)
    z = (torch.randn(BATCH, cfg["z_dim"], generator=g, dtype=torch.float64) * 64).round() / 64
    n = max(cfg["c_dim"], 1)
    c = torch.eye(n, dtype=torch.float64)[torch.arange(BATCH) % n][:, :cfg["c_dim"]]
    r = cfg["img_resolution"]
    noise = (torch.randn(BATCH, cfg["img_channels"], r, r, generator=g, dtype=torch.float64) / r * 1024).round() / 1024
    return z, c, noise


def pl(sd, cfg, z, c, pl_noise, pkeys, pl_mean=0.0, **kw):
    """(pl_lengths, loss, pl_mean after the step, {parameter: d loss}) of the restatement by double backward, in the dtype of the arguments"""
    sd = dict(sd)
    for k in pkeys:
        sd[k] = sd[k].clone().requires_grad_(True)
    ws = S.broadcast_truncate(S.mapping_w(sd, cfg, z, c), S.num_ws(cfg))
    img = S.synthesis(sd, cfg, ws, "const", **kw)[0]
    (g,) = torch.autograd.grad((img * pl_noise).sum(), ws, create_graph=True)
    lengths = g.square().sum(2).mean(1).sqrt()
    mean = pl_mean + PL_DECAY * (lengths.mean() - pl_mean)
    loss = ((lengths - mean).square() * PL_WEIGHT).mean()
    dp = torch.autograd.grad(loss, [sd[k] for k in pkeys], allow_unused=True)
    return lengths.detach(), loss.detach(), mean.detach(), {k: (torch.zeros_like(sd[k]) if d is None else d) for k, d in zip(pkeys, dp)}


class record_pre:
    """with record_pre() as pre: every leaky ReLU input and every clamp input of the restatement, in evaluation order"""

    def __enter__(self):
        self.saved = (S.lrelu, S.clamp)
        self.lrelu, self.clamp = [], []

        def lrelu(x, mask=None):
            self.lrelu.append(x.detach())
            return self.saved[0](x, mask)

        def clamp(x, c):
            if c is not None:
                self.clamp.append((x.detach(), c))
            return self.saved[1](x, c)

        S.lrelu, S.clamp = lrelu, clamp
        return self

    def __exit__(self, *a):
        S.lrelu, S.clamp = self.saved


def kink_margin(sd, sd32, cfg, z, c, pl_noise, pkeys, **kw):
    """min over the leaky ReLU inputs (and clamp inputs) of |distance of the fp64 value from the kink| / (largest fp32 error in that tensor)"""
    with record_pre() as p64:
        pl(sd, cfg, z, c, pl_noise, pkeys, **kw)
    with record_pre() as p32:
        pl(sd32, cfg, z.float(), c.float(), pl_noise.float(), pkeys, **kw)
    margin = float("inf")
    assert len(p64.lrelu) == len(p32.lrelu) > 0 and len(p64.clamp) == len(p32.clamp)
    for a, b in zip(p64.lrelu, p32.lrelu):
        e = max(float((a - b.double()).abs().max()), 1e-30)
        margin = min(margin, float(a.abs().min()) / e)
    for (a, cl), (b, _) in zip(p64.clamp, p32.clamp):
        e = max(float((a - b.double()).abs().max()), 1e-30)
        margin = min(margin, float((a.abs() - cl).abs().min()) / e)
    return margin


def bf16_sides(sd, cfg, z, c, pl_noise, pkeys):
    """the share of leaky ReLU sides on which the bf16 emulation differs from fp64 (largest over the layers); asserts the cap and that every difference is
    within the emulation's own error of the kink"""
    with record_pre() as p64:
        pl(sd, cfg, z, c, pl_noise, pkeys, **S.LOWP)
    with record_pre() as pbf:
        pl(sd, cfg, z, c, pl_noise, pkeys, act_dtype=BF, **S.LOWP)
    worst = 0.0
    for a, b in zip(p64.lrelu, pbf.lrelu):
        flip = (a > 0) != (b > 0)
        worst = max(worst, float(flip.double().mean()))
        if bool(flip.any()):
            assert float(a[flip].abs().max()) <= float((a - b).abs().max()), "a side differs away from the kink"
    assert worst <= FLIP_CAP, f"the bf16 emulation alone differs from fp64 on {worst:.2%} of a layer's sides (cap {FLIP_CAP:.1%}): change the seed"
    return worst


def lowp_floors(sd, cfg, z, c, pl_noise, pkeys):
    """(fp64 with the clamp, {quantity: distance of the bf16 emulation from it})"""
    want = pl(sd, cfg, z, c, pl_noise, pkeys, **S.LOWP)
    emu = pl(sd, cfg, z, c, pl_noise, pkeys, act_dtype=BF, **S.LOWP)
    floors = {"pl_lengths": err(emu[0], want[0]), "loss": err(emu[1], want[1]), "pl_mean": err(emu[2], want[2])}
    floors.update({f"dp/{k}": rel_l2(emu[3][k], want[3][k]) for k in pkeys if float(want[3][k].abs().max()) > 0})
    return want, floors


def compute():
    from oracle import ref_import as RI
    RI._prepare()
    sg2 = importlib.import_module("models.stylegan2")
    ref_losses = importlib.import_module("utils.losses")
    gen = {k: (torch.from_numpy(v) if v.dtype.kind in "fi" else v) for k, v in S.load_golden().items()}
    fix = {}
    for i, (tag, cfg) in enumerate(S.CASES.items()):
        keys = [str(k) for k in gen[f"{tag}/keys"]]
        sd32 = {k: gen[f"{tag}/sd/{k}"].float() for k in keys}
        sd = {k: v.double() for k, v in sd32.items()}
        pkeys = param_keys(sd)
        lowp = tag == LOWP_CASE
        for attempt in range(20):       # the next seeded latents wherever a pre-activation sits on a kink
            z, c, noise = inputs(i, cfg, attempt)
            margin = kink_margin(sd, sd32, cfg, z, c, noise, pkeys)
            margin_lowp = kink_margin(sd, sd32, cfg, z, c, noise, pkeys, **S.LOWP) if lowp else float("inf")
            if min(margin, margin_lowp) >= MARGIN:
                break
            print(f"{tag}: latents {attempt} have a pre-activation within {min(margin, margin_lowp):.2f} x the fp32 error of a kink; taking the next seed")
        assert min(margin, margin_lowp) >= MARGIN
        fix[f"{tag}/z"], fix[f"{tag}/c"], fix[f"{tag}/pl_noise"], fix[f"{tag}/z_seed"] = z.float().numpy(), c.float().numpy(), noise.float().numpy(), np.int64(attempt)
        # the reference (fp32) as its worker runs it: training mode, both settings of pl_no_weight_grad
        G = sg2.Generator(**S.kwargs_of(cfg))
        G.load_state_dict(sd32, strict=True)
        G.train()
        params = dict(G.named_parameters())
        assert pkeys == list(params)
        runs = []
        for nwg in (True, False):
            reg = ref_losses.PathLengthRegularizer(device="cpu", pl_decay=PL_DECAY, pl_weight=PL_WEIGHT, pl_no_weight_grad=nwg)
            ws = G.mapping(z.float(), c.float())
            img = G.synthesis(ws, noise_mode="const")
            real_randn_like = torch.randn_like
            # the regulariser draws its own noise: hand it the seeded one, scaled back by the sqrt(H W) it divides by
            torch.randn_like = lambda t, **kw: noise.float() * float(np.sqrt(t.shape[2] * t.shape[3]))
            try:
                loss_ref = reg.cal_pl_reg(fake_images=img, ws=ws)
            finally:
                torch.randn_like = real_randn_like
            dp_ref = torch.autograd.grad(loss_ref, list(params.values()), allow_unused=True)
            runs.append((loss_ref.detach(), reg.pl_mean.detach().clone(), dp_ref))
        assert err(runs[0][0], runs[1][0]) <= 1e-6 and all((a is None) == (b is None) and (a is None or err(a, b) <= 1e-5 or float(b.abs().max()) == 0)
                                                            for a, b in zip(runs[0][2], runs[1][2])), "pl_no_weight_grad changes the training-mode result"
        loss_ref, mean_ref, dp_ref = runs[0]
        # the reference's pl_lengths are not returned: recomputed from its graph
        ws = G.mapping(z.float(), c.float())
        (g_ref,) = torch.autograd.grad((G.synthesis(ws, noise_mode="const") * noise.float()).sum(), ws)
        len_ref = g_ref.square().sum(2).mean(1).sqrt()
        l32, p32, m32, dp32 = pl(sd32, cfg, z.float(), c.float(), noise.float(), pkeys)
        lens, loss, mean, dp = pl(sd, cfg, z, c, noise, pkeys)
        assert err(l32, len_ref) <= 2e-6 and err(p32, loss_ref) <= 2e-6 and err(m32, mean_ref) <= 2e-6, (tag, err(l32, len_ref), err(p32, loss_ref), err(m32, mean_ref))
        fix[f"{tag}/pl_lengths"], fix[f"{tag}/loss"], fix[f"{tag}/pl_mean"] = lens.numpy(), loss.numpy(), mean.numpy()
        fix[f"{tag}/ref32_err/pl_lengths"] = np.float64(err(len_ref, lens))
        fix[f"{tag}/ref32_err/loss"] = np.float64(err(loss_ref, loss))
        fix[f"{tag}/ref32_err/pl_mean"] = np.float64(err(mean_ref, mean))
        zeros = []
        for k, gk in zip(pkeys, dp_ref):
            fix[f"{tag}/dp/{k}"] = dp[k].float().numpy()
            gk = torch.zeros_like(params[k]) if gk is None else gk
            if float(dp[k].abs().max()) > 0:
                fix[f"{tag}/ref32_err/dp/{k}"] = np.float64(err(gk, dp[k]))
                assert err(dp32[k], gk) <= max(2e-5, 4 * err(gk, dp[k])), (tag, k, err(dp32[k], gk), err(gk, dp[k]))
            else:
                assert float(gk.abs().max()) == 0, (tag, k)
                zeros.append(k)
        assert zeros and all(k.endswith("torgb.bias") for k in zeros), zeros
        worst = max(float(v) for k, v in fix.items() if k.startswith(f"{tag}/ref32_err/"))
        line = f"{tag}: latents {attempt}, loss {float(loss):.4e}, worst ref32_err {worst:.2e}, kink margin {margin:.1e}, {len(zeros)} exactly zero gradients"
        if lowp:
            want, floors = lowp_floors(sd, cfg, z, c, noise, pkeys)
            sides = bf16_sides(sd, cfg, z, c, noise, pkeys)
            fix[f"{tag}/lowp/pl_lengths"], fix[f"{tag}/lowp/loss"], fix[f"{tag}/lowp/pl_mean"] = (t.numpy() for t in want[:3])
            for k in pkeys:
                fix[f"{tag}/lowp/dp/{k}"] = want[3][k].float().numpy()
            fix[f"{tag}/bf16_floor"] = np.float64(max(floors.values()))
            for k, v in floors.items():
                fix[f"{tag}/bf16_floor_of/{k}"] = np.float64(v)
            print("   ", ", ".join(f"{k} {v:.1e}" for k, v in floors.items()))
            line += f" (with the clamp {margin_lowp:.1e}), bf16_floor {max(floors.values()):.2e}, bf16 sides differing {sides:.3%}"
        print(line)
    return fix


if __name__ == "__main__":
    fix = compute()
    np.savez_compressed(GOLDEN, **fix)
    print(f"wrote {GOLDEN}: {len(fix)} arrays, {os.path.getsize(GOLDEN)} bytes")
    assert os.path.getsize(GOLDEN) < (1 << 20)
