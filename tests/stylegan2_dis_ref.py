"""Plain-torch, dtype-generic statement of the StyleGAN2 discriminator (blocks, minibatch standard deviation, epilogue, conditioning heads) as a function of a
state_dict, and of the two kernels under it (style_ops.act_fir, style_ops.minibatch_std). fp64 gives the expectation of tests/golden/stylegan2_dis.npz;
`act_dtype=torch.bfloat16` rounds what the device stores in a low-precision block and so measures the floor a bf16 run can reach. TEST INFRASTRUCTURE ONLY.

Also the cases, the seeded inputs and the kernel-test shapes of tests/test_stylegan2_dis_{cpu,gpu}.py."""
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

import modconv_ref as R
import stylegan2_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stylegan2_dis.npz")
SQRT2, SQRT_HALF = S.SQRT2, S.SQRT_HALF
rnd, lrelu, clamp, fc = S.rnd, S.lrelu, S.clamp, S.fc

# ---- network cases: channels 12, 24, 24 at 16, 8, 4 (12 is no multiple of a bf16 vector; the epilogue convolution reads 25 channels) -----------------------
_BASE = dict(img_resolution=16, img_channels=3, channel_base=192, channel_max=24, num_classes=3, d_embed_dim=None, normalize_d_embed=False, aux_cls_type="W/O",
             info="N/A", freeze_layers=0)
CASES = {
    "orig": dict(_BASE, architecture="orig", d_cond_mtd="W/O", c_dim=0, group=2),
    "resnet": dict(_BASE, architecture="resnet", d_cond_mtd="SPD", c_dim=3, group=4),
    "skip": dict(_BASE, architecture="skip", d_cond_mtd="D2DCE", c_dim=3, d_embed_dim=16, normalize_d_embed=True, aux_cls_type="TAC", group=None, freeze_layers=2),
    # heads only: the backbone (and its seeded state) is the `orig` case's, the fixture stores the head's state and gradients
    "ac_adc": dict(_BASE, architecture="orig", d_cond_mtd="AC", c_dim=0, aux_cls_type="ADC", normalize_d_embed=True, group=2),
    "mh": dict(_BASE, architecture="orig", d_cond_mtd="MH", c_dim=0, group=2),
    "md": dict(_BASE, architecture="orig", d_cond_mtd="MD", c_dim=0, group=2),
    "info": dict(_BASE, architecture="orig", d_cond_mtd="W/O", c_dim=0, info="both", group=2),
}
FULL_CASES = ("orig", "resnet", "skip")
BATCH = 4
LOWP = dict(num_fp16_res=1, conv_clamp=256)      # the bf16 runs: block b16 in low precision
OUT_KEYS = ("h", "adv_output", "embed", "proxy", "cls_output", "label", "mi_embed", "mi_proxy", "mi_cls_output", "info_discrete_c_logits", "info_conti_mu",
            "info_conti_var")
INFO = dict(info_num_discrete_c=2, info_dim_discrete_c=3, info_num_conti_c=2)


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def is_head_key(k):
    return not (k[0] == "b" and k[1].isdigit())


def kwargs_of(cfg, **extra):
    """Discriminator keyword arguments (reference and this package alike) of a case; extra: num_fp16_res / conv_clamp / block_kwargs entries"""
    info = cfg["info"]
    model = types.SimpleNamespace(info_type=info, g_info_injection="N/A", backbone="stylegan2",
                                  **({k: v for k, v in INFO.items()} if info != "N/A" else {k: "N/A" for k in INFO}))
    block = {k: extra.pop(k) for k in list(extra) if k in ("fused_down",)}
    if cfg["freeze_layers"]:
        block["freeze_layers"] = cfg["freeze_layers"]
    return dict(c_dim=cfg["c_dim"], img_resolution=cfg["img_resolution"], img_channels=cfg["img_channels"], architecture=cfg["architecture"],
                channel_base=cfg["channel_base"], channel_max=cfg["channel_max"], cmap_dim=None, d_cond_mtd=cfg["d_cond_mtd"], aux_cls_type=cfg["aux_cls_type"],
                d_embed_dim=cfg["d_embed_dim"], num_classes=cfg["num_classes"], normalize_d_embed=cfg["normalize_d_embed"], block_kwargs=block,
                mapping_kwargs={}, epilogue_kwargs={"mbstd_group_size": cfg["group"]}, MODEL=model, **extra)


def case_inputs(i, cfg):
    """seeded image (multiples of 2^-6), labels, and one upstream gradient generator"""
    g = torch.Generator().manual_seed(4100 + i)
    q = lambda *s: (torch.randn(*s, generator=g, dtype=torch.float64) * 64).round() / 64      # noqa: E731
    img = q(BATCH, cfg["img_channels"], cfg["img_resolution"], cfg["img_resolution"])
    label = (torch.arange(BATCH) + i) % cfg["num_classes"]
    return img, label, q


# ---- the operators ----------------------------------------------------------------------------------------------------------------------------------------
def fir(x, f, pad, down=1, gain=1.0):
    """upfirdn2d at up = 1 on NCHW x: zero padding (negative crops) pad = (padx0, padx1, pady0, pady1), true convolution with f, decimation"""
    C = x.shape[1]
    x = F.pad(x, list(pad))
    taps = (f.to(x.dtype) * gain).flip(0, 1)[None, None].expand(C, 1, *f.shape)
    return F.conv2d(x, taps, groups=C)[:, :, ::down, ::down]


def bias_act(x, b=None, act="linear", gain=1.0, clamp_=None, mask=None):
    """clamp(gain * act(x + b)) on NCHW x; mask: the activation sides to take instead of the own ones (low-precision runs held to fp64's sides)"""
    if b is not None:
        x = x + b.reshape(1, -1, 1, 1)
    if act == "lrelu":
        x = lrelu(x, mask)
    return clamp(x * gain, clamp_)


def act_fir(x, f, pad, down=1, bias=None, act="linear", gain=1.0, clamp_=None, filter_gain=1.0):
    """style_ops.act_fir: the FIR of the ACTIVATED map, whose padding is zeros (not act(bias))"""
    return fir(bias_act(x, bias, act, gain, clamp_), f, pad, down, filter_gain)


def minibatch_std(x, group, nch=1):
    N, C, H, W = x.shape
    G = N if group is None else min(group, N)
    y = x.reshape(G, -1, nch, C // nch, H, W)
    y = y - y.mean(dim=0)
    y = (y.square().mean(dim=0) + 1e-8).sqrt().mean(dim=[2, 3, 4])
    return torch.cat([x, y.reshape(-1, nch, 1, 1).repeat(G, 1, H, W)], dim=1)


def conv(x, sd, p, stride=1, lp=None):
    """the equalised-lr correlation of layer p: pad k // 2 at stride 1, none at stride 2; the weight image is stored in the block's dtype"""
    W = sd[p + ".weight"]
    W = rnd(W * (1.0 / (W.shape[1] * W.shape[2] ** 2) ** 0.5), lp)
    return F.conv2d(x, W, stride=stride, padding=W.shape[2] // 2 if stride == 1 else 0)


def layer(sd, p, x, gain=1.0, conv_clamp=None, lp=None, act="lrelu"):
    """a down = 1 DConv2dLayer, convolution and separate bias_act (whose bias is in the activation's dtype)"""
    b = sd.get(p + ".bias")
    y = rnd(conv(x, sd, p, lp=lp), lp)
    return rnd(bias_act(y, None if b is None else rnd(b, lp), act, (SQRT2 if act == "lrelu" else 1.0) * gain, None if conv_clamp is None else conv_clamp * gain), lp)


def block(sd, p, arch, x, img, first, conv_clamp=None, lp=None, fused=True):
    """DiscriminatorBlock p. lp: the storage dtype of a low-precision block; fused: the device's fused_down evaluation order (the activated conv0 output is
    never stored and conv0's bias enters in fp32; the resnet skip's sqrt 1/2 rides on its filter)"""
    r = lambda t: rnd(t, lp)      # noqa: E731
    f = sd[p + ".resample_filter"]
    if x is not None:
        x = r(x)
    if first or arch == "skip":
        img = r(img)
        y = layer(sd, p + ".fromrgb", img, conv_clamp=conv_clamp, lp=lp)
        x = y if x is None else r(x + y)
        img = r(fir(img, f, (1, 1, 1, 1), 2)) if arch == "skip" else None
    g = SQRT_HALF if arch == "resnet" else 1.0
    y = None
    if arch == "resnet":
        if fused:
            y = r(conv(r(fir(x, f, (1, 1, 1, 1), 2, gain=g)), sd, p + ".skip", lp=lp))
        else:
            y = r(r(conv(r(fir(x, f, (1, 1, 1, 1), 2)), sd, p + ".skip", lp=lp)) * g)
    raw0 = r(conv(x, sd, p + ".conv0", lp=lp))
    b0 = sd[p + ".conv0.bias"]
    a = bias_act(raw0, b0 if fused else r(b0), "lrelu", SQRT2, conv_clamp)
    t = r(fir(a if fused else r(a), f, (2, 2, 2, 2)))
    raw1 = r(conv(t, sd, p + ".conv1", stride=2, lp=lp))
    x = r(bias_act(raw1, r(sd[p + ".conv1.bias"]), "lrelu", SQRT2 * g, None if conv_clamp is None else conv_clamp * g))
    if y is not None:
        x = r(y + x)
    return x, img


def epilogue(sd, p, arch, x, img, group, conv_clamp=None):
    if arch == "skip":
        x = x + layer(sd, p + ".fromrgb", img)
    x = minibatch_std(x, group)
    x = layer(sd, p + ".conv", x, conv_clamp=conv_clamp)
    return fc(sd, p + ".fc", x.flatten(1), act="lrelu")


def embed_net(sd, p, onehot, layers):
    """MappingNetwork(z_dim=0, num_ws=None, w_avg_beta=None) on a one-hot label"""
    x = S.norm2(fc(sd, p + ".embed", onehot))
    for i in range(layers):
        x = fc(sd, f"{p}.fc{i}", x, lr=0.01, act="lrelu")
    return x


def discriminator(sd, cfg, img, label, adc_fake=False, num_fp16_res=0, conv_clamp=None, act_dtype=None, fused=True):
    """-> the twelve-key dict of Discriminator.forward (label as the network returns it)"""
    arch, log2 = cfg["architecture"], int(np.log2(cfg["img_resolution"]))
    first_low = max(2 ** (log2 + 1 - num_fp16_res), 8)
    x = None
    for r in [2 ** i for i in range(log2, 2, -1)]:
        x, img = block(sd, f"b{r}", arch, x, img, r == cfg["img_resolution"], conv_clamp, act_dtype if r >= first_low else None, fused)
    h = epilogue(sd, "b4", arch, x, img, cfg["group"], conv_clamp)
    out = dict.fromkeys(OUT_KEYS)
    cond, adc, ncls = cfg["d_cond_mtd"], cfg["aux_cls_type"] == "ADC", cfg["num_classes"]
    adv = None if cond == "SPD" else fc(sd, "linear1", h).squeeze()
    if adc:
        label = label * 2 + 1 if adc_fake else label * 2
    onehot = F.one_hot(label, ncls * 2 if adc else ncls).to(h.dtype)
    if cfg["info"] in ("discrete", "both"):
        out["info_discrete_c_logits"] = h @ (sd["info_discrete_linear.weight"] / h.shape[1] ** 0.5).t()
    if cfg["info"] in ("continuous", "both"):
        out["info_conti_mu"] = h @ (sd["info_conti_mu_linear.weight"] / h.shape[1] ** 0.5).t()
        out["info_conti_var"] = torch.exp(h @ (sd["info_conti_var_linear.weight"] / h.shape[1] ** 0.5).t())
    unit = (lambda t: F.normalize(t, dim=1)) if cfg["normalize_d_embed"] else (lambda t: t)
    lin = lambda p, t: t @ (sd[p + ".weight"] / t.shape[1] ** 0.5).t() + (sd[p + ".bias"] if p + ".bias" in sd else 0)      # noqa: E731
    if cond == "AC":
        h = unit(h)
        out["cls_output"] = lin("linear2", h)
    elif cond == "SPD":
        out["embed"] = lin("linear1", h)
        cmap = embed_net(sd, "mapping", onehot, 8)
        adv = (out["embed"] * cmap).sum(dim=1, keepdim=True) / cmap.shape[1] ** 0.5
    elif cond in ("2C", "D2DCE"):
        out["embed"], out["proxy"] = unit(lin("linear2", h)), unit(embed_net(sd, "embedding", onehot, 1))
    elif cond == "MD":
        adv = adv[torch.arange(label.shape[0]), label]
    if cfg["aux_cls_type"] == "TAC":
        if cond == "AC":
            out["mi_cls_output"] = lin("linear_mi", h)
        else:
            out["mi_embed"], out["mi_proxy"] = unit(lin("linear_mi", h)), unit(embed_net(sd, "embedding_mi", onehot, 1))
    out.update(h=h, adv_output=adv, label=label)
    return out


def float_outputs(out):
    return {k: v for k, v in out.items() if v is not None and k != "label"}


def discriminator_grads(sd, cfg, img, label, gys, param_keys, **kw):
    """(outputs, dimg, {parameter: gradient}) of sum_k <out[k], gys[k]> by autograd in the dtype of the arguments"""
    img = img.clone().requires_grad_(True)
    sd = dict(sd)
    for k in param_keys:
        sd[k] = sd[k].clone().requires_grad_(True)
    out = discriminator(sd, cfg, img, label, **kw)
    loss = sum((v * gys[k]).sum() for k, v in float_outputs(out).items())
    grads = torch.autograd.grad(loss, [img] + [sd[k] for k in param_keys], allow_unused=True)
    dp = {k: (torch.zeros_like(sd[k]) if g is None else g) for k, g in zip(param_keys, grads[1:])}
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, grads[0], dp


# ---- kernel-test shapes and inputs ------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = {"edge": (3, 12, 4, 4), "odd": (2, 13, 10, 6), "seams": (2, 40, 24, 16), "strip": (1, 8, 70, 5)}       # (N, C, H, W)
HEAD_PADS = {"p2": (2, 2, 2, 2), "p1": (1, 1, 1, 1), "asym": (2, -1, 1, 3)}
HEAD_EPI = {"clamp": dict(act="lrelu", gain=SQRT2, clamp_=2.5, bias=True), "noclamp": dict(act="lrelu", gain=1.0, clamp_=None, bias=True),
            "plain": dict(act="linear", gain=1.0, clamp_=None, bias=False)}
# (N, C, H, W, group, F); `split`: 4096 elements per (group, slice) pair, which the kernel cuts into 4 chunks handed over through the ticket counter
MBSTD_CASES = {"g4f2": (8, 8, 4, 4, 4, 2), "g2f1": (4, 6, 4, 4, 2, 1), "g3": (3, 8, 4, 4, 4, 1), "all": (6, 8, 2, 2, None, 4), "split": (4, 256, 4, 4, 4, 1)}


def out_hw(H, W, pad, down, fh=4, fw=4):
    return (H + pad[2] + pad[3] - fh) // down + 1, (W + pad[0] + pad[1] - fw) // down + 1


def head_inputs(shape, pad, down, seed=0):
    """x on the 2^-6 grid below 3, bias on the grid + 2^-7 below 2 (8 significant bits each: bf16 holds both, no pre-activation is 0 and every dtype gets the
    sum's sign exactly), gy on the grid"""
    N, C, H, W = HEAD_SHAPES[shape]
    g = torch.Generator().manual_seed(5000 + seed)
    q = lambda *s, scale=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale * 64).round().clamp(-192, 192) / 64      # noqa: E731
    x = q(N, C, H, W)
    bias = q(C, scale=0.5).clamp(-126 / 64, 126 / 64) + 2.0 ** -7
    Ho, Wo = out_hw(H, W, HEAD_PADS[pad], down)
    return x, bias, q(N, C, Ho, Wo)


def head_ref(x, bias, gy, pad, down, epi):
    """fp64 (y, dx, dbias) of act_fir; asserts the inputs' margins: no pre-activation at 0, no activated value within 1e-3 of the clamp"""
    e = HEAD_EPI[epi]
    x = x.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True) if e["bias"] else None
    pre = x if b is None else x + b.reshape(1, -1, 1, 1)
    assert e["act"] == "linear" or float(pre.detach().abs().min()) > 0      # (a linear epilogue has no side to land on)
    a = bias_act(x, b, e["act"], e["gain"], None).detach()
    if e["clamp_"] is not None:
        assert float((a.abs() - e["clamp_"]).abs().min()) > 1e-3
        assert bool((a.abs() > e["clamp_"]).any()), "the clamp does not bite"
    y = act_fir(x, R.low_pass().double(), HEAD_PADS[pad], down, b, e["act"], e["gain"], e["clamp_"])
    gr = torch.autograd.grad(y, [x] + ([b] if b is not None else []), gy)
    return y.detach(), gr[0], (gr[1] if b is not None else None)


def mbstd_inputs(case, constant=False):
    N, C, H, W, group, nch = MBSTD_CASES[case]
    G = N if group is None else min(group, N)
    g = torch.Generator().manual_seed(5100 + N * 7 + C)
    q = lambda *s: (torch.randn(*s, generator=g, dtype=torch.float64) * 64).round().clamp(-192, 192) / 64      # noqa: E731
    x = q(N, C, H, W)
    if constant:        # every group constant: sample g M + m <- sample m
        M = N // G
        x = x[:M].repeat(G, 1, 1, 1)
    else:               # every group's variance >= 2^-6: one sample of each group is pushed a quarter off where needed
        M = N // G
        v = x.reshape(G, M, C, H, W)
        var = v.var(dim=0, unbiased=False)
        v[0] = torch.where(var < 2.0 ** -6, v[0] + 0.5, v[0])
        x = v.reshape(N, C, H, W)
        assert float(x.reshape(G, M, C, H, W).var(dim=0, unbiased=False).min()) >= 2.0 ** -6
    return x, q(N, C + nch, H, W)


def mbstd_ref(x, gy, group, nch):
    x = x.clone().requires_grad_(True)
    out = minibatch_std(x, group, nch)
    return out.detach(), torch.autograd.grad(out, x, gy)[0]
