"""Plain-torch, dtype-generic statement of the StyleGAN2 generator (mapping + synthesis networks) as a function of a state_dict, written from the maths on
tests/modconv_ref.py's modulated convolution. fp64 gives the expectation of tests/golden/stylegan2_gen.npz; `act_dtype=torch.bfloat16` rounds what the device
stores in a low-precision block (the block input, the convolution's weight image, the [2H+1]^2 core of an up = 2 layer, every layer's output, the bias of
the separate bias_act launches) and so measures the floor a bf16 run can reach. TEST INFRASTRUCTURE ONLY.

Also the seeded inputs and the restatement of the fused up = 2 layer tail (style_ops.modulated_conv2d_act) that tests/test_stylegan2_gpu.py checks."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import modconv_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stylegan2_gen.npz")
SQRT2, SQRT_HALF = 2 ** 0.5, 0.5 ** 0.5

# network cases of the fixture: tag -> Generator arguments (channels 24, 24, 12 at 4, 8, 16: the width changes and 12 is no multiple of a bf16 vector)
_BASE = dict(z_dim=24, w_dim=40, img_resolution=16, img_channels=3, num_layers=2, channel_base=192, channel_max=24)
CASES = {
    "skip": dict(_BASE, c_dim=3, architecture="skip"),
    "resnet": dict(_BASE, c_dim=0, architecture="resnet"),
    "orig": dict(_BASE, c_dim=3, architecture="orig"),
}
BATCH = 3
LOWP = dict(num_fp16_res=2, conv_clamp=256)      # the bf16 runs: blocks b8 and b16 in low precision

# fused-tail cases of the GPU test: (N, C, Cout, H) -> core (2H+1)^2, output (2H)^2
TAIL_SHAPES = {"edge": (3, 12, 12, 4), "seams": (2, 40, 24, 16)}
TAIL_NOISE = ("sample", "shared", None)
# The clamp bites in every case (a demodulated output is unit-variance, so sqrt 2 |pre| passes 2.5 on several per cent of the elements even without noise)
# but stays at the scale of the layer's intermediates (FIR output, noise and bias are a few units): the bf16 bound is 'of the output's range', and the
# separate operators round those intermediates, so a clamp far below them would hold the chain of EXISTING operators to less than a bf16 rounding of its own
# operands (at clamp 1.5 that chain sits at 1.1e-2 of range by the arithmetic alone, in an emulation on the CPU).
TAIL_EPI = {"clamp": dict(gain=1.0, clamp=2.5), "noclamp": dict(gain=1.0, clamp=None), "halfgain": dict(gain=SQRT_HALF, clamp=None)}


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def kwargs_of(cfg, **extra):
    """Generator keyword arguments (reference and this package alike) of a case"""
    import types
    model = types.SimpleNamespace(info_type="N/A", g_info_injection="N/A", info_num_discrete_c="N/A", info_num_conti_c="N/A", info_dim_discrete_c="N/A",
                                  backbone="stylegan2")
    syn = dict(channel_base=cfg["channel_base"], channel_max=cfg["channel_max"], architecture=cfg["architecture"], **extra)
    return dict(z_dim=cfg["z_dim"], c_dim=cfg["c_dim"], w_dim=cfg["w_dim"], img_resolution=cfg["img_resolution"], img_channels=cfg["img_channels"], MODEL=model,
                mapping_kwargs=dict(num_layers=cfg["num_layers"]), synthesis_kwargs=syn)


def rnd(t, dtype):
    """t with its values rounded to dtype (None: untouched)"""
    return t if dtype is None else t.to(dtype).to(t.dtype)


def lrelu(x, mask=None):
    return F.leaky_relu(x, 0.2) if mask is None else torch.where(mask, x, 0.2 * x)


def clamp(x, c):
    return x if c is None else x.clamp(-c, c)


def fc(sd, p, x, lr=1.0, act="linear"):
    """equalised-lr fully connected layer: x (lr W / sqrt(fan_in))^T + lr b, then lrelu * sqrt 2"""
    W, b = sd[p + ".weight"], sd[p + ".bias"]
    y = x @ (W * (lr / W.shape[1] ** 0.5)).t() + b * lr
    return y if act == "linear" else lrelu(y) * SQRT2


def norm2(x):
    return x * (x.square().mean(dim=1, keepdim=True) + 1e-8).rsqrt()


def mapping_w(sd, cfg, z, c):
    """[N, w_dim]: the mapping layers' output, before broadcast and truncation"""
    x = norm2(z)
    if cfg["c_dim"] > 0:
        x = torch.cat([x, norm2(fc(sd, "mapping.embed", c))], dim=1)
    for i in range(cfg["num_layers"]):
        x = fc(sd, f"mapping.fc{i}", x, lr=0.01, act="lrelu")
    return x


def num_ws(cfg):
    n = int(np.log2(cfg["img_resolution"])) - 1      # blocks
    return 2 * n - 1 + 1


def broadcast_truncate(w, n_ws, w_avg=None, psi=1, cutoff=None):
    ws = w.unsqueeze(1).repeat(1, n_ws, 1)
    if psi != 1:
        k = n_ws if cutoff is None else cutoff
        ws = torch.cat([w_avg + psi * (ws[:, :k] - w_avg), ws[:, k:]], dim=1)
    return ws


def up2_core(xs, weight):
    """transposed stride-2 convolution of the styled input with the taps as stored -> [N, O, 2H+1, 2W+1]"""
    return F.conv_transpose2d(xs, weight.transpose(0, 1), stride=2)


def fir_up2(core, f):
    """the 4-tap low-pass behind an up = 2, 3 x 3 transposed convolution: pad 1 / 1, gain 4 -> [N, O, 2H, 2W]"""
    O, fw = core.shape[1], f.shape[-1]
    taps = (f.to(core.dtype) * 4).flip(0, 1)[None, None].expand(O, 1, fw, fw)
    return F.conv2d(F.pad(core, [1, 1, 1, 1]), taps, groups=O)


def modconv_up2(x, weight, styles, f, weight_d=None, core_dtype=None):
    """R.modconv_ref(up=2, flip_weight=False) without the noise, with the stored core rounded to core_dtype"""
    N, C = styles.shape
    Q = (weight if weight_d is None else weight_d).square().sum(dim=(2, 3))
    d = (styles.square() @ Q.t() + 1e-8).rsqrt()
    core = up2_core(x * styles.reshape(N, C, 1, 1), weight) * d.reshape(N, -1, 1, 1)
    return fir_up2(rnd(core, core_dtype), f)


def synthesis_layer(sd, p, x, w, up, noise_mode, gain=1.0, conv_clamp=None, lp=None, mask=None):
    """SynthesisLayer p on x with the latent row w; lp: the storage dtype of a low-precision block (None: no rounding)"""
    W = sd[p + ".weight"]
    styles = fc(sd, p + ".affine", w)
    noise = sd[p + ".noise_const"] * sd[p + ".noise_strength"] if noise_mode == "const" else None
    Wc = rnd(W, lp)
    b = sd[p + ".bias"].reshape(1, -1, 1, 1)
    if up == 1:
        y = rnd(R.modconv_ref(x, Wc, styles, noise, weight_d=W), lp)
        y = y + rnd(b, lp)      # the separate bias_act launch takes the bias in the activation's dtype
    else:
        y = modconv_up2(x, Wc, styles, sd[p + ".resample_filter"], weight_d=W, core_dtype=lp)
        y = y + (0 if noise is None else noise) + b      # the fused tail: fp32 noise and bias on the accumulator
    return rnd(clamp(lrelu(y, mask) * (SQRT2 * gain), None if conv_clamp is None else conv_clamp * gain), lp)


def torgb_layer(sd, p, x, w, conv_clamp=None, lp=None):
    W = sd[p + ".weight"]
    styles = fc(sd, p + ".affine", w) / (W.shape[1] * W.shape[2] ** 2) ** 0.5
    y = rnd(R.modconv_ref(x, rnd(W, lp), styles, demodulate=False), lp)
    return rnd(clamp(y + rnd(sd[p + ".bias"].reshape(1, -1, 1, 1), lp), conv_clamp), lp)


def upsample2(x, f):
    """zero insertion by 2 through the low-pass with gain 4 (pad 2 / 1)"""
    N, C, H, W = x.shape
    u = torch.zeros(N, C, 2 * H, 2 * W, dtype=x.dtype)
    u[:, :, ::2, ::2] = x
    taps = (f.to(x.dtype) * 4).flip(0, 1)[None, None].expand(C, 1, 4, 4)
    return F.conv2d(F.pad(u, [2, 1, 2, 1]), taps, groups=C)


def synthesis(sd, cfg, ws, noise_mode="const", num_fp16_res=0, conv_clamp=None, act_dtype=None):
    """-> (image, {resolution: block activation}); the low-precision blocks round to act_dtype"""
    arch, log2 = cfg["architecture"], int(np.log2(cfg["img_resolution"]))
    first_low = max(2 ** (log2 + 1 - num_fp16_res), 8)
    x = img = None
    acts, row = {}, 0
    for r in [2 ** i for i in range(2, log2 + 1)]:
        p = f"synthesis.b{r}"
        lp = act_dtype if r >= first_low else None
        last = r == cfg["img_resolution"]
        kw = dict(noise_mode=noise_mode, conv_clamp=conv_clamp, lp=lp)
        if r == 4:
            x = sd[p + ".const"].unsqueeze(0).repeat(ws.shape[0], 1, 1, 1)
            x = synthesis_layer(sd, p + ".conv1", rnd(x, lp), ws[:, row], 1, **kw)
            row += 1
        else:
            x = rnd(x, lp)
            if arch == "resnet":
                Wk = sd[p + ".skip.weight"]
                f = sd[p + ".skip.resample_filter"]
                y = rnd(F.conv2d(x, rnd(Wk * (1.0 / Wk.shape[1] ** 0.5), lp)), lp)
                y = rnd(rnd(upsample2(y, f), lp) * SQRT_HALF, lp)
                x = synthesis_layer(sd, p + ".conv0", x, ws[:, row], 2, **kw)
                x = synthesis_layer(sd, p + ".conv1", x, ws[:, row + 1], 1, gain=SQRT_HALF, **kw)
                x = rnd(y + x, lp)
            else:
                x = synthesis_layer(sd, p + ".conv0", x, ws[:, row], 2, **kw)
                x = synthesis_layer(sd, p + ".conv1", x, ws[:, row + 1], 1, **kw)
            row += 2
        if img is not None:
            img = upsample2(img, sd[p + ".resample_filter"])
        if last or arch == "skip":
            y = torgb_layer(sd, p + ".torgb", x, ws[:, row], conv_clamp=conv_clamp, lp=lp)
            img = y if img is None else img + y
        acts[r] = x
    return img, acts


def generator(sd, cfg, z, c, noise_mode="const", psi=1, cutoff=None, **kw):
    w = mapping_w(sd, cfg, z, c)
    ws = broadcast_truncate(w, num_ws(cfg), sd.get("mapping.w_avg"), psi, cutoff)
    return synthesis(sd, cfg, ws, noise_mode, **kw)[0]


def generator_grads(sd, cfg, z, c, gy, noise_mode="const"):
    """(image, dz, {parameter: gradient}) by autograd; parameters = every floating entry of sd that is not a buffer"""
    buffers = ("resample_filter", "noise_const", "w_avg")
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items() if k.split(".")[-1] not in buffers}
    zl = z.detach().clone().requires_grad_(True)
    img = generator({**sd, **leaves}, cfg, zl, c, noise_mode)
    names = list(leaves)
    gr = torch.autograd.grad(img, [zl] + [leaves[k] for k in names], gy, allow_unused=True)
    return img.detach(), gr[0], {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(names, gr[1:])}


# ---- the fused up = 2 tail ------------------------------------------------------------------------------------------------------------------------------

def tail_inputs(shape, noise, seed=0):
    """seeded inputs of a fused-tail case that fp32 holds exactly: (x, weight, styles, noise or None, bias, gy)"""
    N, C, Cout, H = TAIL_SHAPES[shape]
    x, w, s, nz, gy = R.exact_inputs(4000 + 17 * list(TAIL_SHAPES).index(shape) + TAIL_NOISE.index(noise) + 100 * seed, N, C, Cout, H, 3, 2, noise)
    g = torch.Generator().manual_seed(4500 + seed)
    bias = (torch.randn(Cout, generator=g, dtype=torch.float64) * 32).round() / 64
    return x, w, s, nz, bias, gy


def tail_ref(x, w, s, nz, bias, gain=1.0, clamp_=None, mask=None, weight_d=None, core_dtype=None, inside=None):
    """the up = 2 SynthesisLayer arithmetic: clamp( gain sqrt 2 lrelu( FIR(core) + noise + bias ) ); returns (y, pre-activation). mask / inside (bool, shape
    of y): the side of the leaky ReLU / whether the clamp passes the gradient, when the caller fixes them (both derivatives jump; see test_stylegan2_gpu.py)"""
    pre = modconv_up2(x, w, s, R.low_pass().to(x.dtype), weight_d=weight_d, core_dtype=core_dtype)
    pre = pre + (0 if nz is None else nz) + bias.reshape(1, -1, 1, 1)
    a = lrelu(pre, mask) * (SQRT2 * gain)
    if clamp_ is not None and inside is not None:
        return torch.where(inside, a, a.detach().clamp(-clamp_, clamp_)), pre
    return clamp(a, clamp_), pre


def tail_grads(x, w, s, nz, bias, gy, mask=None, **kw):
    """((y, pre), {x, w, s, bias, noise: gradient})"""
    names = ["x", "w", "s", "bias"] + (["noise"] if nz is not None else [])
    lv = [t.detach().clone().requires_grad_(True) for t in (x, w, s, bias)] + ([nz.detach().clone().requires_grad_(True)] if nz is not None else [])
    y, pre = tail_ref(lv[0], lv[1], lv[2], lv[4] if nz is not None else None, lv[3], mask=mask, **kw)
    return (y.detach(), pre.detach()), dict(zip(names, torch.autograd.grad(y, lv, gy)))
