"""This project's restatement of the StyleGAN3 generator (Karras et al. 2021) as plain functions of a state_dict, in whatever dtype the state_dict has (fp64 for
expectations, fp32 to pin it against the reference). TEST INFRASTRUCTURE: the checker of tests/test_stylegan3_{cpu,gpu}.py and of tests/make_golden_stylegan3.py.
The filtered leaky ReLU and the FIR resampling are oracle/style_ref.py's. The per-layer geometry (factors, paddings, canvas sizes, which layers store bf16) is not
re-derived here: it is read from the fixture, where tests/make_golden_stylegan3.py recorded it from the reference's own network.

`store`: a dtype (torch.bfloat16) emulates the device's storage in the layers that use it: the convolution's input, its weight image and its output, the bias
and the layer's output are rounded to it, forward and backward (gradients of those tensors are stored in the same dtype on the device)."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import style_ref as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stylegan3_gen.npz")
BATCH = 2
EMA_BETA = 0.75         # magnitude_ema_beta of every case: one update moves the average visibly
# tiny networks: at most 16 channels and a margin of 2 pixels (the kink condition of tests/make_golden_stylegan3.py is a condition on EVERY pre-activation:
# the fewer there are, the sooner a seed meets it), 2 critically sampled layers
CASES = {
    # config T, conditional, magnitude_ema != 1, a non-identity input.transform
    "t_cond": dict(z_dim=16, c_dim=3, w_dim=16, img_resolution=16, img_channels=3,
                   synthesis_kwargs=dict(channel_base=64, channel_max=16, margin_size=2, num_layers=4, num_critical=2, num_fp16_res=0, magnitude_ema_beta=EMA_BETA)),
    # config R: 1x1 kernels, radial down filters in the non-critical layers
    "r": dict(z_dim=16, c_dim=0, w_dim=16, img_resolution=16, img_channels=3,
              synthesis_kwargs=dict(channel_base=64, channel_max=16, margin_size=2, num_layers=5, num_critical=2, num_fp16_res=0, conv_kernel=1, use_radial_filters=True,
                                    magnitude_ema_beta=EMA_BETA)),
    # 32 x 32, the two highest resolutions in low precision
    "t32_lowp": dict(z_dim=16, c_dim=0, w_dim=16, img_resolution=32, img_channels=3,
                     synthesis_kwargs=dict(channel_base=64, channel_max=16, margin_size=2, num_layers=6, num_critical=2, num_fp16_res=2, magnitude_ema_beta=EMA_BETA)),
}


class _Info:
    info_type = "N/A"


def kwargs_of(cfg):
    return dict(cfg, MODEL=_Info())


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def layer_meta(fix, tag):
    """[(name, up, down, [px0, px1, py0, py1], kernel, is_torgb, use_fp16)] and the input layer's (size, sampling_rate, bandwidth), as recorded from the reference"""
    names = [str(n) for n in fix[f"{tag}/layer_names"]]
    geo = fix[f"{tag}/layer_geometry"]          # per layer: up, down, px0, px1, py0, py1, kernel, is_torgb, use_fp16
    layers = [(n, int(g[0]), int(g[1]), [int(v) for v in g[2:6]], int(g[6]), bool(g[7]), bool(g[8])) for n, g in zip(names, geo)]
    size, rate, band = fix[f"{tag}/input_geometry"]
    return layers, (int(size), float(rate), float(band))


class _Store(torch.autograd.Function):
    """storage in a narrower dtype: the value is rounded to it, and so is the gradient that comes back"""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def _st(x, dtype):
    return x if dtype is None else _Store.apply(x, dtype)


def fc(sd, p, x, act="linear", lr=1.0):
    w, b = sd[p + ".weight"], sd[p + ".bias"]
    y = x @ (w * (lr / math.sqrt(w.shape[1]))).t() + b * lr
    return TF.leaky_relu(y, 0.2) * math.sqrt(2) if act == "lrelu" else y


def _norm2(x):
    return x * (x.square().mean(dim=1, keepdim=True) + 1e-8).rsqrt()


def mapping_w(sd, cfg, z, c, num_layers=2):
    x = _norm2(z)
    if cfg["c_dim"] > 0:
        x = torch.cat([x, _norm2(fc(sd, "mapping.embed", c))], dim=1)
    for i in range(num_layers):
        x = fc(sd, f"mapping.fc{i}", x, "lrelu", 0.01)
    return x


def broadcast_truncate(w, num_ws, w_avg, psi=1, cutoff=None):
    ws = w.unsqueeze(1).repeat(1, num_ws, 1)
    if psi != 1:
        k = num_ws if cutoff is None else cutoff
        ws = torch.cat([w_avg + psi * (ws[:, :k] - w_avg), ws[:, k:]], dim=1)
    return ws


def synthesis_input(sd, geo, w):
    size, rate, band = geo
    p = "synthesis.input"
    N, dt = w.shape[0], w.dtype
    t = fc(sd, p + ".affine", w)
    t = t / t[:, :2].norm(dim=1, keepdim=True)
    cs, sn, tx, ty = t.unbind(dim=1)
    o, l = torch.zeros_like(cs), torch.ones_like(cs)
    rot = torch.stack([cs, -sn, o, sn, cs, o, o, o, l], dim=1).reshape(N, 3, 3)
    tr = torch.stack([l, o, -tx, o, l, -ty, o, o, l], dim=1).reshape(N, 3, 3)
    m = rot @ tr @ sd[p + ".transform"].unsqueeze(0)
    f0, ph0 = sd[p + ".freqs"].unsqueeze(0), sd[p + ".phases"].unsqueeze(0)
    phases = ph0 + (f0 @ m[:, :2, 2:]).squeeze(2)
    freqs = f0 @ m[:, :2, :2]
    amps = (1 - (freqs.norm(dim=2) - band) / (rate / 2 - band)).clamp(0, 1)
    # pixel centres of a size x size grid spanning size / rate image widths
    pos = ((torch.arange(size, dtype=dt) + 0.5) / size * 2 - 1) * (0.5 * size / rate)
    gx, gy = pos.reshape(1, 1, size, 1), pos.reshape(1, size, 1, 1)
    x = gx * freqs[:, :, 0].reshape(N, 1, 1, -1) + gy * freqs[:, :, 1].reshape(N, 1, 1, -1)         # [N, H, W, C]
    x = torch.sin((x + phases.reshape(N, 1, 1, -1)) * (2 * math.pi)) * amps.reshape(N, 1, 1, -1)
    C = x.shape[-1]
    return (x @ (sd[p + ".weight"] / math.sqrt(C)).t()).permute(0, 3, 1, 2)


def synthesis_layer(sd, meta, x, w, clamp=256, store=None, update_beta=None, rec=None):
    """one layer; -> (output, the magnitude_ema it used). update_beta: the moving average is updated from x first. rec: a list that receives
    (name, pre-activation u, sum of |terms| of u) of the layer"""
    name, up, down, pad, k, torgb, lowp = meta
    p = "synthesis." + name
    st = store if lowp else None
    ema = sd[p + ".magnitude_ema"]
    if update_beta is not None:
        cur = x.detach().square().mean()
        ema = cur + update_beta * (ema - cur)
    s = fc(sd, p + ".affine", w)
    W = sd[p + ".weight"]
    N, C = s.shape
    if torgb:
        s = s * (1 / math.sqrt(C * k * k))
    else:
        W = W * W.square().mean([1, 2, 3], keepdim=True).rsqrt()
        s = s * s.square().mean().rsqrt()
    wm = _st(W, st).unsqueeze(0) * s.reshape(N, 1, C, 1, 1)
    if not torgb:       # (the demodulation comes from the unrounded fp32 values on the device)
        wd = W.unsqueeze(0) * s.reshape(N, 1, C, 1, 1)
        wm = wm * (wd.square().sum(dim=[2, 3, 4], keepdim=True) + 1e-8).rsqrt()
    wm = wm * ema.rsqrt()
    x = _st(x, st)
    y = TF.conv2d(x.reshape(1, N * C, *x.shape[2:]), wm.reshape(-1, C, k, k), padding=k - 1, groups=N)
    y = _st(y.reshape(N, -1, *y.shape[2:]), st)
    fu, fd = sd.get(p + ".up_filter"), sd.get(p + ".down_filter")
    yb = SR.bias_act(y, _st(sd[p + ".bias"], st))
    u = SR.upfirdn2d(yb, fu, up=up, padding=pad, gain=up ** 2)
    if rec is not None:     # (with the sum of the magnitudes of the element's terms: what its rounding error scales with)
        rec.append((name, u.detach(), SR.upfirdn2d(yb.detach().abs(), None if fu is None else fu.abs(), up=up, padding=pad, gain=up ** 2)))
    v = SR.bias_act(u, act="lrelu", alpha=1.0 if torgb else 0.2, gain=1.0 if torgb else math.sqrt(2), clamp=clamp)
    return _st(SR.upfirdn2d(v, fd, down=down), st), ema


def synthesis(sd, fix, tag, ws, store=None, update_beta=None, rec=None, emas=None):
    layers, geo = layer_meta(fix, tag)
    x = synthesis_input(sd, geo, ws[:, 0])
    for i, meta in enumerate(layers):
        x, ema = synthesis_layer(sd, meta, x, ws[:, i + 1], store=store, update_beta=update_beta, rec=rec)
        if emas is not None:
            emas[meta[0]] = ema
    return x * 0.25


def generator(sd, fix, tag, z, c, psi=1, cutoff=None, **kw):
    cfg = CASES[tag]
    num_ws = cfg["synthesis_kwargs"]["num_layers"] + 2
    ws = broadcast_truncate(mapping_w(sd, cfg, z, c), num_ws, sd["mapping.w_avg"], psi, cutoff)
    return synthesis(sd, fix, tag, ws, **kw)


def generator_grads(sd, fix, tag, z, c, gy, params, **kw):
    """img, dz and {parameter: gradient} of <img, gy> by autograd on the restatement"""
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in params}
    zl = z.detach().clone().requires_grad_(True)
    img = generator({**sd, **leaves}, fix, tag, zl, c, **kw)
    gr = torch.autograd.grad(img, [zl] + list(leaves.values()), gy, allow_unused=True)
    dp = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(leaves, gr[1:])}
    return img.detach(), gr[0], dp
