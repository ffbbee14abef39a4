"""Plain-torch statement of the modulated convolution and its gradients, written from the maths (no reference code):

    y[n,o,p] = d[n,o] * sum_{r,s,c} W[o,c,r,s] * ( s[n,c] * x[n,c,tap(p,r,s)] ) + noise[n,p]
    d[n,o]   = ( sum_c s[n,c]^2 Q[o,c] + 1e-8 )^(-1/2),   Q[o,c] = sum_{r,s} W[o,c,r,s]^2          (d == 1 without demodulation)

up = 1: a 'same' correlation (flip_weight=True) or convolution (False). up = 2 (3 x 3): zero-insertion upsampling by 2 through a transposed stride-2
convolution followed by the FIR low-pass `f` with gain 4, the noise last. The oracle of the GPU tests beyond the golden cases; TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_FILES = ("modconv.npz", "modconv_af.npz", "modconv_c.npz")


def golden_file_of(key):
    """which file of the fixture holds an array: operator cases a and f, case c, everything else"""
    tag = key.split("/")[1] if key.startswith("op/") else ""
    return "modconv_c.npz" if tag == "c" else "modconv_af.npz" if tag in ("a", "f") else "modconv.npz"


def load_golden():
    """the whole fixture as one dict of numpy arrays (tests/make_golden_modconv.py wrote it)"""
    fix = {}
    for name in GOLDEN_FILES:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as z:
            fix.update({k: z[k] for k in z.files})
    return fix


# operator cases of tests/golden/modconv.npz: tag -> (N, C, Cout, H, k, up, demodulate, noise, flip_weight)
OP_CASES = {
    "a": (5, 24, 40, 8, 3, 1, True, "sample", True),
    "b": (3, 20, 12, 6, 3, 1, True, "shared", True),
    "c": (2, 64, 64, 16, 3, 1, True, None, True),
    "d": (3, 16, 3, 8, 1, 1, False, None, True),
    "e": (3, 8, 16, 4, 3, 2, True, "sample", False),
    "f": (2, 32, 32, 8, 3, 2, True, "shared", False),
    "g": (2, 8, 8, 5, 3, 1, True, None, False),
}
# layer cases: tag -> (class name, constructor kwargs, input resolution, noise_mode)
LAYER_CASES = {
    "syn_up": ("SynthesisLayer", dict(in_channels=8, out_channels=16, w_dim=12, resolution=16, up=2), 8, "const"),
    "syn_up_none": ("SynthesisLayer", dict(in_channels=8, out_channels=16, w_dim=12, resolution=16, up=2), 8, "none"),
    "syn": ("SynthesisLayer", dict(in_channels=16, out_channels=16, w_dim=12, resolution=8, up=1, conv_clamp=256), 8, "const"),
    "syn_none": ("SynthesisLayer", dict(in_channels=16, out_channels=16, w_dim=12, resolution=8, up=1, conv_clamp=256), 8, "none"),
    "rgb": ("ToRGBLayer", dict(in_channels=16, out_channels=3, w_dim=12, conv_clamp=256), 8, None),
}
LAYER_BATCH, LAYER_WDIM = 3, 12


def low_pass(taps=(1, 3, 3, 1)):
    """the normalised 2-D FIR StyleGAN2 resamples with (outer product of the taps, unit sum), fp32"""
    t = torch.tensor(taps, dtype=torch.float32)
    f = torch.outer(t, t)
    return f / f.sum()


def exact_inputs(seed, N, C, Cout, H, k, up, noise):
    """seeded inputs that fp32 holds exactly (multiples of 2^-6 below 8 in magnitude): styles 1 + N(0,1) with some coefficients exactly 0"""
    g = torch.Generator().manual_seed(seed)

    def q(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale * 64).round().clamp(-448, 448) / 64

    x, w = q(N, C, H, H), q(Cout, C, k, k, scale=0.5)
    s = 1 + q(N, C)
    s[torch.rand(N, C, generator=g) < 0.15] = 0.0
    s[0, 0] = 0.0
    Ho = H * up
    nz = None if noise is None else (q(N, 1, Ho, Ho, scale=0.5) if noise == "sample" else q(Ho, Ho, scale=0.5))
    gy = q(N, Cout, Ho, Ho)
    return x, w, s, nz, gy


def modconv_ref(x, weight, styles, noise=None, up=1, demodulate=True, flip_weight=True, f=None, weight_d=None):
    """y in the dtype of its arguments (differentiable). weight_d: the weight the demodulation coefficients are taken from when it is not the one the
    convolution multiplies with (bf16 runs: the image is rounded, d comes from the fp32 parameter)"""
    N, C, H, W = x.shape
    Cout, _, k, _ = weight.shape
    xs = x * styles.reshape(N, C, 1, 1)
    if up == 1:
        w = weight if flip_weight else weight.flip(2, 3)
        u = F.conv2d(xs, w, padding=k // 2)
    else:
        # u[o, 2h + r, 2w + s] += xs[c, h, w] * W'[o, c, r, s] on a [2H + 1, 2W + 1] grid, W' = W (flip_weight=False) or its tap reversal; then the FIR
        w = weight.flip(2, 3) if flip_weight else weight
        u = F.conv_transpose2d(xs, w.transpose(0, 1), stride=2)
        f = torch.ones(1, 1) if f is None else f      # no low-pass: zero insertion times the gain
        fw = f.shape[-1]
        p0, p1 = k // 2 + (fw + 1) // 2 - (k - 1), k // 2 + (fw - 2) // 2 - (k - 2)
        u = F.pad(u, [p0, p1, p0, p1])
        taps = (f.to(u.dtype) * 4).flip(0, 1)[None, None].expand(Cout, 1, fw, fw)
        u = F.conv2d(u, taps, groups=Cout)
    if demodulate:
        Q = (weight if weight_d is None else weight_d).square().sum(dim=(2, 3))
        d = (styles.square() @ Q.t() + 1e-8).rsqrt()
        u = u * d.reshape(N, Cout, 1, 1)
    if noise is not None:
        u = u + noise
    return u


def modconv_ref_grads(x, weight, styles, noise, gy, **kw):
    """(y, dx, dweight, dstyles, dnoise or None) by autograd through modconv_ref"""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, weight, styles)]
    nz = None if noise is None else noise.detach().clone().requires_grad_(True)
    y = modconv_ref(leaves[0], leaves[1], leaves[2], nz, **kw)
    gr = torch.autograd.grad(y, leaves + ([nz] if nz is not None else []), gy)
    return (y.detach(),) + tuple(gr[:3]) + ((gr[3],) if nz is not None else (None,))


def layer_ref(cls, kw, sd, x, wl, noise_mode=None, conv_weight=None, act_mask=None):
    """The two layers from their definition, in the dtype of the arguments. sd: the layer's state (parameters and buffers by the reference's names).
    affine: styles = wl @ (A / sqrt(w_dim))^T + b_A. SynthesisLayer: lrelu_0.2( modconv(x, W, styles, noise_const * noise_strength) + b ) * sqrt(2), clamped;
    ToRGBLayer: clamp( modconv(x, W, styles / sqrt(C k^2), no demodulation) + b ). conv_weight: what the convolution multiplies with when it is not
    sd['weight'] (see modconv_ref weight_d). act_mask (bool, shape of y): which side of the leaky ReLU every element is on, when the caller fixes it (the
    derivative at a pre-activation within rounding of zero is either slope; see tests/test_modconv_gpu.py). Returns (y, {name: tensor} of the differentiable leaves it built)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items() if k not in ("resample_filter", "noise_const")}
    leaves["x"], leaves["wl"] = x.detach().clone().requires_grad_(True), wl.detach().clone().requires_grad_(True)
    W = leaves["weight"]
    Wc = W if conv_weight is None else W + (conv_weight - W).detach()      # the rounded values, the parameter's gradient
    styles = leaves["wl"] @ (leaves["affine.weight"] / wl.shape[1] ** 0.5).t() + leaves["affine.bias"]
    clamp = kw.get("conv_clamp")
    if cls == "ToRGBLayer":
        y = modconv_ref(leaves["x"], Wc, styles / (W.shape[1] * W.shape[2] ** 2) ** 0.5, demodulate=False) + leaves["bias"].reshape(1, -1, 1, 1)
    else:
        noise = sd["noise_const"] * leaves["noise_strength"] if noise_mode == "const" else None
        up = kw.get("up", 1)
        y = modconv_ref(leaves["x"], Wc, styles, noise, up=up, flip_weight=(up == 1), f=sd["resample_filter"], weight_d=W)
        pre = y + leaves["bias"].reshape(1, -1, 1, 1)
        y = (F.leaky_relu(pre, 0.2) if act_mask is None else torch.where(act_mask, pre, 0.2 * pre)) * 2 ** 0.5
    if clamp is not None:
        y = y.clamp(-clamp, clamp)
    return y, leaves
