"""Operator cases of the one-launch filtered_lrelu backward (csrc/style.hip sg_filtered_lrelu_gate / sg_filtered_lrelu_bwd), shared by
tests/test_stylegan3_cpu.py (through the interpreter) and tests/test_stylegan3_gpu.py. TEST INFRASTRUCTURE.

Every case spans more than one tile per axis in the forward launch (16 x 16 outputs) and in the backward launch (each axis in equal pieces of at most 16 inputs), with extents
that are no multiple of the forward's tile and, but for the 20 x 20 case, leave the backward's last tile partial. Inputs sit on a 1/64 grid and the filters on a 1/256 grid, so fp32 and bf16 (x, b: 1/16 grid) hold them exactly where the test needs it.
Expectations are oracle/style_ref.py in fp64, computed once per case and cached. `inputs()` asserts the project's rule for fixtures with a kink: in fp32 no
pre-activation lies within MARGIN fp32 errors of the kink or of the clamp (an fp32 error here = the rounding of a sum of `terms` products at the tensor's range),
so no fp32 evaluation order can land on another side than fp64; a seed that misses the rule is skipped for the next one."""
import functools

import torch

from oracle import style_ref as SR

MARGIN = 4.0
# tag: (shape, up taps, down taps, up, down, padding, gain, slope, clamp, flip_filter)
CASES = {
    "t_layer": ((2, 5, 20, 20), 24, 12, 4, 2, [-3, -4, -2, -6], 2 ** 0.5, 0.2, 256.0, False),       # a StyleGAN3-T layer: up 4, down 2, cropping
    "t_layer_odd": ((2, 3, 23, 21), 24, 12, 4, 2, [-3, -4, -2, -6], 2 ** 0.5, 0.2, 256.0, True),      # the same layer with a partial last tile on both axes
    "critical": ((2, 3, 21, 19), 12, 12, 2, 2, [9, 8, 9, 8], 2 ** 0.5, 0.2, 256.0, False),          # critically sampled, non-square, odd channels
    "up2": ((2, 3, 19, 18), 8, 4, 2, 1, [5, 4, 5, 4], 2 ** 0.5, 0.2, None, False),
    "down2": ((2, 4, 37, 35), None, 6, 1, 2, [3, 2, 3, 2], 2 ** 0.5, 0.2, None, True),
    "torgb": ((2, 3, 19, 21), None, None, 1, 1, 0, 1.0, 1.0, 256.0, False),                          # the degenerate ToRGB use
    "clamp": ((2, 3, 21, 19), 12, 12, 2, 2, [9, 8, 9, 8], 2 ** 0.5, 0.2, 0.75, False),               # a clamp that bites
    "clamp_flip": ((2, 3, 21, 19), 12, 12, 2, 2, [9, 8, 9, 8], 2 ** 0.5, 0.2, 0.75, True),
}


def taps(n):
    """an asymmetric low-pass of n taps on the 1/256 grid (flip_filter changes the result), None for the one-tap identity"""
    if n is None:
        return None
    t = torch.arange(n, dtype=torch.float64)
    w = torch.sin(torch.pi * (t + 0.5) / n) ** 2 * (1.0 + 0.5 * (t - (n - 1) / 2) / n)
    return ((w / w.sum()) * 256).round().div(256).float()


def pre_activation(x, b, fu, up, pad, flip):
    p = [pad] * 4 if isinstance(pad, int) else list(pad)
    return SR.upfirdn2d(SR.bias_act(x, b), fu, up=up, padding=p, gain=up ** 2, flip_filter=flip)


def gates(u, gain, slope, clamp):
    """the fp64 restatement's gate states, in the kernel's code: 1 positive, 2 negative, 0 clamped"""
    v = torch.where(u > 0, u, u * slope) * gain
    g = torch.where(u > 0, 1, 2)
    if clamp is not None:
        g = torch.where((v > -clamp) & (v < clamp), g, 0)
    return g.to(torch.uint8)


def unpack_gate(plane, aw):
    """[P, AH, ceil(AW / 4)] bytes -> [P, AH, AW] states"""
    p = plane.to(torch.int32)
    s = torch.stack([(p >> (2 * k)) & 3 for k in range(4)], dim=-1).reshape(p.shape[0], p.shape[1], -1)
    return s[:, :, :aw].to(torch.uint8)


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """dict of fp64 x, b, gy, fp32 fu, fd, and the fp64 expectations y, dx, db, gate of a case (cached: shared, never modified)"""
    shape, nu, nd, up, down, pad, gain, slope, clamp, flip = CASES[tag]
    fu, fd = taps(nu), taps(nd)
    fu64, fd64 = (None if fu is None else fu.double()), (None if fd is None else fd.double())
    for seed in range(7300, 7400):
        g = torch.Generator().manual_seed(seed)
        q = lambda *s, grid=64: (torch.randn(*s, generator=g, dtype=torch.float64) * grid).round().clamp(-3 * grid, 3 * grid) / grid      # noqa: E731
        x, b = q(*shape, grid=16), q(shape[1], grid=16) / 2 + 2.0 ** -7       # (the offset keeps x + b off zero where there is no up filter; bf16 holds it)
        u = pre_activation(x, b, fu64, up, pad, flip)
        terms = 2 * (-(-(nu or 1) // up)) ** 2
        eps = MARGIN * terms * 2.0 ** -24 * float(u.abs().max())
        near = float(u[u != 0].abs().min()) <= eps         # (an exact zero is the operator's zero padding: zero in every precision, the negative branch on both sides)
        if clamp is not None:
            v = (torch.where(u > 0, u, u * slope) * gain).abs()
            near = near or float((v - clamp).abs().min()) <= eps * gain
        if not near:
            break
    else:
        raise AssertionError(f"{tag}: no seed keeps the pre-activations off the kink and the clamp")
    xr, br = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = SR.filtered_lrelu(xr, fu=fu64, fd=fd64, b=br, up=up, down=down, padding=pad, gain=gain, slope=slope, clamp=clamp, flip_filter=flip)
    gy = q(*y.shape)
    dx, db = torch.autograd.grad(y, [xr, br], gy)
    if clamp is not None and clamp < 1:
        assert bool((gates(u, gain, slope, clamp) == 0).any()), f"{tag}: the clamp does not bite"
    return dict(x=x, b=b, gy=gy, fu=fu, fd=fd, y=y.detach(), dx=dx, db=db, gate=gates(u, gain, slope, clamp).reshape(-1, *u.shape[2:]))


@functools.lru_cache(maxsize=None)
def bf16_floor(tag):
    """what bf16 storage alone costs: the fp64 restatement on the bf16-rounded x, b, gy, its dx / db rounded to bf16, against the fp64 expectation
    (max error / max expectation); and the share of gates that the rounding of the inputs flips against fp64"""
    shape, nu, nd, up, down, pad, gain, slope, clamp, flip = CASES[tag]
    c = inputs(tag)
    r = lambda t: t.to(torch.bfloat16).double()      # noqa: E731
    xr, br = r(c["x"]).requires_grad_(True), r(c["b"]).requires_grad_(True)
    fu64, fd64 = (None if c["fu"] is None else c["fu"].double()), (None if c["fd"] is None else c["fd"].double())
    y = SR.filtered_lrelu(xr, fu=fu64, fd=fd64, b=br, up=up, down=down, padding=pad, gain=gain, slope=slope, clamp=clamp, flip_filter=flip)
    dx, db = torch.autograd.grad(y, [xr, br], r(c["gy"]))
    err = lambda a, e: float((r(a) - e).abs().max() / e.abs().max())      # noqa: E731
    g = gates(pre_activation(xr.detach(), br.detach(), fu64, up, pad, flip), gain, slope, clamp).reshape(c["gate"].shape)
    return dict(y=err(y.detach(), c["y"]), dx=err(dx, c["dx"]), db=err(db, c["db"]), gate=g, flips=float((g != c["gate"]).double().mean()))
