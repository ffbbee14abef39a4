"""fir_bias_act: the tail of an up = 2 StyleGAN2 synthesis layer in one launch (csrc/style_fir.hip sg_fir_bias_act_nhwc).

    y = clamp( gain * act( FIR(x; f, padding, filter_gain) + noise + bias ) )

on a channels-last activation, with no layout change: x is the [N, C, 2H+1, 2W+1] core the transposed convolution wrote (NHWC in memory), the result is the
channels-last [N, C, 2H, 2W] activation of the layer. noise ([N, 1, Ho, Wo] per sample or one shared [Ho, Wo] plane) and bias ([C]) are fp32 and enter the fp32
accumulator; the only rounding is the store. act: 'linear' or 'lrelu'.

Gradients (first order; y is kept, as bias_act keeps it):
    dpre   = sg_bias_act's gradient evaluator on (dy, y): gain * act'(.) dy, zero where the forward clamped
    dbias  = sum_{n,p} dpre,   dnoise = sum_c dpre (summed over n as well for a shared plane)
    dx     = the same kernel in plain mode on dpre: filter flipped, the adjoint padding (upfirdn2d.py derives it)
Second order, inside style_ops.second_order(generator=True): all three are linear in dy, so cotangents (v_x, v_noise, v_bias) give
    d_dy   = m (FIR(v_x) + v_noise + v_bias), m the gate of the kept y          (one sg_fir_bias_act_nhwc_gate launch; nothing flows to x, noise or bias)"""
import torch

from .. import _lib as L
from ..functional._base import _first_order_only
from ._fir_common import ACTS, MAX_TAPS, check_args, epilogue_args, epilogue_defaults, filter_2d, nhwc_out, out_size  # noqa: F401  (ACTS, MAX_TAPS, filter_2d: this module's public names)
from .bias_act import activation_funcs
from .modulated_conv2d import _reduce_raw, dnoise_of, noise_plane


def fir_nhwc_raw(xh, f2d, pad, flip_filter=False, filter_gain=1.0, noise=None, noise_stride=0, bias=None, act="linear", alpha=0.0, gain=1.0, clamp=-1.0):
    """one sg_fir_bias_act_nhwc launch. xh: dense [N, Hi, Wi, C] fp32 / bf16 on the GPU; pad = (padx0, padx1, pady0, pady1); -> [N, Ho, Wo, C] of xh's dtype"""
    y, (N, Hi, Wi, C, fh, fw) = nhwc_out("fir_bias_act", xh, f2d, pad)
    if y.numel():
        L.call("sg_fir_bias_act_nhwc", L.dt(xh), L.ptr(xh), L.ptr(f2d), L.ptr(y), L.ptr(noise), noise_stride, L.ptr(bias), N, Hi, Wi, C, fh, fw,
               *epilogue_args(pad, flip_filter, filter_gain, act, alpha, gain, clamp))
    return y


class FirBiasActFn(torch.autograd.Function):
    """apply(x, f2d, noise, bias, pad, flip_filter, filter_gain, act, alpha, gain, clamp): x an NCHW view of NHWC memory, the result likewise"""

    @staticmethod
    def forward(ctx, x, f2d, noise, bias, pad, flip_filter, filter_gain, act, alpha, gain, clamp):
        xh = x.permute(0, 2, 3, 1).contiguous()                 # free for a channels_last x
        nz, nstride = noise_plane(None if noise is None else noise.detach())
        b32 = None if bias is None else bias.detach().to(torch.float32).contiguous()
        y = fir_nhwc_raw(xh, f2d, pad, flip_filter, filter_gain, nz, nstride, b32, act, alpha, gain, clamp)
        ctx.save_for_backward(f2d, y)
        ctx.cfg = (tuple(xh.shape), pad, flip_filter, filter_gain, act, alpha, gain, clamp,
                   None if noise is None else (noise.dtype, tuple(noise.shape)), None if bias is None else bias.dtype)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        differentiable = _first_order_only("fir_bias_act")
        f2d, y = ctx.saved_tensors
        needs = (ctx.needs_input_grad[0], ctx.cfg[8] is not None and ctx.needs_input_grad[2], ctx.cfg[9] is not None and ctx.needs_input_grad[3])
        if differentiable:      # inside second_order(generator=True): the same launches, recorded as a grad-function with a backward of its own
            dx, dn, db = _FirBiasActGradFn.apply(dy, f2d, y, ctx.cfg, needs)
        else:
            dx, dn, db = _first_order(dy, f2d, y, ctx.cfg, needs)
        return dx, None, dn, db, None, None, None, None, None, None, None


def _first_order(dy, f2d, y, cfg, needs):
    """the tail's first-order backward: (dx, dnoise, dbias), each None where needs says so"""
    (N, Hi, Wi, C), pad, flip_filter, filter_gain, act, alpha, gain, clamp, noise_info, bias_dtype = cfg
    _, Ho, Wo, _ = y.shape
    dpre = dy.to(y.dtype).permute(0, 2, 3, 1).contiguous()
    if act != "linear" or gain != 1 or clamp >= 0:
        out = torch.empty_like(dpre)
        L.call("sg_bias_act", L.dt(dpre), L.ptr(dpre), None, None, L.ptr(y), None, L.ptr(out), dpre.numel(), 1, 1, 1, activation_funcs[act].cuda_idx,
               float(alpha), float(gain), float(clamp), L.stream())
        dpre = out
    dx = dn = db = None
    if needs[0]:
        fh, fw = int(f2d.shape[0]), int(f2d.shape[1])
        px0, _, py0, _ = pad
        adj = (fw - px0 - 1, Wi - Wo + px0, fh - py0 - 1, Hi - Ho + py0)
        dx = fir_nhwc_raw(dpre, f2d, adj, not flip_filter, filter_gain).permute(0, 3, 1, 2)
    if needs[1]:
        dn = dnoise_of(_reduce_raw(dpre, want_rowsum=True)[2], noise_info)
    if needs[2]:
        db = dpre.sum(dim=(0, 1, 2), dtype=torch.float32).to(bias_dtype)
    return dx, dn, db


def fir_gate_raw(vh, y, f2d, pad, flip_filter=False, filter_gain=1.0, v_noise=None, noise_stride=0, v_bias=None, act="linear", alpha=0.0, gain=1.0, clamp=-1.0):
    """one sg_fir_bias_act_nhwc_gate launch: m(y) * (FIR(vh) + v_noise + v_bias), the forward's filter and padding; vh [N, Hi, Wi, C], y [N, Ho, Wo, C]"""
    out, (N, Hi, Wi, C, fh, fw) = nhwc_out("fir_bias_act", vh, f2d, pad)
    assert tuple(out.shape) == tuple(y.shape) and y.dtype == vh.dtype and y.is_contiguous()
    if out.numel():
        L.call("sg_fir_bias_act_nhwc_gate", L.dt(vh), L.ptr(vh), L.ptr(y), L.ptr(f2d), L.ptr(out), L.ptr(v_noise), noise_stride, L.ptr(v_bias), N, Hi, Wi, C, fh, fw,
               *epilogue_args(pad, flip_filter, filter_gain, act, alpha, gain, clamp))
    return out


class _FirBiasActGradFn(torch.autograd.Function):
    """The tail's first-order backward as a differentiable function of dy. dx = FIR^T(m dy), dnoise = sum_c m dy, dbias = sum_{n,p} m dy with m the slope /
    gain / clamp gate of the kept y: linear in dy, piecewise constant in x, noise and bias. Cotangents (v_x, v_noise, v_bias) give
    d_dy = m (FIR(v_x) + v_noise + v_bias) in one sg_fir_bias_act_nhwc_gate launch; nothing flows anywhere else."""

    @staticmethod
    def forward(ctx, dy, f2d, y, cfg, needs):
        ctx.save_for_backward(f2d, y)
        ctx.cfg, ctx.dy_dtype = cfg, dy.dtype
        ctx.set_materialize_grads(False)
        return _first_order(dy, f2d, y, cfg, needs)

    @staticmethod
    def backward(ctx, vx, vn, vb):
        _first_order_only("fir_bias_act (third order)")
        f2d, y = ctx.saved_tensors
        (N, Hi, Wi, C), pad, flip_filter, filter_gain, act, alpha, gain, clamp, noise_info, bias_dtype = ctx.cfg
        vh = torch.zeros((N, Hi, Wi, C), dtype=y.dtype, device=y.device) if vx is None else vx.to(y.dtype).permute(0, 2, 3, 1).contiguous()
        vn32, nstride = noise_plane(vn)
        vb32 = None if vb is None else vb.to(torch.float32).contiguous()
        d_dy = fir_gate_raw(vh, y, f2d, pad, flip_filter, filter_gain, vn32, nstride, vb32, act, alpha, gain, clamp)
        return d_dy.permute(0, 3, 1, 2).to(ctx.dy_dtype), None, None, None, None


def fir_bias_act(x, f, padding, noise=None, bias=None, act="linear", alpha=None, gain=None, clamp=None, flip_filter=False, filter_gain=1.0):
    """x: [N, C, Hi, Wi], channels_last (a contiguous x is copied once), float32 / bfloat16 on the GPU. f: None, or a float32 filter of at most 4 x 4 taps.
    padding = [padx0, padx1, pady0, pady1]. Returns the channels_last [N, C, Ho, Wo] result; alpha / gain default to the activation's (bias_act's table)."""
    check_args("fir_bias_act", x, act, clamp, padding, bias)
    N = x.shape[0]
    f2d = filter_2d(f, x.device)
    Ho, Wo = out_size(x.shape[2], x.shape[3], f2d.shape[0], f2d.shape[1], padding)
    if noise is not None and not (isinstance(noise, torch.Tensor) and tuple(noise.shape) in ((N, 1, Ho, Wo), (Ho, Wo))):
        raise NotImplementedError(f"fir_bias_act: noise must be [N, 1, {Ho}, {Wo}] per sample or one shared [{Ho}, {Wo}] plane")
    return FirBiasActFn.apply(x, f2d, noise, bias, tuple(int(p) for p in padding), bool(flip_filter), float(filter_gain), act,
                              *epilogue_defaults(act, alpha, gain, clamp))
