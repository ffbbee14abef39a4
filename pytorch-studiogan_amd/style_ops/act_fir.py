"""act_fir: the head of a StyleGAN2 discriminator down layer in one launch (csrc/style_fir.hip sg_act_fir_nhwc).

    a = clamp( gain * act( x + bias ) )  inside the image, 0 outside        y = FIR(a; f, padding, filter_gain), decimated by `down`

on a channels-last activation with no layout change: the mirror image of fir_bias_act, with the activation on the load side of the filter. x is the RAW output
of the convolution in front (its bias, lrelu, gain and clamp ride in here), the result is what the stride-2 convolution (or, for the skip path, the 1x1
convolution) reads. a is never stored. act: 'linear' or 'lrelu'; with neither bias nor activation nor gain nor clamp the operator is a plain decimating FIR.

Gradients (first order; x is kept, not a):
    dx    = sg_act_fir_nhwc_bwd: (adjoint FIR of dy) * da/dx in one launch, da/dx re-evaluated from x and bias
    dbias = sum_{n,p} dx
Second order, inside style_ops.second_order() only: the backward runs as ActFirGradFn, whose own backward is one sg_act_fir_nhwc_gate launch,
    d_dy  = FIR( v * da/dx ), decimated                 v: the cotangent on dx; d_x = d_bias = 0 (a is piecewise linear)"""
import torch

from .. import _lib as L
from ..functional._base import _first_order_only
from ._fir_common import check_args, epilogue_args, epilogue_defaults, filter_2d, nhwc_out, out_size


def act_fir_nhwc_raw(xh, f2d, pad, down=1, flip_filter=False, filter_gain=1.0, bias=None, act="linear", alpha=0.0, gain=1.0, clamp=-1.0):
    """one sg_act_fir_nhwc launch. xh: dense [N, Hi, Wi, C] fp32 / bf16 on the GPU; pad = (padx0, padx1, pady0, pady1); -> [N, Ho, Wo, C] of xh's dtype"""
    y, (N, Hi, Wi, C, fh, fw) = nhwc_out("act_fir", xh, f2d, pad, down)
    if y.numel():
        L.call("sg_act_fir_nhwc", L.dt(xh), L.ptr(xh), L.ptr(f2d), L.ptr(y), L.ptr(bias), N, Hi, Wi, C, fh, fw, int(down),
               *epilogue_args(pad, flip_filter, filter_gain, act, alpha, gain, clamp))
    return y


def _gated(bias, act, gain, clamp):
    return bias is not None or act != "linear" or gain != 1 or clamp >= 0


def act_fir_nhwc_bwd_raw(x_shape, xh, dyh, f2d, pad, down=1, flip_filter=False, filter_gain=1.0, bias=None, act="linear", alpha=0.0, gain=1.0, clamp=-1.0):
    """one sg_act_fir_nhwc_bwd launch with the forward's arguments. x_shape: the forward input's (N, Hi, Wi, C); xh: that input (None for the plain FIR, which
    has no gate to re-evaluate); dyh: dense [N, Ho, Wo, C]; -> dx [N, Hi, Wi, C]"""
    L.require_gpu(dyh.device)
    if not dyh.is_contiguous() or (xh is not None and (not xh.is_contiguous() or xh.dtype != dyh.dtype or tuple(xh.shape) != tuple(x_shape))):
        raise AssertionError("act_fir: the kernel takes dense NHWC tensors of one dtype")
    if xh is None and _gated(bias, act, gain, clamp):
        raise AssertionError("act_fir: the gated backward needs the forward's input")
    N, Hi, Wi, C = x_shape
    dx = torch.empty((N, Hi, Wi, C), dtype=dyh.dtype, device=dyh.device)
    fh, fw = int(f2d.shape[0]), int(f2d.shape[1])
    if tuple(dyh.shape) != (N,) + out_size(Hi, Wi, fh, fw, pad, down) + (C,):
        raise AssertionError("act_fir: dy does not match the forward's output")
    if dx.numel():
        L.call("sg_act_fir_nhwc_bwd", L.dt(dyh), L.ptr(xh), L.ptr(dyh), L.ptr(f2d), L.ptr(dx), L.ptr(bias), N, Hi, Wi, C, fh, fw, int(down),
               *epilogue_args(pad, flip_filter, filter_gain, act, alpha, gain, clamp))
    return dx


def act_fir_nhwc_gate_raw(vh, xh, f2d, pad, down=1, flip_filter=False, filter_gain=1.0, bias=None, act="linear", alpha=0.0, gain=1.0, clamp=-1.0):
    """one sg_act_fir_nhwc_gate launch with the forward's arguments. vh: dense [N, Hi, Wi, C], the cotangent on dx; xh: the forward's input (None for the
    plain FIR); -> d_dy [N, Ho, Wo, C]"""
    y, (N, Hi, Wi, C, fh, fw) = nhwc_out("act_fir", vh, f2d, pad, down)
    if xh is None and _gated(bias, act, gain, clamp):
        raise AssertionError("act_fir: the gated second-order pass needs the forward's input")
    if xh is not None and (not xh.is_contiguous() or xh.dtype != vh.dtype or tuple(xh.shape) != tuple(vh.shape)):
        raise AssertionError("act_fir: the kernel takes dense NHWC tensors of one dtype")
    if y.numel():
        L.call("sg_act_fir_nhwc_gate", L.dt(vh), L.ptr(vh), L.ptr(xh), L.ptr(f2d), L.ptr(y), L.ptr(bias), N, Hi, Wi, C, fh, fw, int(down),
               *epilogue_args(pad, flip_filter, filter_gain, act, alpha, gain, clamp))
    return y


class ActFirGradFn(torch.autograd.Function):
    """apply(dyh, xh, b32, f2d, x_shape, pad, down, flip_filter, filter_gain, act, alpha, gain, clamp) -> dxh: ActFirFn's data gradient as a differentiable
    function of dy (all tensors dense NHWC). Its backward is the gate launch; x and bias get no gradient (zero: the activation is piecewise linear)."""

    @staticmethod
    def forward(ctx, dyh, xh, b32, f2d, x_shape, pad, down, flip_filter, filter_gain, act, alpha, gain, clamp):
        ctx.save_for_backward(xh, b32, f2d)
        ctx.cfg = (pad, down, flip_filter, filter_gain, act, alpha, gain, clamp)
        return act_fir_nhwc_bwd_raw(x_shape, xh, dyh, f2d, pad, down, flip_filter, filter_gain, b32, act, alpha, gain, clamp)

    @staticmethod
    def backward(ctx, v):
        _first_order_only("act_fir (third order)")
        xh, b32, f2d = ctx.saved_tensors
        pad, down, flip_filter, filter_gain, act, alpha, gain, clamp = ctx.cfg
        d_dy = None
        if ctx.needs_input_grad[0]:
            d_dy = act_fir_nhwc_gate_raw(v.contiguous(), xh, f2d, pad, down, flip_filter, filter_gain, b32, act, alpha, gain, clamp)
        return (d_dy,) + (None,) * 12


class ActFirFn(torch.autograd.Function):
    """apply(x, f2d, bias, pad, down, flip_filter, filter_gain, act, alpha, gain, clamp): x an NCHW view of NHWC memory, the result likewise"""

    @staticmethod
    def forward(ctx, x, f2d, bias, pad, down, flip_filter, filter_gain, act, alpha, gain, clamp):
        xh = x.detach().permute(0, 2, 3, 1).contiguous()                 # free for a channels_last x
        b32 = None if bias is None else bias.detach().to(torch.float32).contiguous()
        y = act_fir_nhwc_raw(xh, f2d, pad, down, flip_filter, filter_gain, b32, act, alpha, gain, clamp)
        ctx.save_for_backward(f2d, xh if _gated(b32, act, gain, clamp) else None, b32)      # (the plain FIR's adjoint needs no x)
        ctx.cfg = (tuple(xh.shape), xh.dtype, pad, down, flip_filter, filter_gain, act, alpha, gain, clamp, None if bias is None else bias.dtype)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        differentiable = _first_order_only("act_fir")
        f2d, xh, b32 = ctx.saved_tensors
        x_shape, x_dtype, pad, down, flip_filter, filter_gain, act, alpha, gain, clamp, bias_dtype = ctx.cfg
        dx = db = None
        if ctx.needs_input_grad[0] or (bias_dtype is not None and ctx.needs_input_grad[2]):
            dyh = dy.to(x_dtype).permute(0, 2, 3, 1).contiguous()
            if differentiable:
                dxh = ActFirGradFn.apply(dyh, xh, b32, f2d, x_shape, pad, down, flip_filter, filter_gain, act, alpha, gain, clamp)
            else:
                dxh = act_fir_nhwc_bwd_raw(x_shape, xh, dyh, f2d, pad, down, flip_filter, filter_gain, b32, act, alpha, gain, clamp)
            if ctx.needs_input_grad[0]:
                dx = dxh.permute(0, 3, 1, 2)
            if bias_dtype is not None and ctx.needs_input_grad[2]:
                db = dxh.sum(dim=(0, 1, 2), dtype=torch.float32).to(bias_dtype)
        return dx, None, db, None, None, None, None, None, None, None, None


def act_fir(x, f, padding, down=1, bias=None, act="linear", alpha=None, gain=None, clamp=None, flip_filter=False, filter_gain=1.0):
    """x: [N, C, Hi, Wi], channels_last (a contiguous x is copied once), float32 / bfloat16 on the GPU. f: None, or a float32 filter of at most 4 x 4 taps.
    padding = [padx0, padx1, pady0, pady1]; down: 1 or 2. Returns the channels_last [N, C, Ho, Wo] result; alpha / gain default to the activation's."""
    check_args("act_fir", x, act, clamp, padding, bias)
    if down not in (1, 2):
        raise NotImplementedError(f"act_fir: down={down!r} is not supported (1 or 2; upfirdn2d takes the others)")
    return ActFirFn.apply(x, filter_2d(f, x.device), bias, tuple(int(p) for p in padding), int(down), bool(flip_filter), float(filter_gain), act,
                          *epilogue_defaults(act, alpha, gain, clamp))
