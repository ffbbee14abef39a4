"""conv2d_resample: the plain (unmodulated) convolutions of the StyleGAN2 discriminator, channels-last, float32 or bfloat16, with first-order gradients
(second-order ones inside style_ops.second_order()).

    conv2d_plain(x, w, stride)     1x1 or 3x3 at stride 1 / pad k // 2, or 3x3 at stride 2 / pad 0; correlation, like torch's conv2d
    conv2d_resample(x, w, f, down, padding, ...)   the reference's operator for up = 1 (conv2d_resample.py:86-108): a 1x1 kernel decimates through the low-pass
                                   first and convolves the small map, a 3x3 kernel low-passes at full resolution and convolves at stride 2

The generator's Conv2dLayer runs the modulated operator with unit styles and pays two sg_modconv_reduce passes (s x, s gxs) per layer for it; a network made
of plain convolutions must not, so this is an autograd.Function of its own. Each launch goes to one of two entries (`entry_for`):
    sg_conv2d_fwd      (conv2d_raw) when the input channels fill 16-byte vectors (C % 8 in bf16, C % 4 in fp32): the planned dispatch, whose bf16 side has the
                       halo kernels for 3x3 / stride 1 and the DMA-staged tile kernel for 1x1 and for 3x3 / stride 2; the transposed gather runs on its
                       generic engine
    sg_modconv2d_fwd   with NULL scale tables otherwise (C = 3 of the image, C + 1 of the epilogue, 12 bf16 channels): the same generic engine behind an
                       entry that serves these three geometries for any channel count
Data gradient: the same dispatch on the transposed image at stride 1, the SG_PIX_TRANSPOSED gather at stride 2; weight gradient: sg_conv2d_wgrad (at stride 2
in the geometry the up = 2 path uses with swapped roles). Second order (R1), inside style_ops.second_order() only: the backward runs as _PlainConvDgradFn /
_PlainConvWgradFn. A convolution is bilinear, so their backwards are the same three launches with the roles permuted (roles `dgrad2` / `wgrad2` in the log);
a weight gradient nobody asked for (autograd.grad(inputs=[images]), the reference's no_weight_gradients) is not launched. `record()` collects which entry every launch took (tools/stylegan2_dis_bench.py prints it per layer);
FORCE pins one entry for an A/B."""
import torch

from .. import _lib as L
from ..functional._base import _first_order_only, _param_grad_wanted, conv2d_raw, conv2d_wgrad_raw
from . import upfirdn2d as _upfirdn2d
from ._fir_common import MAX_TAPS, down2_padding
from .act_fir import act_fir
from .modulated_conv2d import _modconv_raw

ENTRIES = ("sg_conv2d_fwd", "sg_modconv2d_fwd")
FORCE = None        # one of ENTRIES: every launch on that entry (benchmarks; both take every problem of this module)
_log = None


class record:
    """with record() as log: every convolution launch of this module appends (role, entry, dtype, N, Hs, Ws, C, Cout, k, geometry) to log"""

    def __enter__(self):
        global _log
        self.saved, _log = _log, []
        return _log

    def __exit__(self, *a):
        global _log
        _log = self.saved


def entry_for(C, dtype):
    """the entry a launch with C input channels takes: the planned dispatch when they fill 16-byte vectors, the NULL-table modulated entry otherwise"""
    if FORCE is not None:
        return FORCE
    return ENTRIES[0] if C % (8 if dtype == torch.bfloat16 else 4) == 0 else ENTRIES[1]


def _conv_raw(role, xh, wimg, Cout, k, mode):
    """one convolution launch on dense NHWC xh with the weight image [Cout][k*k*C]; mode as _modconv_raw's: 'same', 'down2' (3x3, stride 2, pad 0) or 'up2'
    (its transposed gather, [N, 2Hs+1, 2Ws+1, Cout])"""
    N, Hs, Ws, C = xh.shape
    entry = entry_for(C, xh.dtype)
    if _log is not None:
        _log.append((role, entry, "bf16" if xh.dtype == torch.bfloat16 else "fp32", N, Hs, Ws, C, Cout, k, mode))
    if entry == ENTRIES[1]:
        return _modconv_raw(xh, wimg, Cout, k, mode)
    if mode == "same":
        return conv2d_raw(xh, L.ptr(wimg), C, Cout, k, k, 1, k // 2, k // 2)
    if mode == "down2":
        return conv2d_raw(xh, L.ptr(wimg), C, Cout, k, k, 2, 0, 0)
    return conv2d_raw(xh, L.ptr(wimg), C, Cout, k, k, 2, 0, 0, L.PIX_TRANSPOSED, transposed_out_hw=(2 * Hs + 1, 2 * Ws + 1))


def _fwd(role, xh, weight, stride):
    """y (NHWC) of the correlation of dense NHWC xh with weight [O, I, k, k]"""
    Cout, C, k, _ = weight.shape
    wimg = weight.detach().permute(0, 2, 3, 1).contiguous().to(xh.dtype)         # [Cout][r][s][C]
    return _conv_raw(role, xh, wimg, Cout, k, "same" if stride == 1 else "down2")


def _dgrad(role, gyh, weight, stride):
    """dx (NHWC) from dense NHWC gyh"""
    Cout, C, k, _ = weight.shape
    w = weight.detach()
    if stride == 1:
        wd = w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(gyh.dtype)        # [C][2-r][2-s][Cout]
        return _conv_raw(role, gyh, wd, C, k, "same")
    # the adjoint of y[h, w] = sum x[2h + r, 2w + s] W[r, s] is the transposed gather with the same taps
    wd = w.permute(1, 2, 3, 0).contiguous().to(gyh.dtype)                       # [C][r][s][Cout]
    return _conv_raw(role, gyh, wd, C, k, "up2")


def _wgrad(role, xh, gyh, wshape, stride, out_dtype):
    """dw [O, I, k, k] in out_dtype from dense NHWC xh and gyh (fp32 accumulation)"""
    Cout, C, k, _ = wshape
    N, H, W, _ = xh.shape
    if _log is not None and role is not None:       # (role None: the first-order backward outside second_order(), whose log lists the convolution entries only)
        _log.append((role, "sg_conv2d_wgrad", "bf16" if xh.dtype == torch.bfloat16 else "fp32", N, H, W, C, Cout, k, "same" if stride == 1 else "down2"))
    dwi = torch.zeros((Cout, k, k, C), dtype=torch.float32, device=xh.device)
    if stride == 1:
        conv2d_wgrad_raw(xh, gyh, L.ptr(dwi), C, Cout, k, k, H, W, 1, k // 2, k // 2)
    else:
        conv2d_wgrad_raw(xh, gyh, L.ptr(dwi), C, Cout, k, k, gyh.shape[1], gyh.shape[2], 2, 0, 0)
    return dwi.permute(0, 3, 1, 2).to(out_dtype)


class _PlainConvDgradFn(torch.autograd.Function):
    """apply(gyh, weight, stride) -> dxh: the data gradient as a differentiable function of gy and the weight (dense NHWC tensors of one dtype)"""

    @staticmethod
    def forward(ctx, gyh, weight, stride):
        ctx.save_for_backward(gyh, weight)
        ctx.stride = stride
        return _dgrad("dgrad", gyh, weight, stride)

    @staticmethod
    def backward(ctx, v):
        _first_order_only("conv2d_resample (third order)")
        gyh, weight = ctx.saved_tensors
        vh = v.to(gyh.dtype).contiguous()
        d_gy = d_w = None
        if ctx.needs_input_grad[0]:         # dx is linear in gy: the forward convolution of the cotangent
            d_gy = _fwd("dgrad2", vh, weight, ctx.stride)
        if ctx.needs_input_grad[1] and _param_grad_wanted(weight):      # <v, dgrad(gy, W)> = <conv(v, W), gy>: the weight gradient with v in x's place
            d_w = _wgrad("wgrad2", vh, gyh, weight.shape, ctx.stride, weight.dtype)
        return d_gy, d_w, None


class _PlainConvWgradFn(torch.autograd.Function):
    """apply(xh, gyh, weight, stride) -> dw: the weight gradient as a differentiable function of x and gy (weight: shape and dtype only)"""

    @staticmethod
    def forward(ctx, xh, gyh, weight, stride):
        ctx.save_for_backward(xh, gyh)
        ctx.stride = stride
        return _wgrad("wgrad", xh, gyh, weight.shape, stride, weight.dtype)

    @staticmethod
    def backward(ctx, v):
        _first_order_only("conv2d_resample (third order)")
        xh, gyh = ctx.saved_tensors
        d_x = d_gy = None
        if ctx.needs_input_grad[0]:         # <v, wgrad(x, gy)> = <conv(x, v), gy>
            d_x = _dgrad("dgrad2", gyh, v, ctx.stride)
        if ctx.needs_input_grad[1]:
            d_gy = _fwd("dgrad2", xh, v, ctx.stride)
        return d_x, d_gy, None, None


class _PlainConvFn(torch.autograd.Function):
    """apply(x, weight, stride): x an NCHW view of NHWC memory, weight [O, I, k, k]; the result likewise channels-last"""

    @staticmethod
    def forward(ctx, x, weight, stride):
        xh = x.detach().permute(0, 2, 3, 1).contiguous()                 # free for a channels_last x
        y = _fwd("fwd", xh, weight, stride)
        ctx.save_for_backward(xh, weight, x)        # (x: for the second-order pass, whose gradient has to reach the graph behind it; xh's storage)
        ctx.stride = stride
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        xh, weight, x = ctx.saved_tensors
        stride = ctx.stride
        gyh = gy.to(xh.dtype).permute(0, 2, 3, 1).contiguous()
        dx = dw = None
        if _first_order_only("conv2d_resample"):
            if ctx.needs_input_grad[0]:
                dx = _PlainConvDgradFn.apply(gyh, weight, stride).permute(0, 3, 1, 2)
            if ctx.needs_input_grad[1] and _param_grad_wanted(weight):
                dw = _PlainConvWgradFn.apply(x.permute(0, 2, 3, 1).contiguous(), gyh, weight, stride)
            return dx, dw, None
        if ctx.needs_input_grad[0]:
            dx = _dgrad("dgrad", gyh, weight, stride).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            dw = _wgrad(None, xh, gyh, weight.shape, stride, weight.dtype)
        return dx, dw, None


def conv2d_plain(x, w, stride=1):
    """x: [N, C, H, W] float32 / bfloat16 on the GPU (channels_last costs no copy); w: [O, C, k, k], k = 1 or 3 at stride 1 (pad k // 2), k = 3 at stride 2
    (pad 0, H and W odd). Correlation. Returns the channels_last result."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 4 and isinstance(w, torch.Tensor) and w.dim() == 4 and w.shape[1] == x.shape[1]):
        raise AssertionError("conv2d_resample: x [N, I, H, W] and weight [O, I, k, k] do not agree")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"conv2d_resample: x of dtype {x.dtype} is not supported (float32 / bfloat16)")
    k = w.shape[2]
    if w.shape[3] != k or (stride, k) not in ((1, 1), (1, 3), (2, 3)):
        raise NotImplementedError(f"conv2d_resample: a {w.shape[2]} x {w.shape[3]} kernel at stride {stride} is not supported (1x1 / 3x3 at stride 1, 3x3 at stride 2)")
    if stride == 2 and (x.shape[2] % 2 == 0 or x.shape[3] % 2 == 0 or min(x.shape[2], x.shape[3]) < 3):
        raise NotImplementedError("conv2d_resample: the stride-2 convolution takes an odd extent of at least 3 (the low-passed map of a down layer)")
    L.require_gpu(x.device)
    return _PlainConvFn.apply(x, w, stride)


def conv2d_resample(x, w, f=None, up=1, down=1, padding=0, groups=1, flip_weight=True, flip_filter=False, fused=True):
    """The reference's signature. Supported: up = 1, groups = 1, flip_weight = True (correlation), down = 1 or 2, padding = k // 2, a filter of at most 4 x 4
    taps at down = 2. fused: the FIR in front of / behind nothing but the convolution runs channels-last through sg_act_fir_nhwc in plain mode; otherwise
    through upfirdn2d on the NCHW copy."""
    if up != 1 or groups != 1 or not flip_weight:
        raise NotImplementedError("conv2d_resample: up = 1, groups = 1 and flip_weight = True only (the generator's path is modulated_conv2d)")
    if down not in (1, 2):
        raise NotImplementedError(f"conv2d_resample: down={down} is not supported (1 or 2)")
    k = w.shape[2]
    if padding != k // 2:
        raise NotImplementedError(f"conv2d_resample: padding={padding} is not supported (padding = kernel_size // 2 = {k // 2})")
    if down == 1:
        return conv2d_plain(x, w, 1)
    pad = down2_padding(f, padding)
    use_fused = fused and max(_upfirdn2d._get_filter_size(f)) <= MAX_TAPS
    fir_down = 2 if k == 1 else 1       # a 1x1 kernel decimates in the low-pass, a 3x3 kernel in the convolution
    if use_fused:
        x = act_fir(x, f, pad, down=fir_down, flip_filter=flip_filter)
    else:
        x = _upfirdn2d.upfirdn2d(x, f, down=fir_down, padding=pad, flip_filter=flip_filter)
    return conv2d_plain(x, w, 1 if k == 1 else 2)
