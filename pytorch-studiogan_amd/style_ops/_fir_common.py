"""What fir_bias_act (epilogue at the store) and act_fir (epilogue at the load) share: both are entry points of one kernel (csrc/style_fir.hip), so they take the
same filters, activations and tensors and refuse the same things. `op` is the operator's name in the messages."""
import torch

from .. import _lib as L
from .bias_act import activation_funcs
from .upfirdn2d import _get_filter_size

MAX_TAPS = 4
ACTS = ("linear", "lrelu")


def filter_2d(f, device):
    """the filter constant of upfirdn2d.setup_filter (None, 1-D separable or 2-D) as the dense fp32 [fh][fw] table the kernel takes"""
    if f is None:
        return torch.ones((1, 1), dtype=torch.float32, device=device)
    if not (isinstance(f, torch.Tensor) and f.dim() in (1, 2) and f.dtype == torch.float32):
        raise AssertionError("fir_bias_act: the filter must be None or a float32 vector / matrix from upfirdn2d.setup_filter")
    f2 = torch.outer(f, f) if f.dim() == 1 else f
    if f2.shape[0] > MAX_TAPS or f2.shape[1] > MAX_TAPS:
        raise NotImplementedError(f"fir_bias_act: a filter of {tuple(f2.shape)} taps is not supported (at most {MAX_TAPS} x {MAX_TAPS}; upfirdn2d takes the others)")
    return f2.to(device).contiguous()


def out_size(Hi, Wi, fh, fw, pad, down=1):
    px0, px1, py0, py1 = pad
    return (Hi + py0 + py1 - fh) // down + 1, (Wi + px0 + px1 - fw) // down + 1


def down2_padding(f, padding):
    """[padx0, padx1, pady0, pady1] of the low-pass of a down = 2 layer whose convolution pads by `padding` (the reference's conv2d_resample.py:76-83)"""
    fw, fh = _get_filter_size(f)
    return [padding + (fw - 1) // 2, padding + (fw - 2) // 2, padding + (fh - 1) // 2, padding + (fh - 2) // 2]


def check_args(op, x, act, clamp, padding, bias):
    if not (isinstance(x, torch.Tensor) and x.dim() == 4):
        raise AssertionError(f"{op}: x must be a 4-D NCHW tensor")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"{op}: x of dtype {x.dtype} is not supported (float32 / bfloat16)")
    if act not in ACTS:
        raise NotImplementedError(f"{op}: act={act!r} is not supported ({' / '.join(ACTS)}; bias_act takes the others)")
    if clamp is not None and clamp < 0:
        raise AssertionError(f"{op}: clamp must be >= 0")
    if len(padding) != 4:
        raise AssertionError(f"{op}: padding = [padx0, padx1, pady0, pady1]")
    if bias is not None and not (isinstance(bias, torch.Tensor) and tuple(bias.shape) == (x.shape[1],)):
        raise AssertionError(f"{op}: bias must be a vector of {x.shape[1]} channels")


def epilogue_defaults(act, alpha, gain, clamp):
    """(alpha, gain, clamp) as the kernel takes them: the activation's own slope and gain (bias_act's table) where none is given, clamp -1 for none"""
    spec = activation_funcs[act]
    return float(spec.def_alpha if alpha is None else alpha), float(spec.def_gain if gain is None else gain), float(-1 if clamp is None else clamp)


def nhwc_out(op, xh, f2d, pad, down=1):
    """the checks of a raw launch on the dense [N, Hi, Wi, C] tensor xh -> (the empty [N, Ho, Wo, C] result, (N, Hi, Wi, C, fh, fw))"""
    L.require_gpu(xh.device)
    if xh.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"{op}: x of dtype {xh.dtype} is not supported (float32 / bfloat16)")
    if not xh.is_contiguous():
        raise AssertionError(f"{op}: the kernel takes a dense NHWC tensor")
    N, Hi, Wi, C = xh.shape
    fh, fw = int(f2d.shape[0]), int(f2d.shape[1])
    if Hi + pad[2] + pad[3] < fh or Wi + pad[0] + pad[1] < fw:
        raise RuntimeError(f"{op}: the padded image is smaller than the filter")
    return torch.empty((N,) + out_size(Hi, Wi, fh, fw, pad, down) + (C,), dtype=xh.dtype, device=xh.device), (N, Hi, Wi, C, fh, fw)


def epilogue_args(pad, flip_filter, filter_gain, act, alpha, gain, clamp):
    """the arguments every entry point ends with, from the padding on"""
    return (*pad, 1 if flip_filter else 0, float(filter_gain), activation_funcs[act].cuda_idx, float(alpha), float(gain), float(clamp), L.stream())
