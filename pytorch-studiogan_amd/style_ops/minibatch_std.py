"""minibatch_std: the minibatch standard deviation layer (Karras et al. 2018, section 3; the StyleGAN2 discriminator epilogue), csrc/mbstd.hip.

    G = min(group_size, N) (N when group_size is None),  M = N / G,  c = C / num_channels;  sample n = g M + m is in group m
    s[m, f]  = mean_{j,h,w} sqrt( var_g x[g M + m, f c + j, h, w] + 1e-8 )           (biased variance over the G samples)
    out      = cat([x, s broadcast to [N, num_channels, H, W]], dim=1)

One launch forward, writing the concatenated channels-last tensor itself, and one launch backward (mean and variance recomputed from the kept x). fp32,
deterministic. Second order inside style_ops.second_order() only: the backward runs as MinibatchStdGradFn, whose own backward is one sg_mbstd_bwd2 launch
(gradients for both dout and x: the statistic is the one operator on the discriminator's path with a second derivative)."""
import torch

from .. import _lib as L
from ..functional._base import _first_order_only, zeros_small


def _groups(N, C, group_size, num_channels):
    G = N if group_size is None else min(int(group_size), N)
    F = int(num_channels)
    if G < 1 or N % G != 0:
        raise AssertionError(f"minibatch_std: the group size {G} must divide the batch {N}")
    if F < 1 or C % F != 0:
        raise AssertionError(f"minibatch_std: num_channels {F} must divide the channels {C}")
    return G, F


def _scratch(N, H, W, C, G, F, device):
    """(part, tickets) of a launch whose (group, slice) pairs are cut into chunks: their partial sums, and the zeroed counter the last chunk is found with"""
    S = L.lib().sg_mbstd_splits(N, H, W, C, G, F)
    if S <= 1:
        return None, None
    return torch.empty((N // G) * F * S, dtype=torch.float32, device=device), zeros_small((N // G) * F, torch.int32, device)


class MinibatchStdGradFn(torch.autograd.Function):
    """apply(dh, xh, G, F) -> dxh: MinibatchStdFn's backward as a differentiable function of dout AND x (dense fp32 NHWC tensors)"""

    @staticmethod
    def forward(ctx, dh, xh, G, F):
        N, H, W, C = xh.shape
        dx = torch.empty_like(xh)
        L.call("sg_mbstd_bwd", L.ptr(xh), C, L.ptr(dh), L.ptr(dx), N, H, W, C, G, F, L.stream())
        ctx.save_for_backward(dh, xh)
        ctx.cfg = (G, F)
        return dx

    @staticmethod
    def backward(ctx, v):
        _first_order_only("minibatch_std (third order)")
        dh, xh = ctx.saved_tensors
        G, F = ctx.cfg
        N, H, W, C = xh.shape
        vh = v.to(torch.float32).contiguous()
        d_dout = torch.empty_like(dh)
        d_x = torch.empty_like(xh)
        part, tickets = _scratch(N, H, W, C, G, F, xh.device)
        L.call("sg_mbstd_bwd2", L.ptr(xh), C, L.ptr(dh), L.ptr(vh), L.ptr(d_dout), L.ptr(d_x), L.ptr(part), L.ptr(tickets), N, H, W, C, G, F, L.stream())
        return d_dout, d_x, None, None


class MinibatchStdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, G, F):
        L.require_gpu(x.device)
        N, C, H, W = x.shape
        xh = x.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()       # free for an fp32 channels_last x
        out = torch.empty((N, H, W, C + F), dtype=torch.float32, device=x.device)
        part, tickets = _scratch(N, H, W, C, G, F, x.device)
        L.call("sg_mbstd_fwd", L.ptr(xh), C, L.ptr(out), L.ptr(part), L.ptr(tickets), N, H, W, C, G, F, L.stream())
        # (x itself rides along for the second-order pass, whose gradient has to reach the graph behind it; for an fp32 channels_last x it is xh's storage)
        ctx.save_for_backward(xh, x)
        ctx.cfg = (G, F, x.dtype)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        differentiable = _first_order_only("minibatch_std")
        xh, x = ctx.saved_tensors
        G, F, x_dtype = ctx.cfg
        N, H, W, C = xh.shape
        dh = dout.to(torch.float32).permute(0, 2, 3, 1).contiguous()
        if differentiable:
            dx = MinibatchStdGradFn.apply(dh, x.to(torch.float32).permute(0, 2, 3, 1).contiguous(), G, F)
            return dx.permute(0, 3, 1, 2).to(x_dtype), None, None
        dx = torch.empty_like(xh)
        L.call("sg_mbstd_bwd", L.ptr(xh), C, L.ptr(dh), L.ptr(dx), N, H, W, C, G, F, L.stream())
        return dx.permute(0, 3, 1, 2).to(x_dtype), None, None


def minibatch_std(x, group_size, num_channels=1):
    """x: [N, C, H, W] on the GPU (channels_last costs no copy). Returns the channels_last float32 [N, C + num_channels, H, W] tensor."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 4):
        raise AssertionError("minibatch_std: x must be a 4-D NCHW tensor")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"minibatch_std: x of dtype {x.dtype} is not supported (float32 / bfloat16)")
    G, F = _groups(x.shape[0], x.shape[1], group_size, num_channels)
    return MinibatchStdFn.apply(x, G, F)
