"""modulated_conv2d: StyleGAN2's modulated, demodulated convolution (reference src/models/stylegan2.py:28-98) with its first-order gradients.

The reference builds per-sample weights [N, Cout, Cin, k, k] and runs a grouped convolution with groups = N (or, with fused_modconv=False, three passes
over the activation). Both compute

    y[n,o,p] = d[n,o] * sum_{r,s,c} W[o,c,r,s] * ( s[n,c] * x[n,c,tap(p,r,s)] ) + noise[n,p],     d[n,o] = ( sum_c s[n,c]^2 Q[o,c] + 1e-8 )^(-1/2),
    Q[o,c] = sum_{r,s} W[o,c,r,s]^2

which is a convolution with ONE weight image and two per-sample scale tables: csrc/modconv.hip runs it in one launch (sg_modconv2d_fwd), the styles on the
activation operand as it is loaded, d and the noise on the fp32 accumulator. No per-sample weight exists at any point.

Gradients (gy = dL/dy; u = the convolution before demodulation, so y = d u + noise):
    gu = d gy;   gxs = conv^T(W, gu);   dx = s gxs
    ds = sum_p x gxs  -  s * ( (gd d^3) @ Q ),            gd[n,o] = sum_p gy u
    dW = wgrad(s x, gu)  -  W * ( (gd d^3)^T @ s^2 )[:, :, None, None]
    dnoise = sum_o gy  (summed over n as well when the noise is one shared plane)
The backward keeps y, not u: sum_p gy (y - noise) = d gd, so gd d^3 = d^2 sum_p gy (y - noise) and nothing is ever divided by a style or a coefficient
(styles may be exactly zero). The data gradient runs through the same kernel (pre-scale d on gy), the weight gradient through sg_conv2d_wgrad on the
materialised s x and gu; the two demodulation terms are [N x Cout]^T [N x C]-sized products in plain torch."""
import collections

import torch

from .. import _lib as L
from ..functional._base import _first_order_only, _param_grad_wanted, conv2d_wgrad_raw
from . import upfirdn2d as _upfirdn2d


def _validate_operands(op, x, weight, styles):
    """the refusals every route of the operator shares (op: the name they speak under): tensor ranks, shape agreement, dtype; -> (N, C, H, W, Cout, kh, kw)"""
    if not (isinstance(x, torch.Tensor) and x.dim() == 4):
        raise AssertionError(f"{op}: x must be a 4-D NCHW tensor")
    if not (isinstance(weight, torch.Tensor) and weight.dim() == 4):
        raise AssertionError(f"{op}: weight must be [out_channels, in_channels, kh, kw]")
    N, C, H, W = x.shape
    Cout, Cw, kh, kw = weight.shape
    if Cw != C or not (isinstance(styles, torch.Tensor) and tuple(styles.shape) == (N, C)):
        raise AssertionError(f"{op}: weight [O, I, kh, kw], x [N, I, H, W] and styles [N, I] do not agree")
    if x.dtype not in (torch.float32, torch.bfloat16):      # float16 included: the reference's pre-normalisation for it is not carried over
        raise NotImplementedError(f"{op}: x of dtype {x.dtype} is not supported (float32 / bfloat16)")
    return N, C, H, W, Cout, kh, kw


def _validate_kernel(op, kh, kw):
    """the shared refusal of anything but a square 1 x 1 or 3 x 3 kernel; -> k"""
    if kh != kw or kh not in (1, 3):
        raise NotImplementedError(f"{op}: weight with a {kh} x {kw} kernel is not supported (square 1 x 1 or 3 x 3)")
    return kh


def _validate(x, weight, styles, noise, up, down, padding, resample_filter):
    """every refusal of the operator, before any device work; -> (N, C, H, W, Cout, k)"""
    N, C, H, W, Cout, kh, kw = _validate_operands("modulated_conv2d", x, weight, styles)
    if down != 1:
        raise NotImplementedError(f"modulated_conv2d: down={down} is not supported (down=1 only)")
    if up not in (1, 2):
        raise NotImplementedError(f"modulated_conv2d: up={up} is not supported (up=1 or up=2)")
    k = _validate_kernel("modulated_conv2d", kh, kw)
    if up == 2 and k == 1:
        raise NotImplementedError("modulated_conv2d: up=2 with a 1 x 1 weight is not supported")
    if padding != k // 2:
        raise NotImplementedError(f"modulated_conv2d: padding={padding} is not supported (padding = kernel_size // 2 = {k // 2})")
    if resample_filter is not None and not (isinstance(resample_filter, torch.Tensor) and resample_filter.dim() in (1, 2) and resample_filter.dtype == torch.float32):
        raise AssertionError("modulated_conv2d: resample_filter must be None (no low-pass) or a float32 vector / matrix from upfirdn2d.setup_filter")
    if noise is not None:
        Ho, Wo = H * up, W * up
        if not (isinstance(noise, torch.Tensor) and (tuple(noise.shape) == (N, 1, Ho, Wo) or tuple(noise.shape) == (Ho, Wo))):
            raise NotImplementedError(f"modulated_conv2d: noise of shape {tuple(noise.shape) if isinstance(noise, torch.Tensor) else noise!r} is not supported "
                                      f"([N, 1, {Ho}, {Wo}] per sample or one shared [{Ho}, {Wo}] plane)")
    return N, C, H, W, Cout, k


def _up2_fir_padding(padding, k, resample_filter, up=2):
    """[padx0, padx1, pady0, pady1] of the low-pass behind the transposed convolution (conv2d_resample.py:81-125)"""
    fw, fh = _upfirdn2d._get_filter_size(resample_filter)
    return [padding + (fw + up - 1) // 2 - (k - 1), padding + (fw - up) // 2 - (k - up), padding + (fh + up - 1) // 2 - (k - 1), padding + (fh - up) // 2 - (k - up)]


def noise_plane(noise):
    """(the fp32 contiguous values, floats between two samples' planes) of a noise tensor as the kernels take it: [N, 1, Ho, Wo] per sample, or one shared
    [Ho, Wo] plane (stride 0); (None, 0) without noise. A forward hands its argument over detached."""
    if noise is None:
        return None, 0
    nz = noise.to(torch.float32).contiguous()
    return nz, (nz.shape[-2] * nz.shape[-1] if nz.dim() == 4 else 0)


def dnoise_of(rowsum, noise_info):
    """the noise's gradient from the per-pixel sums over the channels (fp32 [N, Ho * Wo]): per sample, or summed over the batch for one shared plane;
    noise_info: (dtype, shape) of the noise tensor"""
    dtype, shape = noise_info
    return (rowsum if len(shape) == 4 else rowsum.sum(dim=0)).reshape(shape).to(dtype)


def _weight_image(w32, flipped, up, dtype, data_grad=False):
    """the image the kernel reads, of dtype, from the fp32 weight [Cout, C, k, k] (flipped: its taps turned round). The forward's: [Cout][r][s][C]. The data
    gradient's: [C][r][s][Cout], at up = 1 with the taps turned round once more ([C][2-r][2-s][Cout], a `same` convolution), at up = 2 as they are (`down2`:
    gxs[h,w] = sum gu[2h+r, 2w+s] W[r,s])"""
    weff = w32.flip(2, 3) if flipped else w32
    if not data_grad:
        return weff.permute(0, 2, 3, 1).contiguous().to(dtype)
    return (weff.flip(2, 3) if up == 1 else weff).permute(1, 2, 3, 0).contiguous().to(dtype)


def _fill_conv(c, x, wimg, Cout, k, mode):
    """fills the sg_conv_fwd_desc c of a modulated-convolution launch and allocates its NHWC result. x: dense [N,Hs,Ws,C] NHWC; wimg: [Cout][k*k*C] of x.dtype.
    mode 'same' (stride 1, pad k//2), 'up2' (transposed stride-2 gather, [N,2Hs+1,2Ws+1,Cout]) or 'down2' (plain stride 2, pad 0)."""
    N, Hs, Ws, C = x.shape
    c.dtype = L.dt(x)
    c.N, c.Hs, c.Ws, c.C, c.ldx = N, Hs, Ws, C, C
    c.R = c.S = k
    if mode == "same":
        Ho, Wo, c.stride, c.pad_h, c.pad_w, c.pix_flags = Hs, Ws, 1, k // 2, k // 2, 0
    elif mode == "up2":
        Ho, Wo, c.stride, c.pad_h, c.pad_w, c.pix_flags = 2 * Hs + 1, 2 * Ws + 1, 2, 0, 0, L.PIX_TRANSPOSED
    else:
        Ho, Wo, c.stride, c.pad_h, c.pad_w, c.pix_flags = (Hs - 3) // 2 + 1, (Ws - 3) // 2 + 1, 2, 0, 0, 0
    c.Ho, c.Wo, c.Cout = Ho, Wo, Cout
    c.epi_flags, c.alpha, c.beta = 0, 1.0, 1.0
    out = torch.empty((N, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    c.x, c.w, c.out, c.ldo = L.ptr(x), L.ptr(wimg), L.ptr(out), Cout
    return out


def _modconv_raw(x, wimg, Cout, k, mode, pre=None, post=None, noise=None, noise_stride=0):
    """one sg_modconv2d_fwd launch; x, wimg and mode as _fill_conv takes them. Returns the NHWC result."""
    d = L.ModConvDesc()
    out = _fill_conv(d.conv, x, wimg, Cout, k, mode)
    d.pre, d.post, d.noise, d.noise_stride = L.ptr(pre), L.ptr(post), L.ptr(noise), noise_stride
    if L.lib().sg_modconv2d_ok(L.C.byref(d)) != 1:
        raise RuntimeError("modulated_conv2d: sg_modconv2d_ok refused the problem (there is no other path)")
    L.call("sg_modconv2d_fwd", d, L.stream())
    return out


def _jvp_raw(xh, vxh, wimg, Cout, k, mode, s32, vs32, post, y, e, noise, noise_stride):
    """one sg_modconv2d_jvp launch: post * K(W)[s vx + vs x] + e (y - noise), the forward's tangent along (vx, vs); geometry as _modconv_raw"""
    j = L.ModConvJvpDesc()
    out = _fill_conv(j.m.conv, xh, wimg, Cout, k, mode)
    j.m.pre, j.m.post, j.m.noise, j.m.noise_stride = L.ptr(s32), L.ptr(post), L.ptr(noise), noise_stride
    j.vx, j.vs, j.y, j.e, j.ldy = L.ptr(vxh), L.ptr(vs32), L.ptr(y), L.ptr(e), Cout
    if L.lib().sg_modconv2d_jvp_ok(L.C.byref(j)) != 1:
        raise RuntimeError("modulated_conv2d: sg_modconv2d_jvp_ok refused the problem (there is no other path)")
    L.call("sg_modconv2d_jvp", j, L.stream())
    return out


def _reduce_raw(a, b=None, rowsub=None, rowsub_stride=0, scale=None, want_rowsum=False):
    """sg_modconv_reduce over dense NHWC a (and b): -> (scale * a or None, sum_p a (b - rowsub) [N, C] or None, sum_c a [N, P] or None)"""
    N, C = a.shape[0], a.shape[3]
    P = a.shape[1] * a.shape[2]
    out = torch.empty_like(a) if scale is not None else None
    part = None
    if b is not None:
        part = torch.empty((N, L.lib().sg_modconv_reduce_slabs(P), C), dtype=torch.float32, device=a.device)
    rowsum = torch.empty((N, P), dtype=torch.float32, device=a.device) if want_rowsum else None
    L.call("sg_modconv_reduce", L.dt(a), L.ptr(a), L.ptr(b), L.ptr(rowsub), rowsub_stride, L.ptr(scale), L.ptr(out), L.ptr(part), L.ptr(rowsum),
           N, P, C, C, C, L.stream())
    return out, (part.sum(dim=1) if part is not None else None), rowsum


# what a forward leaves for its backward. noise_info: None, or (dtype, shape) of the noise tensor; noise_stride: of the saved plane nz (noise_plane)
_Cfg = collections.namedtuple("_Cfg", "up demodulate flipped k w_dtype s_dtype noise_info noise_stride")
# the saved tensors the first-order backward reads, in the order they are saved and handed to _ModConvGradFn; the graph's own x, weight and styles follow
# them. post = g d (dco when there is no post_gain): what scales gy; d alone stays in gd d^3
_Saved = collections.namedtuple("_Saved", "xh w32 s32 Q dco y nz post")
_N_SAVED = len(_Saved._fields)


class _ModConvFn(torch.autograd.Function):
    """the kernel's part of the operator: y = d * conv(W, s * x) (+ noise at up = 1) as a channels_last NCHW tensor; at up = 2 the [2H+1, 2W+1] result of the
    transposed convolution, in front of the FIR"""

    @staticmethod
    def forward(ctx, x, weight, styles, noise, up, demodulate, flip_weight, post_gain=None):
        """post_gain: None, or a one-element fp32 tensor g (a constant: no gradient) with y = g * d * conv(W, s * x): it rides in the per-[N, Cout] post-scale
        table, g * d, or g alone without demodulation (StyleGAN3's input_gain; no elementwise pass of its own)"""
        N, C, H, W = x.shape
        Cout, k = weight.shape[0], weight.shape[2]
        xh = x.permute(0, 2, 3, 1).contiguous()                 # NHWC in memory: free for a channels_last x
        w32 = weight.detach().to(torch.float32).contiguous()
        s32 = styles.detach().to(torch.float32).contiguous()
        Q = torch.empty((Cout, C), dtype=torch.float32, device=x.device)
        dco = torch.empty((N, Cout), dtype=torch.float32, device=x.device) if demodulate else None
        # d always from the fp32 values the caller passed, whatever the activation dtype (reference :52-59)
        L.call("sg_modconv_dcoef", L.ptr(w32), L.ptr(s32) if demodulate else None, L.ptr(Q), L.ptr(dco), N, C, Cout, k * k, L.stream())
        # taps of the image the kernel reads: correlation at up = 1, the gather of the transposed convolution at up = 2 (conv2d_resample.py:124 passes
        # `not flip_weight` on, and conv_transpose2d scatters with the taps as given)
        flipped = (k > 1) and ((up == 1) != bool(flip_weight))
        nz, nstride = noise_plane(None if noise is None else noise.detach())
        post = dco
        if post_gain is not None:
            g = post_gain.detach().to(torch.float32).reshape(1, 1)
            post = dco * g if demodulate else g.expand(N, Cout).contiguous()
        y = _modconv_raw(xh, _weight_image(w32, flipped, up, x.dtype), Cout, k, "same" if up == 1 else "up2", pre=s32, post=post, noise=nz, noise_stride=nstride)
        ctx.save_for_backward(*_Saved(xh, w32, s32, Q, dco, y, nz, post), x, weight, styles)     # (the last three: for the second-order route)
        ctx.cfg = _Cfg(up, demodulate, flipped, k, weight.dtype, styles.dtype, None if noise is None else (noise.dtype, tuple(noise.shape)), nstride)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        differentiable = _first_order_only("modulated_conv2d")
        saved, (x, weight, styles) = _Saved(*ctx.saved_tensors[:_N_SAVED]), ctx.saved_tensors[_N_SAVED:]
        need_noise = saved.nz is not None and ctx.needs_input_grad[3]
        if differentiable:
            # inside second_order(generator=True): the same launches, recorded as a grad-function with a backward of its own. The weight gradient only where
            # the running graph task wants it (path-length regularisation asks for the latents' alone, as the reference's no_weight_gradients does).
            want_w = ctx.needs_input_grad[1] and _param_grad_wanted(weight)
            dx, dw, ds, dn = _ModConvGradFn.apply(gy, x, weight, styles, ctx.cfg, want_w, need_noise, *saved)
            return dx, dw, ds, dn, None, None, None, None
        dx, dw, ds, dn, _ = _first_order(saved, ctx.cfg, gy, ctx.needs_input_grad[1], need_noise)
        return dx, dw, ds, dn, None, None, None, None


def _data_grad(gyh, w32, pre, cfg, C):
    """K^T[pre * gy]: the unscaled data gradient through the same kernel (pre rides on gy as its pre-scale: fp32 product, one rounding)"""
    return _modconv_raw(gyh, _weight_image(w32, cfg.flipped, cfg.up, gyh.dtype, data_grad=True), C, cfg.k, "same" if cfg.up == 1 else "down2", pre=pre)


def _tangent_operand(xh, vxh, s32, vs32):
    """s vx + vs x, materialised: what the composition convolves and what the weight-gradient kernel takes"""
    return _reduce_raw(vxh, scale=s32)[0] + _reduce_raw(xh, scale=vs32)[0]


def _wgrad_into(dwi, operand, gu, up, k, C, Cout, H, W):
    """dwi += wgrad(operand, gu); dwi is [Cout, k, k, C] at up = 1 and [C, k, k, Cout] at up = 2, where the roles swap (the stride-2 convolution gu -> gxs
    has the weight image [C][r][s][Cout])"""
    if up == 1:
        conv2d_wgrad_raw(operand, gu, L.ptr(dwi), C, Cout, k, k, H, W, 1, k // 2, k // 2)
    else:
        conv2d_wgrad_raw(gu, operand, L.ptr(dwi), Cout, C, k, k, H, W, 2, 0, 0)


def _wgrad_image(up, k, C, Cout, device):
    return torch.zeros((Cout, k, k, C) if up == 1 else (C, k, k, Cout), dtype=torch.float32, device=device)


def _wgrad_as_weight(dwi, up, flipped):
    dw = dwi.permute(0, 3, 1, 2) if up == 1 else dwi.permute(3, 0, 1, 2)
    return dw.flip(2, 3) if flipped else dw


def _first_order(sv, cfg, gy, need_w, need_noise):
    """the operator's first-order backward from the saved tensors sv (_Saved): (dx NCHW view, dw, ds, dnoise, what a second-order pass keeps)"""
    N, H, W, C = sv.xh.shape
    Cout = sv.w32.shape[0]
    gyh = gy.to(sv.xh.dtype).permute(0, 2, 3, 1).contiguous()
    # gu = d gy, d gd = sum_p gy (y - noise), dnoise = sum_o gy: one pass over gy and y
    gu, dgd, gnoise = gyh, None, None
    if cfg.demodulate:
        gu, dgd, gnoise = _reduce_raw(gyh, b=sv.y, rowsub=sv.nz, rowsub_stride=cfg.noise_stride, scale=sv.post, want_rowsum=need_noise)
    elif sv.post is not None:
        gu, _, gnoise = _reduce_raw(gyh, scale=sv.post, want_rowsum=need_noise)
    elif need_noise:
        _, _, gnoise = _reduce_raw(gyh, want_rowsum=True)
    # unscaled data gradient through the same kernel (d rides on gy as its pre-scale: fp32 product, one rounding), then dx = s gxs, sum_p x gxs
    gxs = _data_grad(gyh, sv.w32, sv.post, cfg, C)
    dx, ds, _ = _reduce_raw(gxs, b=sv.xh, scale=sv.s32)
    t = None
    if cfg.demodulate:
        t = dgd * sv.dco * sv.dco                                            # gd d^3
        ds = ds - sv.s32 * (t @ sv.Q)
    dw = None
    if need_w:
        xs, _, _ = _reduce_raw(sv.xh, scale=sv.s32)                          # s x, materialised for the weight-gradient kernel
        dwi = _wgrad_image(cfg.up, cfg.k, C, Cout, sv.xh.device)
        _wgrad_into(dwi, xs, gu, cfg.up, cfg.k, C, Cout, H, W)
        dw = _wgrad_as_weight(dwi, cfg.up, cfg.flipped)
        if cfg.demodulate:
            dw = dw - sv.w32 * (t.t() @ (sv.s32 * sv.s32))[:, :, None, None]
        dw = dw.to(cfg.w_dtype)
    dn = dnoise_of(gnoise, cfg.noise_info) if need_noise else None
    return dx.permute(0, 3, 1, 2), dw, ds.to(cfg.s_dtype), dn, (gyh, gu, dgd, gxs)


# Which route the tangent d_gy takes. One sg_modconv2d_jvp launch where it does not lose to the composition it replaces (operand combine, sg_modconv2d_fwd,
# multiply-add with y), measured at the layer shapes of a 256^2 network, batch 16 (profiles/stylegan2_pl_bench.txt): fp32 at up = 1 it wins 1.04-1.22x; at
# up = 2 it loses (0.94x), and in bf16 it loses at every shape (0.44-0.92x: the second operand chunk costs the kernel a wave of occupancy and its unpacking
# doubles the vector work of a loop the forward already spends on the styles). Those keep the composition.
TANGENT_ROUTE = [None]      # None: by the rule; "fused" / "composition": forced (tests and tools/stylegan2_pl_bench.py run both everywhere)


def tangent_fused(dtype, up):
    if TANGENT_ROUTE[0] is not None:
        return TANGENT_ROUTE[0] == "fused"
    return dtype == torch.float32 and up == 1


class _ModConvGradFn(torch.autograd.Function):
    """The first-order backward of _ModConvFn as a differentiable function of (gy, x, weight, styles): what path-length regularisation differentiates.

    With cotangents vx on dx and vs on ds, Psi = <vx, dx> + <vs, ds> = <gy, y'>, y' the forward-mode tangent of y along (x', s') = (vx, vs):
        d_gy = y' = g d K(W)[s vx + vs x] + e (y - noise),     e = -d^2 r,  r = (s vs) Q^T          (one sg_modconv2d_jvp launch, or the composition: tangent_fused)
    and Psi = g sum_o ( d a + d' b ) with d' = d e, a = sum_p gy K[s vx + vs x], b = sum_p gy K[s x]. Its other gradients, with
    alpha = g d a = sum_p gy y' - e beta and beta = g d b = sum_p gy (y - noise) (kept from the first pass), so that nothing is divided by d or a style:
        d_x = vs G + s G',          G = K^T[g d gy] (kept),  G' = K^T[g d' gy]                                      (the data-gradient route once more)
        d_s = sum_p vx G + sum_p x G' + s (T1 Q) - vs (T2 Q),     T1 = -alpha d^2 + 3 beta d^4 r,  T2 = beta d^2        (dd'/ds = 3 d^5 s Q r - d^3 vs Q)
        d_W = wgrad(s vx + vs x, g d gy) + wgrad(s x, g d' gy) + W ( T1^T s^2 - 2 T2^T (s vs) )
    Without demodulation e = d' = 0 and only the first term of each is left. A cotangent on dW or dnoise is not a path of the reference and is refused."""

    @staticmethod
    def forward(ctx, gy, x, weight, styles, cfg, want_w, want_noise, *saved):
        dx, dw, ds, dn, kept = _first_order(_Saved(*saved), cfg, gy, want_w, want_noise)
        ctx.save_for_backward(*saved, *kept)
        ctx.cfg, ctx.gy_dtype, ctx.x_dtype = cfg, gy.dtype, x.dtype
        ctx.set_materialize_grads(False)
        return dx, dw, ds, dn

    @staticmethod
    def backward(ctx, vx, vw, vs, vn):
        _first_order_only("modulated_conv2d (third order)")
        if vw is not None or vn is not None:
            raise NotImplementedError("modulated_conv2d: a second-order pass with a cotangent on the weight's or the noise's gradient is not supported "
                                      "(path-length regularisation differentiates the gradient for the latents alone)")
        sv, (gyh, gu, dgd, gxs) = _Saved(*ctx.saved_tensors[:_N_SAVED]), ctx.saved_tensors[_N_SAVED:]
        xh, w32, s32, Q, dco, post, cfg = sv.xh, sv.w32, sv.s32, sv.Q, sv.dco, sv.post, ctx.cfg
        up, k, demodulate = cfg.up, cfg.k, cfg.demodulate
        N, H, W, C = xh.shape
        Cout = w32.shape[0]
        T = xh.dtype
        no_grads = (None,) * (3 + _N_SAVED)      # cfg, want_w, want_noise and the saved tensors of forward's signature
        vxh = torch.zeros_like(xh) if vx is None else vx.to(T).permute(0, 2, 3, 1).contiguous()
        vs32 = torch.zeros_like(s32) if vs is None else vs.to(torch.float32).contiguous()
        wimg = _weight_image(w32, cfg.flipped, up, T)
        r = e = None
        if demodulate:
            r = (s32 * vs32) @ Q.t()
            e = -(dco * dco) * r
        operand = None
        if tangent_fused(T, up):
            ydot = _jvp_raw(xh, vxh, wimg, Cout, k, "same" if up == 1 else "up2", s32, vs32, post, sv.y, e, sv.nz, cfg.noise_stride)
        else:       # the composition: the operand materialised (the weight's gradient below takes it too), the forward launch, one multiply-add with y
            operand = _tangent_operand(xh, vxh, s32, vs32)
            ydot = _modconv_raw(operand, wimg, Cout, k, "same" if up == 1 else "up2", post=post)
            if demodulate:
                u = sv.y if sv.nz is None else sv.y - sv.nz.reshape(-1, H, W, 1).to(T)
                ydot = torch.addcmul(ydot, e.to(T)[:, None, None, :], u)
        d_gy = ydot.permute(0, 3, 1, 2).to(ctx.gy_dtype) if ctx.needs_input_grad[0] else None
        need_x, need_w, need_s = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if not (need_x or need_w or need_s):
            return (d_gy, None, None, None) + no_grads
        # d_x and the pixel sums of d_s: G with the cotangents, then G' through the data-gradient route with the pre-table g d' = post e
        vsG, sum_vxG, _ = _reduce_raw(gxs, b=vxh, scale=vs32)
        d_x, d_s = vsG, sum_vxG
        poste = None
        if demodulate:
            poste = post * e                                                    # g d'
            g2 = _data_grad(gyh, w32, poste, cfg, C)
            sG2, sum_xG2, _ = _reduce_raw(g2, b=xh, scale=s32)
            d_x = d_x + sG2
            _, s1, _ = _reduce_raw(gyh, b=ydot)                                 # sum_p gy y'
            alpha, beta, d2 = s1 - e * dgd, dgd, dco * dco
            t1, t2 = -alpha * d2 + 3.0 * beta * d2 * d2 * r, beta * d2
            d_s = d_s + sum_xG2 + s32 * (t1 @ Q) - vs32 * (t2 @ Q)
        d_w = None
        if need_w:
            if operand is None:
                operand = _tangent_operand(xh, vxh, s32, vs32)
            dwi = _wgrad_image(up, k, C, Cout, xh.device)
            _wgrad_into(dwi, operand, gu, up, k, C, Cout, H, W)
            if demodulate:
                xs, _, _ = _reduce_raw(xh, scale=s32)
                gue, _, _ = _reduce_raw(gyh, scale=poste)                       # g d' gy
                _wgrad_into(dwi, xs, gue, up, k, C, Cout, H, W)
            d_w = _wgrad_as_weight(dwi, up, cfg.flipped)
            if demodulate:
                d_w = d_w + w32 * (t1.t() @ (s32 * s32) - 2.0 * (t2.t() @ (s32 * vs32)))[:, :, None, None]
            d_w = d_w.to(cfg.w_dtype)
        return (d_gy, d_x.permute(0, 3, 1, 2) if need_x else None, d_w, d_s.to(cfg.s_dtype) if need_s else None) + no_grads


def modulated_conv2d(x, weight, styles, noise=None, up=1, down=1, padding=0, resample_filter=None, demodulate=True, flip_weight=True, fused_modconv=True):
    """The reference's signature (stylegan2.py:28-40). x: NCHW, contiguous or channels_last, float32 or bfloat16; weight [O, I, k, k] and styles [N, I] may be
    float32 next to a bfloat16 x; noise: [N, 1, Ho, Wo] or one shared [Ho, Wo] plane. The result is channels_last. fused_modconv is accepted and has no
    effect: there is one route here. Supported: k = 1 or 3 with padding = k // 2, down = 1, up = 1, and up = 2 for k = 3 (transposed stride-2 convolution in
    the kernel, then upfirdn2d with gain 4, then the noise: conv2d_resample.py:81-125; resample_filter=None is the identity filter, plain zero insertion).
    First-order gradients; second order (the gradient of <vx, dx> + <vs, ds> for gy, x, styles and weight: path-length regularisation) inside
    style_ops.second_order(generator=True), _ModConvGradFn."""
    N, C, H, W, Cout, k = _validate(x, weight, styles, noise, up, down, padding, resample_filter)
    L.require_gpu(x.device)
    if up == 1:
        return _ModConvFn.apply(x, weight, styles, noise, 1, bool(demodulate), bool(flip_weight))
    # d commutes with the per-channel FIR, so it stays in the kernel's epilogue; the noise comes after the FIR
    core = _ModConvFn.apply(x, weight, styles, None, 2, bool(demodulate), bool(flip_weight))
    y = _upfirdn2d.upfirdn2d(core, resample_filter, padding=_up2_fir_padding(padding, k, resample_filter), gain=up ** 2)
    if noise is not None:
        y = y + noise.to(y.dtype)
    return y.contiguous(memory_format=torch.channels_last)


def modulated_conv2d_act(x, weight, styles, noise=None, up=1, down=1, padding=0, resample_filter=None, demodulate=True, flip_weight=True, fused_modconv=True,
                         bias=None, act="linear", gain=None, clamp=None):
    """bias_act(modulated_conv2d(...), bias, act=act, gain=gain, clamp=clamp) -- a synthesis layer's whole arithmetic -- with the up = 2 tail in one launch.
    up = 1: the convolution kernel (noise in its epilogue) and sg_bias_act, the two launches of the separate operators. up = 2: the transposed convolution to
    the [2H+1, 2W+1] core, then ONE sg_fir_bias_act_nhwc (style_ops/fir_bias_act.py): low-pass, noise, bias, activation, gain and clamp on the fp32
    accumulator, channels-last in and out. noise and bias enter in fp32 there, where the separate operators round both to x's dtype and round the activation
    after the FIR and after the noise. act: 'linear' or 'lrelu' at up = 2. Second order as modulated_conv2d's (the tail's: fir_bias_act._FirBiasActGradFn)."""
    from .bias_act import bias_act
    from ._fir_common import ACTS, MAX_TAPS
    from .fir_bias_act import fir_bias_act
    N, C, H, W, Cout, k = _validate(x, weight, styles, noise, up, down, padding, resample_filter)
    fw, fh = _upfirdn2d._get_filter_size(resample_filter)
    if up == 2 and (act not in ACTS or max(fw, fh) > MAX_TAPS):
        raise NotImplementedError(f"modulated_conv2d_act: act={act!r} with a {fh} x {fw} filter has no fused tail at up=2 "
                                  f"({' / '.join(ACTS)}, at most {MAX_TAPS} x {MAX_TAPS} taps): use modulated_conv2d and bias_act")
    L.require_gpu(x.device)
    if up == 1:
        y = _ModConvFn.apply(x, weight, styles, noise, 1, bool(demodulate), bool(flip_weight))
        return bias_act(y, None if bias is None else bias.to(y.dtype), act=act, gain=gain, clamp=clamp)
    core = _ModConvFn.apply(x, weight, styles, None, 2, bool(demodulate), bool(flip_weight))
    return fir_bias_act(core, resample_filter, _up2_fir_padding(padding, k, resample_filter), noise=noise, bias=bias, act=act, gain=gain, clamp=clamp,
                        filter_gain=up ** 2)
