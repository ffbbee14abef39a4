"""The StyleGAN2 generator networks (Karras et al. 2020, "Analyzing and Improving the Image Quality of StyleGAN", sections 2-4 and appendix B), on the layers of
stylegan2_layers.py. Written from the paper; what is shared with the reference (src/models/stylegan2.py) is the contract its checkpoints and callers need:
constructor and forward argument lists, and the attribute names behind the state_dict keys (`mapping.fc0.weight`, `mapping.w_avg`, `synthesis.b4.const`,
`synthesis.b8.conv0.affine.weight`, `synthesis.b8.torgb.bias`, `synthesis.b8.skip.weight`, ...), registered in the reference's order, so a reference
state_dict loads with strict=True.

    MappingNetwork     z (and an embedded label c), each normalised to unit second moment -> num_layers equalised-lr lrelu layers (lr multiplier 0.01) -> w,
                       broadcast to num_ws rows; tracks w_avg and truncates towards it (w_avg + psi (w - w_avg) on the first `cutoff` rows)
    SynthesisBlock     resolution r: [const | conv0 (up 2)] -> conv1 -> toRGB; architecture 'orig' (one toRGB at the end), 'skip' (every block's RGB
                       added onto the low-pass upsampled image, fp32) or 'resnet' (a 1x1 up-2 skip convolution around conv0 / conv1, both halves scaled by sqrt 1/2)
    SynthesisNetwork   blocks b4 .. b<img_resolution>, channels min(channel_base / r, channel_max); block i reads rows [i0, i0 + num_conv + num_torgb) of ws,
                       consecutive blocks overlapping in the toRGB row
    Generator          mapping -> synthesis, z_dim widened by the InfoGAN codes of MODEL.info_type

use_fp16=True means BFLOAT16 activations here (channels_last): the operators refuse float16. Parameters, styles, noise and the image stay fp32.

Two things are computed differently from a layer-by-layer evaluation, both switchable and both equal to it to rounding:
  * every layer's style affine of a synthesis forward is ONE sg_linear_group_scaled launch (StyleAffineGroupFn) reading its row of ws in place
    (`grouped_styles`; per layer it is a gain multiply, a cast, a bias multiply and an addmm on a [N, w_dim] x [w_dim, C] problem);
  * the up = 2 layers run modulated_conv2d_act, whose FIR + noise + bias + activation tail is one launch (`fused_resample`).
The discriminator (down = 2 convolutions, minibatch standard deviation) is backbones/stylegan2_dis.py; the StyleGAN2 training loop is still to come."""
import ctypes
import math

import torch
from torch import nn

from .. import _lib as L
from ..style_ops.bias_act import bias_act
from ..style_ops.modulated_conv2d import modulated_conv2d
from ..style_ops.upfirdn2d import setup_filter, upsample2d
from .stylegan2_layers import EqualizedConv2dBase, FullyConnectedLayer, SynthesisLayer, ToRGBLayer, _scaled

ACT_DTYPE = torch.bfloat16      # what use_fp16 selects


def normalize_2nd_moment(x, dim=1, eps=1e-8):
    return x * (x.square().mean(dim=dim, keepdim=True) + eps).rsqrt()


class Conv2dLayer(EqualizedConv2dBase):
    """Plain (unmodulated) equalised-lr convolution with optional 2x upsampling: the resnet architecture's skip path. The convolution is the modulated
    kernel with unit styles and no demodulation. Resampling order: a 1x1 kernel convolves first and upsamples the result through the low-pass
    (fewer pixels to convolve), a 3x3 kernel is the transposed stride-2 convolution followed by the low-pass, as in modulated_conv2d."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True, activation="linear", up=1, down=1, resample_filter=[1, 3, 3, 1], conv_clamp=None,
                 channels_last=False, trainable=True):
        if down != 1:
            raise NotImplementedError(f"Conv2dLayer: down={down} is the discriminator's path, which is not implemented (down=1 only)")
        if kernel_size not in (1, 3) or up not in (1, 2):
            raise NotImplementedError(f"Conv2dLayer: kernel_size={kernel_size}, up={up} is not supported (1 or 3; 1 or 2)")
        super().__init__(in_channels, out_channels, kernel_size, bias, activation, up, down, resample_filter, conv_clamp, channels_last, trainable)

    def forward(self, x, gain=1):
        ones = torch.ones((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
        w = self.weight * self.weight_gain
        if self.up == 2 and self.weight.shape[2] == 1:
            y = upsample2d(modulated_conv2d(x, w, ones, demodulate=False), self.resample_filter)
        else:
            y = modulated_conv2d(x, w, ones, up=self.up, padding=self.padding, resample_filter=self.resample_filter, demodulate=False, flip_weight=self.up == 1)
        b = None if self.bias is None else self.bias.to(y.dtype)
        return bias_act(y, b, act=self.activation, gain=self.act_gain * gain, clamp=_scaled(self.conv_clamp, gain))


class MappingNetwork(nn.Module):
    def __init__(self, z_dim, c_dim, w_dim, num_ws, num_layers=8, embed_features=None, layer_features=None, activation="lrelu", lr_multiplier=0.01,
                 w_avg_beta=0.998):
        super().__init__()
        self.z_dim, self.c_dim, self.w_dim, self.num_ws, self.num_layers, self.w_avg_beta = z_dim, c_dim, w_dim, num_ws, num_layers, w_avg_beta
        embed = 0 if c_dim == 0 else (w_dim if embed_features is None else embed_features)
        hidden = w_dim if layer_features is None else layer_features
        widths = [z_dim + embed] + [hidden] * (num_layers - 1) + [w_dim]
        if c_dim > 0:
            self.embed = FullyConnectedLayer(c_dim, embed)
        for i in range(num_layers):
            setattr(self, f"fc{i}", FullyConnectedLayer(widths[i], widths[i + 1], activation=activation, lr_multiplier=lr_multiplier))
        if num_ws is not None and w_avg_beta is not None:
            self.register_buffer("w_avg", torch.zeros(w_dim))

    def forward(self, z, c, truncation_psi=1, truncation_cutoff=None, update_emas=False):
        parts = []
        if self.z_dim > 0:
            if z.dim() != 2 or z.shape[1] != self.z_dim:
                raise AssertionError(f"MappingNetwork: z must be [N, {self.z_dim}], got {tuple(z.shape)}")
            parts.append(normalize_2nd_moment(z.to(torch.float32)))
        if self.c_dim > 0:
            if c.dim() != 2 or c.shape[1] != self.c_dim:
                raise AssertionError(f"MappingNetwork: c must be [N, {self.c_dim}], got {tuple(c.shape)}")
            parts.append(normalize_2nd_moment(self.embed(c.to(torch.float32))))
        x = torch.cat(parts, dim=1)
        for i in range(self.num_layers):
            x = getattr(self, f"fc{i}")(x)
        return self.broadcast_truncate(x, truncation_psi, truncation_cutoff, update_emas)

    def broadcast_truncate(self, x, truncation_psi=1, truncation_cutoff=None, update_emas=False):
        """what follows the layers, on their [N, w_dim] output: the w_avg update, the broadcast to num_ws rows and the truncation (plain torch, any device)"""
        if update_emas and self.w_avg_beta is not None:
            with torch.no_grad():       # w_avg <- beta w_avg + (1 - beta) mean_n w
                self.w_avg.copy_(x.detach().mean(dim=0).lerp(self.w_avg, self.w_avg_beta))
        if self.num_ws is not None:
            x = x.unsqueeze(1).repeat(1, self.num_ws, 1)
        if truncation_psi != 1:
            if self.w_avg_beta is None:
                raise AssertionError("MappingNetwork: truncation needs the tracked w_avg (w_avg_beta=None)")
            if self.num_ws is None or truncation_cutoff is None:
                x = self.w_avg.lerp(x, truncation_psi)
            else:
                x = torch.cat([self.w_avg.lerp(x[:, :truncation_cutoff], truncation_psi), x[:, truncation_cutoff:]], dim=1)
        return x


def style_affine_items(ws, layers, out):
    """the sg_linear_group_scaled table of a synthesis forward. ws: contiguous fp32 [N, num_ws, w_dim]; layers: [(row of ws, affine FullyConnectedLayer, output
    scale)]; out: flat fp32 buffer of N * sum C_i values. Item i reads ws[:, row_i] in place (ldy = num_ws * w_dim) and writes a dense [N, C_i] block.
    Addresses only: works on any device (tests read the table back on the CPU)."""
    N, num_ws, w_dim = ws.shape
    arr = (L.LinearItemScaled * len(layers))()
    off = 0
    for it, (row, fc, oscale) in zip(arr, layers):
        Cn, K = fc.weight.shape
        if K != w_dim or not (0 <= row < num_ws) or fc.bias is None or not fc.weight.is_contiguous():
            raise AssertionError("style_affine_items: an affine layer does not match ws")
        it.w, it.y, it.bias, it.out = fc.weight.data_ptr(), ws.data_ptr() + 4 * row * w_dim, fc.bias.data_ptr(), out.data_ptr() + 4 * off
        it.rows, it.K, it.ldy, it.ldo = Cn, K, num_ws * w_dim, Cn
        it.wscale, it.bscale, it.oscale = fc.weight_gain, fc.bias_gain, oscale
        off += N * Cn
    if off != out.numel():
        raise AssertionError("style_affine_items: the output buffer does not match the layers")
    return arr


class StyleAffineGroupFn(torch.autograd.Function):
    """apply(ws, layers, cache, weight_0, bias_0, weight_1, ...) -> one [N, C_i] styles tensor per layer: oscale_i * affine_i(ws[:, row_i]), all layers in one
    launch (csrc/linear_group.hip). The backward runs layer by layer in plain torch once every layer's gradient has arrived; the saving is on the forward."""

    @staticmethod
    def forward(ctx, ws, layers, cache, *params):
        ws = ws.detach().to(torch.float32).contiguous()
        L.require_gpu(ws.device)
        N = ws.shape[0]
        out = torch.empty(N * sum(fc.weight.shape[0] for _, fc, _ in layers), dtype=torch.float32, device=ws.device)
        arr = style_affine_items(ws, layers, out)
        # the device copy of the table is kept per set of addresses: the caching allocator hands a steady-state forward the same blocks again
        raw = bytes(bytearray(arr))
        tab = cache.get(raw)
        if tab is None:
            if len(cache) >= 16:
                cache.clear()
            tab = cache[raw] = L.upload_bytes(raw, ws.device)
        L.call("sg_linear_group_scaled", tab.data_ptr(), arr, len(layers), N, L.stream())
        outs, off = [], 0
        for _, fc, _ in layers:
            Cn = fc.weight.shape[0]
            outs.append(out[off:off + N * Cn].view(N, Cn))
            off += N * Cn
        ctx.save_for_backward(ws, *params)
        ctx.meta = [(row, fc.weight_gain, fc.bias_gain, oscale) for row, fc, oscale in layers]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *ds):
        ws, *params = ctx.saved_tensors
        dws = torch.zeros_like(ws) if ctx.needs_input_grad[0] else None
        grads = []
        for i, ((row, wg, bg, os_), d) in enumerate(zip(ctx.meta, ds)):
            W = params[2 * i]
            dW = db = None
            if d is not None:
                d = d.to(torch.float32)
                if ctx.needs_input_grad[3 + 2 * i]:
                    dW = (d.t() @ ws[:, row]) * (os_ * wg)
                if ctx.needs_input_grad[4 + 2 * i]:
                    db = d.sum(dim=0) * (os_ * bg)
                if dws is not None:
                    dws[:, row] += (d @ W) * (os_ * wg)
            grads += [dW, db]
        return (dws, None, None) + tuple(grads)


class SynthesisBlock(nn.Module):
    def __init__(self, in_channels, out_channels, w_dim, resolution, img_channels, is_last, architecture="skip", resample_filter=[1, 3, 3, 1], conv_clamp=None,
                 use_fp16=False, fp16_channels_last=False, fused_resample=True, **layer_kwargs):
        if architecture not in ("orig", "skip", "resnet"):
            raise AssertionError(f"SynthesisBlock: architecture {architecture!r} (orig / skip / resnet)")
        super().__init__()
        self.in_channels, self.w_dim, self.resolution, self.img_channels = in_channels, w_dim, resolution, img_channels
        self.is_last, self.architecture, self.use_fp16 = is_last, architecture, use_fp16
        self.channels_last = use_fp16 and fp16_channels_last
        self.fused_resample = fused_resample        # the up = 2 layer's tail as one launch (profiles/stylegan2_gen_bench.txt)
        self.register_buffer("resample_filter", setup_filter(resample_filter))
        self.num_conv = self.num_torgb = 0
        common = dict(w_dim=w_dim, resolution=resolution, conv_clamp=conv_clamp, channels_last=self.channels_last, **layer_kwargs)
        if in_channels == 0:
            self.const = nn.Parameter(torch.randn(out_channels, resolution, resolution))
        else:
            self.conv0 = SynthesisLayer(in_channels, out_channels, up=2, resample_filter=resample_filter, **common)
            self.num_conv += 1
        self.conv1 = SynthesisLayer(out_channels, out_channels, **common)
        self.num_conv += 1
        if is_last or architecture == "skip":
            self.torgb = ToRGBLayer(out_channels, img_channels, w_dim=w_dim, conv_clamp=conv_clamp, channels_last=self.channels_last)
            self.num_torgb += 1
        if in_channels != 0 and architecture == "resnet":
            self.skip = Conv2dLayer(in_channels, out_channels, kernel_size=1, bias=False, up=2, resample_filter=resample_filter, channels_last=self.channels_last)

    def style_layers(self):
        """[(row of this block's ws, affine layer, output scale)] in the order the forward consumes them"""
        seq = ([self.conv0] if self.in_channels != 0 else []) + [self.conv1]
        out = [(i, m.affine, 1.0) for i, m in enumerate(seq)]
        if self.num_torgb:
            out.append((len(seq), self.torgb.affine, self.torgb.weight_gain))
        return out

    def forward(self, x, img, ws, force_fp32=False, fused_modconv=None, update_emas=False, styles=None, **layer_kwargs):
        """styles: this block's style tensors in style_layers() order when the network computed them already; else each layer runs its own affine on ws"""
        if ws.dim() != 3 or tuple(ws.shape[1:]) != (self.num_conv + self.num_torgb, self.w_dim):
            raise AssertionError(f"SynthesisBlock: ws must be [N, {self.num_conv + self.num_torgb}, {self.w_dim}], got {tuple(ws.shape)}")
        rows = iter(ws.unbind(dim=1))
        sty = iter(styles if styles is not None else [None] * (self.num_conv + self.num_torgb))
        low = self.use_fp16 and not force_fp32
        dtype = ACT_DTYPE if low else torch.float32
        if fused_modconv is None:
            fused_modconv = True        # one route here (modulated_conv2d)
        if self.in_channels == 0:
            x = self.const.to(dtype).unsqueeze(0).repeat(ws.shape[0], 1, 1, 1)
        else:
            side = self.resolution // 2
            if tuple(x.shape[1:]) != (self.in_channels, side, side):
                raise AssertionError(f"SynthesisBlock: x must be [N, {self.in_channels}, {side}, {side}], got {tuple(x.shape)}")
            x = x.to(dtype)
        if low:     # the kernels read and write channels-last; an fp32 block keeps whatever layout arrives (every operator here takes both)
            x = x.contiguous(memory_format=torch.channels_last)
        kw = dict(fused_modconv=fused_modconv, **layer_kwargs)
        if self.in_channels == 0:
            x = self.conv1(x, next(rows), styles=next(sty), **kw)
        elif self.architecture == "resnet":
            y = self.skip(x, gain=math.sqrt(0.5))
            x = self.conv0(x, next(rows), styles=next(sty), fused_resample=self.fused_resample, **kw)
            x = self.conv1(x, next(rows), styles=next(sty), gain=math.sqrt(0.5), **kw)
            x = x + y       # (x first: the sum takes its channels-last layout; the skip path arrives NCHW from upsample2d)
            if low:
                x = x.contiguous(memory_format=torch.channels_last)
        else:
            x = self.conv0(x, next(rows), styles=next(sty), fused_resample=self.fused_resample, **kw)
            x = self.conv1(x, next(rows), styles=next(sty), **kw)
        if img is not None:
            side = self.resolution // 2
            if tuple(img.shape[1:]) != (self.img_channels, side, side):
                raise AssertionError(f"SynthesisBlock: img must be [N, {self.img_channels}, {side}, {side}], got {tuple(img.shape)}")
            img = upsample2d(img, self.resample_filter)
        if self.is_last or self.architecture == "skip":
            y = self.torgb(x, next(rows), fused_modconv=fused_modconv, styles=next(sty)).to(torch.float32).contiguous()
            img = y if img is None else img + y
        assert x.dtype == dtype and (img is None or img.dtype == torch.float32)
        return x, img


class SynthesisNetwork(nn.Module):
    def __init__(self, w_dim, img_resolution, img_channels, channel_base=32768, channel_max=512, num_fp16_res=0, grouped_styles=True, **block_kwargs):
        if img_resolution < 4 or img_resolution & (img_resolution - 1):
            raise AssertionError("SynthesisNetwork: img_resolution must be a power of two >= 4")
        super().__init__()
        self.w_dim, self.img_resolution, self.img_channels = w_dim, img_resolution, img_channels
        self.img_resolution_log2 = int(math.log2(img_resolution))
        self.block_resolutions = [2 ** i for i in range(2, self.img_resolution_log2 + 1)]
        self.grouped_styles = grouped_styles        # every layer's style affine of a forward in one launch
        channels = {r: min(channel_base // r, channel_max) for r in self.block_resolutions}
        first_low = max(2 ** (self.img_resolution_log2 + 1 - num_fp16_res), 8)
        self.num_ws = 0
        for r in self.block_resolutions:
            block = SynthesisBlock(channels[r // 2] if r > 4 else 0, channels[r], w_dim=w_dim, resolution=r, img_channels=img_channels,
                                   is_last=r == img_resolution, use_fp16=r >= first_low, **block_kwargs)
            self.num_ws += block.num_conv + (block.num_torgb if r == img_resolution else 0)
            setattr(self, f"b{r}", block)
        self._style_tabs = {}

    def blocks(self):
        return [getattr(self, f"b{r}") for r in self.block_resolutions]

    def block_rows(self):
        """[(first row of ws, number of rows)] per block: a block's toRGB row is the next block's first convolution row"""
        out, i = [], 0
        for b in self.blocks():
            out.append((i, b.num_conv + b.num_torgb))
            i += b.num_conv
        return out

    def style_layers(self):
        """[(row of ws, affine layer, output scale)] of the whole network, block by block"""
        return [(i0 + j, fc, s) for b, (i0, _) in zip(self.blocks(), self.block_rows()) for j, fc, s in b.style_layers()]

    def prefetch_styles(self, ws):
        """every layer's styles in one launch -> one list of style tensors per block"""
        layers = self.style_layers()
        params = [p for _, fc, _ in layers for p in (fc.weight, fc.bias)]
        flat = list(StyleAffineGroupFn.apply(ws, layers, self._style_tabs, *params))
        out = []
        for b in self.blocks():
            n = b.num_conv + b.num_torgb
            out.append(flat[:n])
            flat = flat[n:]
        return out

    def forward(self, ws, **block_kwargs):
        if ws.dim() != 3 or tuple(ws.shape[1:]) != (self.num_ws, self.w_dim):
            raise AssertionError(f"SynthesisNetwork: ws must be [N, {self.num_ws}, {self.w_dim}], got {tuple(ws.shape)}")
        ws = ws.to(torch.float32)
        styles = self.prefetch_styles(ws) if self.grouped_styles else [None] * len(self.block_resolutions)
        x = img = None
        for b, (i0, n), st in zip(self.blocks(), self.block_rows(), styles):
            x, img = b(x, img, ws.narrow(1, i0, n), styles=st, **block_kwargs)
        return img


class Generator(nn.Module):
    def __init__(self, z_dim, c_dim, w_dim, img_resolution, img_channels, MODEL, mapping_kwargs={}, synthesis_kwargs={}):
        super().__init__()
        self.z_dim, self.c_dim, self.w_dim, self.MODEL = z_dim, c_dim, w_dim, MODEL
        self.img_resolution, self.img_channels = img_resolution, img_channels
        info = getattr(MODEL, "info_type", "N/A")       # InfoGAN: the latent carries the discrete / continuous codes behind z
        if info in ("discrete", "both"):
            self.z_dim += MODEL.info_num_discrete_c * MODEL.info_dim_discrete_c
        if info in ("continuous", "both"):
            self.z_dim += MODEL.info_num_conti_c
        self.synthesis = SynthesisNetwork(w_dim=w_dim, img_resolution=img_resolution, img_channels=img_channels, **synthesis_kwargs)
        self.num_ws = self.synthesis.num_ws
        self.mapping = MappingNetwork(z_dim=self.z_dim, c_dim=c_dim, w_dim=w_dim, num_ws=self.num_ws, **mapping_kwargs)

    def forward(self, z, c, eval=False, truncation_psi=1, truncation_cutoff=None, update_emas=False, **synthesis_kwargs):
        ws = self.mapping(z, c, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff, update_emas=update_emas)
        return self.synthesis(ws, update_emas=update_emas, **synthesis_kwargs)
