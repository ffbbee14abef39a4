"""The StyleGAN2 layers around the modulated convolution, written from their definition (Karras et al. 2020, "Analyzing and Improving the Image Quality
of StyleGAN", section 2 and appendix B). What is shared with the reference (src/models/stylegan2.py) is the contract its checkpoints and callers need:
constructor and forward argument lists, and the attribute names behind the state_dict keys (`affine.weight`, `affine.bias`, `weight`, `bias`,
`noise_const`, `noise_strength`, `resample_filter`), so a reference checkpoint loads with strict=True.

    FullyConnectedLayer   y = act( x (g_w W)^T + g_b b ),  g_w = lr_multiplier / sqrt(fan_in), g_b = lr_multiplier  (equalised learning rate: the stored
                          parameters are N(0,1) / lr_multiplier)
    SynthesisLayer        styles = affine(w);  y = clamp( gain * sqrt(2) * lrelu_0.2( modconv(x, W, styles) + strength * noise + b ) )
    ToRGBLayer            styles = affine(w) / sqrt(fan_in);  y = clamp( modconv(x, W, styles, no demodulation) + b )

The convolution is style_ops.modulated_conv2d (csrc/modconv.hip), the activation style_ops.bias_act; the [N, w_dim] x [w_dim, C] affine is torch unless the
caller hands the styles in (backbones/stylegan2.py computes all of a forward's in one launch). The mapping / synthesis networks are backbones/stylegan2.py;
the discriminator is backbones/stylegan2_dis.py; the StyleGAN2 training loop is still to come, and nothing of this file is registered in config_map.BACKBONES."""
import math

import torch
import torch.nn.functional as F
from torch import nn

from ..style_ops.bias_act import activation_funcs, bias_act
from ..style_ops.modulated_conv2d import modulated_conv2d, modulated_conv2d_act
from ..style_ops.upfirdn2d import setup_filter


def _conv_weight(out_channels, in_channels, k, channels_last):
    """unit-normal [O, I, k, k] filter bank; channels_last only picks the memory order of the stored parameter"""
    w = torch.randn(out_channels, in_channels, k, k)
    return nn.Parameter(w.contiguous(memory_format=torch.channels_last) if channels_last else w)


def _scaled(value, gain):
    """an optional clamp bound follows the layer's output gain"""
    return None if value is None else value * gain


class EqualizedConv2dBase(nn.Module):
    """What the generator's Conv2dLayer and the discriminator's DConv2dLayer share: the equalised-lr weight and the bias, parameters or (Freeze-D, trainable=False)
    buffers, the resample filter, and the gains, registered in the order the reference's state_dict lists them. Each subclass refuses what it does not serve
    before it calls this constructor, and has its own forward."""

    def __init__(self, in_channels, out_channels, kernel_size, bias, activation, up, down, resample_filter, conv_clamp, channels_last, trainable):
        super().__init__()
        self.activation, self.up, self.down, self.conv_clamp = activation, up, down, conv_clamp
        self.register_buffer("resample_filter", setup_filter(resample_filter))
        self.padding = kernel_size // 2
        self.weight_gain = 1.0 / math.sqrt(in_channels * kernel_size ** 2)
        self.act_gain = activation_funcs[activation].def_gain
        weight = _conv_weight(out_channels, in_channels, kernel_size, channels_last)
        b = torch.zeros(out_channels) if bias else None
        if trainable:
            self.weight = weight
            self.register_parameter("bias", None if b is None else nn.Parameter(b))
        else:
            self.register_buffer("weight", weight.detach())
            if b is not None:
                self.register_buffer("bias", b)
            else:
                self.bias = None


class FullyConnectedLayer(nn.Module):
    def __init__(self, in_features, out_features, bias=True, activation="linear", lr_multiplier=1, bias_init=0):
        super().__init__()
        self.activation = activation
        self.weight_gain, self.bias_gain = lr_multiplier / math.sqrt(in_features), lr_multiplier
        self.weight = nn.Parameter(torch.randn(out_features, in_features) / lr_multiplier)
        self.register_parameter("bias", nn.Parameter(torch.full((out_features,), float(bias_init))) if bias else None)

    def forward(self, x):
        b = None if self.bias is None else (self.bias * self.bias_gain).to(x.dtype)
        linear = self.activation == "linear"
        y = F.linear(x, (self.weight * self.weight_gain).to(x.dtype), b if linear else None)
        return y if linear else bias_act(y, b, act=self.activation)


class SynthesisLayer(nn.Module):
    def __init__(self, in_channels, out_channels, w_dim, resolution, kernel_size=3, up=1, use_noise=True, activation="lrelu",
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, channels_last=False):
        super().__init__()
        self.resolution, self.up, self.use_noise = resolution, up, use_noise
        self.activation, self.conv_clamp, self.padding = activation, conv_clamp, kernel_size // 2
        self.act_gain = activation_funcs[activation].def_gain
        self.affine = FullyConnectedLayer(w_dim, in_channels, bias_init=1)      # styles start at 1: the layer starts as a plain convolution
        self.weight = _conv_weight(out_channels, in_channels, kernel_size, channels_last)
        self.register_buffer("resample_filter", setup_filter(resample_filter))
        if use_noise:       # (registered in the order the reference's state_dict lists its keys)
            self.noise_strength = nn.Parameter(torch.zeros(()))
            self.register_buffer("noise_const", torch.randn(resolution, resolution))
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def _noise(self, batch, mode, device):
        """per-sample fresh noise ('random'), the stored plane ('const') or none, scaled by the learned strength"""
        if not self.use_noise or mode == "none":
            return None
        plane = self.noise_const if mode == "const" else torch.randn(batch, 1, self.resolution, self.resolution, device=device)
        return plane * self.noise_strength

    def forward(self, x, w, noise_mode="random", fused_modconv=True, gain=1, styles=None, fused_resample=False):
        """styles: this layer's affine(w) when the caller already has it (the synthesis network computes every layer's in one launch); w is then unused.
        fused_resample: run through modulated_conv2d_act, whose up = 2 tail (FIR, noise, bias, activation) is one launch."""
        if noise_mode not in ("random", "const", "none"):
            raise AssertionError(f"SynthesisLayer: noise_mode {noise_mode!r} (random / const / none)")
        side = self.resolution // self.up
        if tuple(x.shape[1:]) != (self.weight.shape[1], side, side):
            raise AssertionError(f"SynthesisLayer: x must be [N, {self.weight.shape[1]}, {side}, {side}], got {tuple(x.shape)}")
        if styles is None:
            styles = self.affine(w)
        # the transposed convolution of up = 2 scatters the taps as stored (a convolution), up = 1 correlates like torch's conv2d
        kw = dict(noise=self._noise(x.shape[0], noise_mode, x.device), up=self.up, padding=self.padding, resample_filter=self.resample_filter,
                  flip_weight=self.up == 1, fused_modconv=fused_modconv)
        if fused_resample:
            return modulated_conv2d_act(x, self.weight, styles, bias=self.bias, act=self.activation, gain=self.act_gain * gain,
                                        clamp=_scaled(self.conv_clamp, gain), **kw)
        y = modulated_conv2d(x, self.weight, styles, **kw)
        return bias_act(y, self.bias.to(y.dtype), act=self.activation, gain=self.act_gain * gain, clamp=_scaled(self.conv_clamp, gain))


class ToRGBLayer(nn.Module):
    def __init__(self, in_channels, out_channels, w_dim, kernel_size=1, conv_clamp=None, channels_last=False):
        super().__init__()
        self.conv_clamp = conv_clamp
        self.weight_gain = 1.0 / math.sqrt(in_channels * kernel_size * kernel_size)     # no demodulation here: the fan-in scale rides on the styles
        self.affine = FullyConnectedLayer(w_dim, in_channels, bias_init=1)
        self.weight = _conv_weight(out_channels, in_channels, kernel_size, channels_last)
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def forward(self, x, w, fused_modconv=True, styles=None):
        """styles: affine(w) * weight_gain when the caller already has it (see SynthesisLayer.forward)"""
        if styles is None:
            styles = self.affine(w) * self.weight_gain
        y = modulated_conv2d(x, self.weight, styles, demodulate=False, fused_modconv=fused_modconv)
        return bias_act(y, self.bias.to(y.dtype), clamp=self.conv_clamp)
