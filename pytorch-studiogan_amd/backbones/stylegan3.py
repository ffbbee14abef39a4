"""The StyleGAN3 generator (Karras et al. 2021, "Alias-Free Generative Adversarial Networks", sections 3-4 and appendices C, F), on this package's operators.
Written from the paper; what is shared with the reference (src/models/stylegan3.py) is the contract its checkpoints and callers need: constructor and forward
argument lists and the attribute names behind the state_dict keys (`synthesis.input.weight`, `synthesis.input.affine.weight`, `synthesis.input.transform`,
`synthesis.L0_36_32.affine.weight`, `...magnitude_ema`, `...up_filter`, `...down_filter`, `mapping.fc0.weight`, `mapping.w_avg`), registered in the
reference's order, so a reference state_dict loads with strict=True.

    SynthesisInput     Fourier features on a sampling grid wider than the image by the margin, rotated / translated by a 4-parameter affine of w and by the
                       user's `transform`, frequencies beyond the band faded out, then a learned channel mix. Small: plain torch.
    SynthesisLayer     magnitude_ema-normalised modulated convolution (full padding: style_ops/modulated_conv2d_full.py) -> bias -> up-sample through a
                       Kaiser low-pass -> leaky ReLU -> down-sample through a second low-pass, cropped to the layer's canvas: style_ops/filtered_lrelu.py,
                       one launch forward and one backward for separable filters. config R (`use_radial_filters`, conv_kernel=1) has a 2-D jinc down filter
                       in its non-critical layers, which runs the operator chain, forward and backward.
    SynthesisNetwork   num_layers layers + ToRGB; cutoff and stopband grow geometrically up to the last num_critical layers, each layer's sampling rate is the
                       power of two that holds its stopband, its canvas that rate plus the margin; layers are named L{idx}_{size}_{channels}.
    Generator          mapping (StyleGAN2's MappingNetwork arithmetic, two layers by default) -> synthesis, z_dim widened by the InfoGAN codes.

use_fp16=True means BFLOAT16 activations here, as in backbones/stylegan2.py: the operators refuse float16. Parameters, styles and the image stay fp32.
The convolution is channels-last and the filtered leaky ReLU plane-wise (NCHW), so each layer copies its activation between the two layouts, twice forward
and twice backward (tools/stylegan3_bench.py reports the share). First-order gradients only through the convolution."""
import math

import numpy as np
import scipy.signal
import scipy.special
import torch
from torch import nn

from ..style_ops.filtered_lrelu import filtered_lrelu
from ..style_ops.modulated_conv2d_full import modulated_conv2d
from . import stylegan2 as _sg2
from .stylegan2_layers import FullyConnectedLayer as _FC2

ACT_DTYPE = _sg2.ACT_DTYPE      # what use_fp16 selects


class FullyConnectedLayer(_FC2):
    """the StyleGAN2 layer's arithmetic behind the StyleGAN3 argument list (weight_init scales the initial weights, bias_init may be a vector)"""

    def __init__(self, in_features, out_features, activation="linear", bias=True, lr_multiplier=1, weight_init=1, bias_init=0):
        super().__init__(in_features, out_features, bias=bias, activation=activation, lr_multiplier=lr_multiplier)
        self.in_features, self.out_features = in_features, out_features
        with torch.no_grad():
            self.weight.mul_(weight_init)
            if bias:
                self.bias.copy_(torch.as_tensor(np.broadcast_to(np.asarray(bias_init, dtype=np.float32), [out_features]).copy()) / lr_multiplier)


class MappingNetwork(_sg2.MappingNetwork):
    """StyleGAN2's mapping network with StyleGAN3's argument list: two layers by default, the label embedding and every layer w_dim wide"""

    def __init__(self, z_dim, c_dim, w_dim, num_ws, num_layers=2, lr_multiplier=0.01, w_avg_beta=0.998):
        super().__init__(z_dim, c_dim, w_dim, num_ws, num_layers=num_layers, lr_multiplier=lr_multiplier, w_avg_beta=w_avg_beta)

    def forward(self, z, c, truncation_psi=1, truncation_cutoff=None, update_emas=False):
        return super().forward(z, c, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff, update_emas=update_emas)


def _size2(v):
    return np.broadcast_to(np.asarray(v), [2])


class SynthesisInput(nn.Module):
    def __init__(self, w_dim, channels, size, sampling_rate, bandwidth):
        super().__init__()
        self.w_dim, self.channels, self.size, self.sampling_rate, self.bandwidth = w_dim, channels, _size2(size), sampling_rate, bandwidth
        # frequencies inside a disc of radius `bandwidth`: a Gaussian draw g keeps its direction and gets the length exp(-|g|^2 / 4); phases in [-1/2, 1/2)
        freqs = torch.randn(channels, 2)
        radii = freqs.square().sum(dim=1, keepdim=True).sqrt()
        freqs = freqs / (radii * radii.square().exp().pow(0.25)) * bandwidth
        phases = torch.rand(channels) - 0.5
        self.weight = nn.Parameter(torch.randn(channels, channels))
        self.affine = FullyConnectedLayer(w_dim, 4, weight_init=0, bias_init=[1, 0, 0, 0])      # starts as the identity: (cos, sin, tx, ty) = (1, 0, 0, 0)
        self.register_buffer("transform", torch.eye(3))     # the user's inverse transform of the image
        self.register_buffer("freqs", freqs)
        self.register_buffer("phases", phases)

    def forward(self, w):
        N = w.shape[0]
        t = self.affine(w)
        t = t / t[:, :2].norm(dim=1, keepdim=True)          # a unit (cos, sin) and the translation in its units
        cs, sn, tx, ty = t.unbind(dim=1)
        zero, one = torch.zeros_like(cs), torch.ones_like(cs)
        rot = torch.stack([cs, -sn, zero, sn, cs, zero, zero, zero, one], dim=1).reshape(N, 3, 3)
        trans = torch.stack([one, zero, -tx, zero, one, -ty, zero, zero, one], dim=1).reshape(N, 3, 3)
        m = rot @ trans @ self.transform.unsqueeze(0)       # rotate the image, then translate it, then the user's transform
        # a transform of the image plane acts on a plane wave sin(2 pi (f . p + phase)) through its frequency and phase
        phases = self.phases.unsqueeze(0) + (self.freqs.unsqueeze(0) @ m[:, :2, 2:]).squeeze(2)
        freqs = self.freqs.unsqueeze(0) @ m[:, :2, :2]
        # fade what the transform pushed beyond the band, linearly down to zero at the Nyquist rate
        amps = (1 - (freqs.norm(dim=2) - self.bandwidth) / (self.sampling_rate / 2 - self.bandwidth)).clamp(0, 1)
        theta = torch.zeros(2, 3, device=w.device)
        theta[0, 0] = 0.5 * self.size[0] / self.sampling_rate
        theta[1, 1] = 0.5 * self.size[1] / self.sampling_rate
        grid = torch.nn.functional.affine_grid(theta.unsqueeze(0), [1, 1, int(self.size[1]), int(self.size[0])], align_corners=False)     # [1, H, W, 2]
        x = (grid.unsqueeze(3) @ freqs.permute(0, 2, 1).unsqueeze(1).unsqueeze(2)).squeeze(3)       # [N, H, W, C]
        x = torch.sin((x + phases.unsqueeze(1).unsqueeze(2)) * (2 * math.pi)) * amps.unsqueeze(1).unsqueeze(2)
        x = x @ (self.weight / math.sqrt(self.channels)).t()
        return x.permute(0, 3, 1, 2)


def design_lowpass_filter(numtaps, cutoff, width, fs, radial=False):
    """a Kaiser-windowed low-pass of `numtaps` taps at sampling rate fs: cutoff frequency `cutoff`, transition band `width`. One tap: None (identity).
    Separable: the windowed sinc (scipy.signal.firwin), a float32 vector. radial: the 2-D jinc, J1(2 pi fc r) / (pi r), the ideal circular low-pass, under
    the outer product of the Kaiser window whose beta gives the same attenuation, normalised to unit sum: a float32 [numtaps, numtaps] matrix."""
    if numtaps < 1:
        raise AssertionError("design_lowpass_filter: numtaps must be >= 1")
    if numtaps == 1:
        return None
    if not radial:
        return torch.as_tensor(scipy.signal.firwin(numtaps=numtaps, cutoff=cutoff, width=width, fs=fs), dtype=torch.float32)
    pos = (np.arange(numtaps) - (numtaps - 1) / 2) / fs
    r = np.hypot(*np.meshgrid(pos, pos))
    f = scipy.special.j1(2 * cutoff * (np.pi * r)) / (np.pi * r)
    win = np.kaiser(numtaps, scipy.signal.kaiser_beta(scipy.signal.kaiser_atten(numtaps, width / (fs / 2))))
    f = f * np.outer(win, win)
    return torch.as_tensor(f / np.sum(f), dtype=torch.float32)


class SynthesisLayer(nn.Module):
    def __init__(self, w_dim, is_torgb, is_critically_sampled, use_fp16, in_channels, out_channels, in_size, out_size, in_sampling_rate, out_sampling_rate,
                 in_cutoff, out_cutoff, in_half_width, out_half_width, conv_kernel=3, filter_size=6, lrelu_upsampling=2, use_radial_filters=False,
                 conv_clamp=256, magnitude_ema_beta=0.999):
        super().__init__()
        self.w_dim, self.is_torgb, self.is_critically_sampled, self.use_fp16 = w_dim, is_torgb, is_critically_sampled, use_fp16
        self.in_channels, self.out_channels = in_channels, out_channels
        self.in_size, self.out_size = _size2(in_size), _size2(out_size)
        self.in_sampling_rate, self.out_sampling_rate = in_sampling_rate, out_sampling_rate
        # the non-linearity runs at lrelu_upsampling times the larger of the two rates (ToRGB has none)
        self.tmp_sampling_rate = max(in_sampling_rate, out_sampling_rate) * (1 if is_torgb else lrelu_upsampling)
        self.in_cutoff, self.out_cutoff, self.in_half_width, self.out_half_width = in_cutoff, out_cutoff, in_half_width, out_half_width
        self.conv_kernel = 1 if is_torgb else conv_kernel
        self.conv_clamp, self.magnitude_ema_beta = conv_clamp, magnitude_ema_beta

        self.affine = FullyConnectedLayer(w_dim, in_channels, bias_init=1)
        self.weight = nn.Parameter(torch.randn(out_channels, in_channels, self.conv_kernel, self.conv_kernel))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.register_buffer("magnitude_ema", torch.ones([]))

        self.up_factor = int(np.rint(self.tmp_sampling_rate / in_sampling_rate))
        self.down_factor = int(np.rint(self.tmp_sampling_rate / out_sampling_rate))
        if in_sampling_rate * self.up_factor != self.tmp_sampling_rate or out_sampling_rate * self.down_factor != self.tmp_sampling_rate:
            raise AssertionError("SynthesisLayer: the sampling rates are no integer factors apart")
        self.up_taps = filter_size * self.up_factor if self.up_factor > 1 and not is_torgb else 1
        self.down_taps = filter_size * self.down_factor if self.down_factor > 1 and not is_torgb else 1
        self.down_radial = use_radial_filters and not is_critically_sampled
        self.register_buffer("up_filter", design_lowpass_filter(self.up_taps, in_cutoff, in_half_width * 2, self.tmp_sampling_rate))
        self.register_buffer("down_filter", design_lowpass_filter(self.down_taps, out_cutoff, out_half_width * 2, self.tmp_sampling_rate, radial=self.down_radial))

        # padding of the up-sampled signal so that out_size samples come out: what the output needs before decimation, minus what the up-sampled
        # (full-padding) convolution result supplies, plus what the two filters consume; split so that sample positions stay symmetric (appendix C.3)
        total = (self.out_size - 1) * self.down_factor + 1 - (self.in_size + self.conv_kernel - 1) * self.up_factor + self.up_taps + self.down_taps - 2
        lo = (total + self.up_factor) // 2
        hi = total - lo
        self.padding = [int(lo[0]), int(hi[0]), int(lo[1]), int(hi[1])]

    design_lowpass_filter = staticmethod(design_lowpass_filter)

    def forward(self, x, w, noise_mode="random", force_fp32=False, update_emas=False):
        if noise_mode not in ("random", "const", "none"):       # (unused: StyleGAN3 has no noise inputs)
            raise AssertionError(f"SynthesisLayer: noise_mode {noise_mode!r}")
        if tuple(x.shape[1:]) != (self.in_channels, int(self.in_size[1]), int(self.in_size[0])):
            raise AssertionError(f"SynthesisLayer: x must be [N, {self.in_channels}, {int(self.in_size[1])}, {int(self.in_size[0])}], got {tuple(x.shape)}")
        if tuple(w.shape) != (x.shape[0], self.w_dim):
            raise AssertionError(f"SynthesisLayer: w must be [{x.shape[0]}, {self.w_dim}], got {tuple(w.shape)}")
        if update_emas:     # the running mean square of the layer's input; its rsqrt normalises the input (through the convolution's post-scale)
            with torch.no_grad():
                cur = x.detach().to(torch.float32).square().mean()
                self.magnitude_ema.copy_(cur.lerp(self.magnitude_ema, self.magnitude_ema_beta))
        input_gain = self.magnitude_ema.rsqrt()
        styles = self.affine(w)
        if self.is_torgb:
            styles = styles * (1 / math.sqrt(self.in_channels * self.conv_kernel ** 2))
        dtype = ACT_DTYPE if (self.use_fp16 and not force_fp32 and x.is_cuda) else torch.float32
        x = modulated_conv2d(x=x.to(dtype), w=self.weight, s=styles, padding=self.conv_kernel - 1, demodulate=not self.is_torgb, input_gain=input_gain)
        x = filtered_lrelu(x=x, fu=self.up_filter, fd=self.down_filter, b=self.bias.to(x.dtype), up=self.up_factor, down=self.down_factor, padding=self.padding,
                           gain=1 if self.is_torgb else math.sqrt(2), slope=1 if self.is_torgb else 0.2, clamp=self.conv_clamp)
        if tuple(x.shape[1:]) != (self.out_channels, int(self.out_size[1]), int(self.out_size[0])) or x.dtype != dtype:
            raise AssertionError(f"SynthesisLayer: unexpected output {tuple(x.shape)} {x.dtype}")
        return x


class SynthesisNetwork(nn.Module):
    def __init__(self, w_dim, img_resolution, img_channels, channel_base=32768, channel_max=512, num_layers=14, num_critical=2, first_cutoff=2,
                 first_stopband=2 ** 2.1, last_stopband_rel=2 ** 0.3, margin_size=10, output_scale=0.25, num_fp16_res=4, **layer_kwargs):
        super().__init__()
        self.w_dim, self.num_ws, self.img_resolution, self.img_channels = w_dim, num_layers + 2, img_resolution, img_channels
        self.num_layers, self.num_critical, self.margin_size, self.output_scale, self.num_fp16_res = num_layers, num_critical, margin_size, output_scale, num_fp16_res

        # cutoff f_c and minimum stopband f_t per layer: geometric from the first layer's to the image's, reached num_critical layers before the end
        last_cutoff = img_resolution / 2
        last_stopband = last_cutoff * last_stopband_rel
        expo = np.minimum(np.arange(num_layers + 1) / (num_layers - num_critical), 1)
        cutoffs = first_cutoff * (last_cutoff / first_cutoff) ** expo
        stopbands = first_stopband * (last_stopband / first_stopband) ** expo
        # sampling rate: the power of two that holds twice the stopband, at most the image's; the transition band gets whatever the rate leaves
        rates = np.exp2(np.ceil(np.log2(np.minimum(stopbands * 2, img_resolution))))
        half_widths = np.maximum(stopbands, rates / 2) - cutoffs
        sizes = rates + margin_size * 2
        sizes[-2:] = img_resolution
        channels = np.rint(np.minimum((channel_base / 2) / cutoffs, channel_max))
        channels[-1] = img_channels

        self.input = SynthesisInput(w_dim=w_dim, channels=int(channels[0]), size=int(sizes[0]), sampling_rate=rates[0], bandwidth=cutoffs[0])
        self.layer_names = []
        for i in range(num_layers + 1):
            p = max(i - 1, 0)
            layer = SynthesisLayer(w_dim=w_dim, is_torgb=i == num_layers, is_critically_sampled=i >= num_layers - num_critical,
                                   use_fp16=bool(rates[i] * 2 ** num_fp16_res > img_resolution), in_channels=int(channels[p]), out_channels=int(channels[i]),
                                   in_size=int(sizes[p]), out_size=int(sizes[i]), in_sampling_rate=int(rates[p]), out_sampling_rate=int(rates[i]),
                                   in_cutoff=cutoffs[p], out_cutoff=cutoffs[i], in_half_width=half_widths[p], out_half_width=half_widths[i], **layer_kwargs)
            name = f"L{i}_{layer.out_size[0]}_{layer.out_channels}"
            setattr(self, name, layer)
            self.layer_names.append(name)

    def forward(self, ws, **layer_kwargs):
        if ws.dim() != 3 or tuple(ws.shape[1:]) != (self.num_ws, self.w_dim):
            raise AssertionError(f"SynthesisNetwork: ws must be [N, {self.num_ws}, {self.w_dim}], got {tuple(ws.shape)}")
        rows = ws.to(torch.float32).unbind(dim=1)
        x = self.input(rows[0])
        for name, w in zip(self.layer_names, rows[1:]):
            x = getattr(self, name)(x, w, **layer_kwargs)
        if self.output_scale != 1:
            x = x * self.output_scale
        if tuple(x.shape[1:]) != (self.img_channels, self.img_resolution, self.img_resolution):
            raise AssertionError(f"SynthesisNetwork: unexpected image {tuple(x.shape)}")
        return x.to(torch.float32)


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
