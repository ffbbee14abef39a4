"""The StyleGAN2 discriminator (Karras et al. 2020, "Analyzing and Improving the Image Quality of StyleGAN", section 4 and appendix B; the minibatch standard
deviation of Karras et al. 2018), with the conditioning heads StudioGAN puts on it. Written from the papers; what is shared with the reference
(src/models/stylegan2.py) is the contract its checkpoints and callers need: constructor and forward argument lists, the attribute names behind the
state_dict keys (`b32.fromrgb.weight`, `b16.conv1.resample_filter`, `b4.fc.bias`, `linear1.weight`, `embedding.fc0.weight`, ...) in the reference's
registration order, with Freeze-D layers (`freeze_layers`) as buffers, so a reference state_dict loads with strict=True; and the twelve-key dict the forward returns.

    DConv2dLayer            equalised-lr convolution, up = 1, down 1 or 2. down = 2 with a 3x3 kernel: 4x4 low-pass (pad 2) at full resolution, then the stride-2
                            convolution; with a 1x1 kernel: decimating low-pass (pad 1), then the convolution on the small map. Then bias, activation, gain, clamp.
    DiscriminatorBlock      resolution r -> r / 2: [fromrgb] -> conv0 -> conv1 (down 2); 'skip' feeds every block the low-passed image, 'resnet' adds a 1x1
                            down-2 skip convolution around conv0 / conv1, both halves scaled by sqrt 1/2
    MinibatchStdLayer       style_ops.minibatch_std (csrc/mbstd.hip): one launch each way
    DiscriminatorEpilogue   4x4: [fromrgb] -> minibatch std -> conv -> fc; always float32
    Discriminator           blocks b<img_resolution> .. b8, epilogue b4, and the heads of d_cond_mtd (W/O, AC, SPD, 2C, D2DCE, MH, MD), aux_cls_type
                            (TAC, ADC) and MODEL.info_type

use_fp16=True means BFLOAT16 channels-last activations, as in the generator; fp16_channels_last is accepted and has no effect. Parameters and the epilogue stay fp32.

What is computed differently from a layer-by-layer evaluation (`fused_down`, switchable, equal to rounding): conv0 writes its RAW output and the head of conv1 is
ONE sg_act_fir_nhwc launch (style_ops/act_fir.py) that applies conv0's bias, lrelu, gain and clamp to each value as it loads it into the low-pass: the activated
full-resolution map, the largest tensor of the block, is never stored, and nothing changes layout between the two convolutions. The resnet skip's decimating
low-pass is a plain launch of the same kernel with the sqrt 1/2 of that half folded into the filter gain. With fused_down=False every layer is
conv2d_resample -> bias_act, the FIR through upfirdn2d on NCHW copies. Second-order gradients (R1: losses.stylegan_cal_r1_reg)
exist inside style_ops.second_order() and are refused outside it."""
import math

import torch
from torch import nn
from torch.nn import functional as F

from ..style_ops._fir_common import ACTS, MAX_TAPS, down2_padding
from ..style_ops.act_fir import act_fir
from ..style_ops.bias_act import bias_act
from ..style_ops.conv2d_resample import conv2d_plain, conv2d_resample
from ..style_ops.minibatch_std import minibatch_std
from ..style_ops.upfirdn2d import _get_filter_size, downsample2d, setup_filter
from .stylegan2 import ACT_DTYPE, MappingNetwork
from .stylegan2_layers import EqualizedConv2dBase, FullyConnectedLayer, _scaled


class DConv2dLayer(EqualizedConv2dBase):
    """The reference's Conv2dLayer for up = 1 (the generator's Conv2dLayer keeps refusing down = 2). forward(x, gain) is the whole layer; `raw` and `epilogue`
    are its two halves, which DiscriminatorBlock uses to move this layer's epilogue into the head of the next one."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True, activation="linear", up=1, down=1, resample_filter=[1, 3, 3, 1], conv_clamp=None,
                 channels_last=False, trainable=True):
        if up != 1:
            raise NotImplementedError(f"DConv2dLayer: up={up} is the generator's path (backbones.stylegan2.Conv2dLayer)")
        if kernel_size not in (1, 3) or down not in (1, 2):
            raise NotImplementedError(f"DConv2dLayer: kernel_size={kernel_size}, down={down} is not supported (1 or 3; 1 or 2)")
        super().__init__(in_channels, out_channels, kernel_size, bias, activation, up, down, resample_filter, conv_clamp, channels_last, trainable)

    def epilogue(self, gain=1):
        """what follows the convolution, as keyword arguments of bias_act / act_fir"""
        return dict(bias=self.bias, act=self.activation, gain=self.act_gain * gain, clamp=_scaled(self.conv_clamp, gain))

    def fusable_head(self):
        """can the epilogue of the layer in front ride in this layer's FIR? (a down = 2 layer with a filter the kernel takes)"""
        fw, fh = _get_filter_size(self.resample_filter)
        return self.down == 2 and max(fw, fh) <= MAX_TAPS

    def raw(self, x, fused=True, head=None, filter_gain=1.0):
        """the convolution with its resampling, before bias and activation. head: epilogue() of the layer whose RAW output x is, applied on the load side of
        this layer's low-pass (needs fusable_head()); filter_gain scales the low-pass (a linear layer's output gain may ride there)."""
        w = self.weight * self.weight_gain
        if self.down == 1:
            if head is not None or filter_gain != 1.0:
                raise AssertionError("DConv2dLayer: only a down = 2 layer has a head to fuse into")
            return conv2d_plain(x, w, 1)
        if not (fused and self.fusable_head()):
            if head is not None or filter_gain != 1.0:
                raise AssertionError("DConv2dLayer: this layer's resampling is not fused")
            return conv2d_resample(x, w, f=self.resample_filter, down=2, padding=self.padding, fused=False)
        k = self.weight.shape[2]
        head = dict(head or {})
        if head.get("bias") is not None:
            head["bias"] = head["bias"].to(torch.float32)
        x = act_fir(x, self.resample_filter, down2_padding(self.resample_filter, self.padding), down=2 if k == 1 else 1, filter_gain=filter_gain, **head)
        return conv2d_plain(x, w, 1 if k == 1 else 2)

    def finish(self, y, gain=1):
        e = self.epilogue(gain)
        if e["bias"] is not None:
            e["bias"] = e["bias"].to(y.dtype)
        return bias_act(y, e.pop("bias"), **e)

    def forward(self, x, gain=1, fused=True):
        """fused: a down = 2 layer's low-pass runs channels-last through sg_act_fir_nhwc (conv2d_resample's own default); False: through upfirdn2d"""
        return self.finish(self.raw(x, fused=fused), gain)


class DiscriminatorBlock(nn.Module):
    def __init__(self, in_channels, tmp_channels, out_channels, resolution, img_channels, first_layer_idx, architecture="resnet", activation="lrelu",
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, use_fp16=False, fp16_channels_last=False, freeze_layers=0, fused_down=True):
        if in_channels not in (0, tmp_channels):
            raise AssertionError("DiscriminatorBlock: in_channels must be 0 (first block) or tmp_channels")
        if architecture not in ("orig", "skip", "resnet"):
            raise AssertionError(f"DiscriminatorBlock: architecture {architecture!r} (orig / skip / resnet)")
        super().__init__()
        self.in_channels, self.resolution, self.img_channels, self.first_layer_idx = in_channels, resolution, img_channels, first_layer_idx
        self.architecture, self.use_fp16 = architecture, use_fp16
        self.channels_last = use_fp16 and fp16_channels_last      # (kept as an attribute; nothing reads it: low-precision blocks are always channels-last)
        self.fused_down = fused_down        # conv1's head (and the resnet skip's decimation) as one launch (profiles/stylegan2_dis_bench.txt)
        self.register_buffer("resample_filter", setup_filter(resample_filter))
        self.num_layers = 0

        def trainable():        # Freeze-D: the first `freeze_layers` layers of the network, counted in construction order, are buffers
            self.num_layers += 1
            return first_layer_idx + self.num_layers - 1 >= freeze_layers

        if in_channels == 0 or architecture == "skip":
            self.fromrgb = DConv2dLayer(img_channels, tmp_channels, kernel_size=1, activation=activation, trainable=trainable(), conv_clamp=conv_clamp)
        self.conv0 = DConv2dLayer(tmp_channels, tmp_channels, kernel_size=3, activation=activation, trainable=trainable(), conv_clamp=conv_clamp)
        self.conv1 = DConv2dLayer(tmp_channels, out_channels, kernel_size=3, activation=activation, down=2, trainable=trainable(),
                                  resample_filter=resample_filter, conv_clamp=conv_clamp)
        if architecture == "resnet":
            self.skip = DConv2dLayer(tmp_channels, out_channels, kernel_size=1, bias=False, down=2, trainable=trainable(), resample_filter=resample_filter)

    def _head_fusable(self):
        return self.fused_down and self.conv1.fusable_head() and self.conv0.activation in ACTS

    def forward(self, x, img, force_fp32=False):
        low = self.use_fp16 and not force_fp32
        dtype = ACT_DTYPE if low else torch.float32
        side = self.resolution
        if x is not None:
            if tuple(x.shape[1:]) != (self.in_channels, side, side):
                raise AssertionError(f"DiscriminatorBlock: x must be [N, {self.in_channels}, {side}, {side}], got {tuple(x.shape)}")
            x = x.to(dtype)
        if self.in_channels == 0 or self.architecture == "skip":
            if tuple(img.shape[1:]) != (self.img_channels, side, side):
                raise AssertionError(f"DiscriminatorBlock: img must be [N, {self.img_channels}, {side}, {side}], got {tuple(img.shape)}")
            img = img.to(dtype)
            y = self.fromrgb(img)
            x = y if x is None else x + y
            img = downsample2d(img, self.resample_filter) if self.architecture == "skip" else None
        if low:
            x = x.contiguous(memory_format=torch.channels_last)
        g = math.sqrt(0.5) if self.architecture == "resnet" else 1
        y = None
        if self.architecture == "resnet":
            if self.fused_down and self.skip.fusable_head():    # linear, no bias, no clamp: the half's gain rides on the filter
                y = self.skip.raw(x, filter_gain=g)
            else:
                y = self.skip(x, gain=g, fused=self.fused_down)
        if self._head_fusable():
            x = self.conv1.finish(self.conv1.raw(self.conv0.raw(x), head=self.conv0.epilogue()), gain=g)
        else:
            x = self.conv1(self.conv0(x), gain=g, fused=self.fused_down)
        if y is not None:
            x = y + x
        assert x.dtype == dtype
        return x, img


class MinibatchStdLayer(nn.Module):
    def __init__(self, group_size, num_channels=1):
        super().__init__()
        self.group_size, self.num_channels = group_size, num_channels

    def forward(self, x):
        return minibatch_std(x, self.group_size, self.num_channels)


class DiscriminatorEpilogue(nn.Module):
    def __init__(self, in_channels, cmap_dim, resolution, img_channels, architecture="resnet", mbstd_group_size=4, mbstd_num_channels=1, activation="lrelu",
                 conv_clamp=None):
        if architecture not in ("orig", "skip", "resnet"):
            raise AssertionError(f"DiscriminatorEpilogue: architecture {architecture!r} (orig / skip / resnet)")
        super().__init__()
        self.in_channels, self.cmap_dim, self.resolution, self.img_channels, self.architecture = in_channels, cmap_dim, resolution, img_channels, architecture
        if architecture == "skip":
            self.fromrgb = DConv2dLayer(img_channels, in_channels, kernel_size=1, activation=activation)
        self.mbstd = MinibatchStdLayer(group_size=mbstd_group_size, num_channels=mbstd_num_channels) if mbstd_num_channels > 0 else None
        self.conv = DConv2dLayer(in_channels + mbstd_num_channels, in_channels, kernel_size=3, activation=activation, conv_clamp=conv_clamp)
        self.fc = FullyConnectedLayer(in_channels * resolution ** 2, in_channels, activation=activation)

    def forward(self, x, img, force_fp32=False):
        side = self.resolution
        if tuple(x.shape[1:]) != (self.in_channels, side, side):
            raise AssertionError(f"DiscriminatorEpilogue: x must be [N, {self.in_channels}, {side}, {side}], got {tuple(x.shape)}")
        x = x.to(torch.float32)
        if self.architecture == "skip":
            if tuple(img.shape[1:]) != (self.img_channels, side, side):
                raise AssertionError(f"DiscriminatorEpilogue: img must be [N, {self.img_channels}, {side}, {side}], got {tuple(img.shape)}")
            x = x + self.fromrgb(img.to(torch.float32))
        if self.mbstd is not None:
            x = self.mbstd(x)
        x = self.conv(x)
        return self.fc(x.flatten(1))        # (flatten follows the logical NCHW order whatever the memory layout: the fc weight is the reference's)


class Discriminator(nn.Module):
    def __init__(self, c_dim, img_resolution, img_channels, architecture="resnet", channel_base=32768, channel_max=512, num_fp16_res=0, conv_clamp=None,
                 cmap_dim=None, d_cond_mtd=None, aux_cls_type=None, d_embed_dim=None, num_classes=None, normalize_d_embed=None, block_kwargs={},
                 mapping_kwargs={}, epilogue_kwargs={}, MODEL=None):
        if img_resolution < 8 or img_resolution & (img_resolution - 1):
            raise AssertionError("Discriminator: img_resolution must be a power of two >= 8")
        if d_cond_mtd == "PD":      # the reference's forward reads a self.embedding that its constructor never creates on this branch
            raise NotImplementedError("Discriminator: d_cond_mtd = PD is not supported (the reference has no working projection head on this backbone)")
        if d_cond_mtd not in ("W/O", "AC", "SPD", "2C", "D2DCE", "MH", "MD"):
            raise NotImplementedError(f"Discriminator: d_cond_mtd = {d_cond_mtd!r}")
        super().__init__()
        self.c_dim, self.img_resolution, self.img_channels, self.cmap_dim = c_dim, img_resolution, img_channels, cmap_dim
        self.d_cond_mtd, self.aux_cls_type, self.num_classes, self.normalize_d_embed = d_cond_mtd, aux_cls_type, num_classes, normalize_d_embed
        self.img_resolution_log2 = int(math.log2(img_resolution))
        self.block_resolutions = [2 ** i for i in range(self.img_resolution_log2, 2, -1)]
        self.MODEL = MODEL
        channels = {r: min(channel_base // r, channel_max) for r in self.block_resolutions + [4]}
        first_low = max(2 ** (self.img_resolution_log2 + 1 - num_fp16_res), 8)
        if self.cmap_dim is None:
            self.cmap_dim = channels[4]
        if c_dim == 0:
            self.cmap_dim = 0
        common = dict(img_channels=img_channels, architecture=architecture, conv_clamp=conv_clamp)
        layer_idx = 0
        for r in self.block_resolutions:
            block = DiscriminatorBlock(channels[r] if r < img_resolution else 0, channels[r], channels[r // 2], resolution=r, first_layer_idx=layer_idx,
                                       use_fp16=r >= first_low, **block_kwargs, **common)
            setattr(self, f"b{r}", block)
            layer_idx += block.num_layers
        self.b4 = DiscriminatorEpilogue(channels[4], cmap_dim=self.cmap_dim, resolution=4, **epilogue_kwargs, **common)
        feat = channels[4]
        # the adversarial head: one logit, or the multi-hinge / multi-discriminator logits, or the embedding the mapped label is projected on (SPD)
        adv_out = {"MH": lambda: 1 + num_classes, "MD": lambda: num_classes, "SPD": lambda: 1 if self.cmap_dim == 0 else self.cmap_dim}.get(d_cond_mtd, lambda: 1)()
        self.linear1 = FullyConnectedLayer(feat, adv_out, bias=True)
        if aux_cls_type == "ADC":       # real and fake copies of every class
            num_classes, c_dim = num_classes * 2, c_dim * 2
        embed = dict(z_dim=0, c_dim=c_dim, w_dim=d_embed_dim, num_ws=None, w_avg_beta=None, num_layers=1, **mapping_kwargs)
        if d_cond_mtd == "AC":
            self.linear2 = FullyConnectedLayer(feat, num_classes, bias=False)
        elif d_cond_mtd == "SPD":
            self.mapping = MappingNetwork(z_dim=0, c_dim=c_dim, w_dim=self.cmap_dim, num_ws=None, w_avg_beta=None, **mapping_kwargs)
        elif d_cond_mtd in ("2C", "D2DCE"):
            self.linear2 = FullyConnectedLayer(feat, d_embed_dim, bias=True)
            self.embedding = MappingNetwork(**embed)
        if aux_cls_type == "TAC":
            if d_cond_mtd == "AC":
                self.linear_mi = FullyConnectedLayer(feat, num_classes, bias=False)
            elif d_cond_mtd in ("2C", "D2DCE"):
                self.linear_mi = FullyConnectedLayer(feat, d_embed_dim, bias=True)
                self.embedding_mi = MappingNetwork(**embed)
            else:
                raise NotImplementedError("Discriminator: aux_cls_type = TAC needs d_cond_mtd AC, 2C or D2DCE")
        info = getattr(MODEL, "info_type", "N/A")
        if info in ("discrete", "both"):
            self.info_discrete_linear = FullyConnectedLayer(feat, MODEL.info_num_discrete_c * MODEL.info_dim_discrete_c, bias=False)
        if info in ("continuous", "both"):
            self.info_conti_mu_linear = FullyConnectedLayer(feat, MODEL.info_num_conti_c, bias=False)
            self.info_conti_var_linear = FullyConnectedLayer(feat, MODEL.info_num_conti_c, bias=False)

    def forward(self, img, label, eval=False, adc_fake=False, update_emas=False, **block_kwargs):
        x = None
        for r in self.block_resolutions:
            x, img = getattr(self, f"b{r}")(x, img, **block_kwargs)
        h = self.b4(x, img)
        out = dict.fromkeys(("h", "adv_output", "embed", "proxy", "cls_output", "label", "mi_embed", "mi_proxy", "mi_cls_output", "info_discrete_c_logits",
                             "info_conti_mu", "info_conti_var"))
        cond, adc = self.d_cond_mtd, self.aux_cls_type == "ADC"
        adv = None if cond == "SPD" else torch.squeeze(self.linear1(h))
        if adc:     # odd labels are the fake copies of the classes, even ones the real copies
            label = label * 2 + 1 if adc_fake else label * 2
        onehot = F.one_hot(label, self.num_classes * 2 if adc else self.num_classes)
        info = getattr(self.MODEL, "info_type", "N/A")
        if info in ("discrete", "both"):
            out["info_discrete_c_logits"] = self.info_discrete_linear(h)
        if info in ("continuous", "both"):
            out["info_conti_mu"] = self.info_conti_mu_linear(h)
            out["info_conti_var"] = torch.exp(self.info_conti_var_linear(h))
        unit = (lambda t: F.normalize(t, dim=1)) if self.normalize_d_embed else (lambda t: t)
        if cond == "AC":
            h = unit(h)     # (only the features are normalised: the reference's loop over the classifier's parameters rebinds a local name)
            out["cls_output"] = self.linear2(h)
        elif cond == "SPD":
            out["embed"] = self.linear1(h)
            adv = (out["embed"] * self.mapping(None, onehot)).sum(dim=1, keepdim=True) * (1 / math.sqrt(self.cmap_dim))
        elif cond in ("2C", "D2DCE"):
            out["embed"], out["proxy"] = unit(self.linear2(h)), unit(self.embedding(None, onehot))
        elif cond == "MD":
            adv = adv[torch.arange(label.shape[0], device=label.device), label]
        if self.aux_cls_type == "TAC":
            if cond == "AC":
                out["mi_cls_output"] = self.linear_mi(h)
            else:
                out["mi_embed"], out["mi_proxy"] = unit(self.linear_mi(h)), unit(self.embedding_mi(None, onehot))
        out.update(h=h, adv_output=adv, label=label)
        return out
