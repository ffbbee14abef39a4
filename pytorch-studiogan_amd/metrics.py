"""FID / IS feature-extraction path on the GPU, mirroring the reference's evaluation interfaces:

  LoadEvalModel(...).get_outputs(x, quantize)           reference src/metrics/preparation.py:43-122 (InceptionV3_tf, DINO_torch)
  generate_images_and_stack_features(...)               reference src/metrics/features.py:17-65
  calculate_moments / frechet_inception_distance        reference src/metrics/fid.py:34-98
  calculate_kl_div / top-k accuracy                     reference src/metrics/ins.py:28-79

What changes underneath: the per-batch GPU->CPU->per-image-resize->GPU round trip (reference src/utils/ops.py:251-263) is
ONE kernel (`sg_quantize_resize_normalize`: bit-exact uint8 quantisation, bilinear align_corners=False, normalise,
NHWC); InceptionV3 runs as 94 fused conv+foldedBN+ReLU launches writing straight into the concat buffers (no cat
copies), pools and the fc on libsgamd.so; FID moments are accumulated on the device in fp64 instead of gathering
50k x 2048 features to the host. The matrix square root stays on the host in fp64 like the reference.

  calculate_intra_class_fid / intra_class_frechet       reference src/worker.py:1380-1465 (`-ifid`): all classes' small-sample Frechet distances on the
                                                        device from the samples themselves (csrc/frechet_small.hip)
"""
import math

import numpy as np
import torch

from . import _lib as L
from . import functional as F

BN_EPS = 1e-3


def _spec():
    def A(p, c, pf):
        return [(p + ".branch1x1", c, 64, 1, 1, 1, 0, 0), (p + ".branch5x5_1", c, 48, 1, 1, 1, 0, 0), (p + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2),
                (p + ".branch3x3dbl_1", c, 64, 1, 1, 1, 0, 0), (p + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), (p + ".branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1),
                (p + ".branch_pool", c, pf, 1, 1, 1, 0, 0)]

    def B(p, c):
        return [(p + ".branch3x3", c, 384, 3, 3, 2, 0, 0), (p + ".branch3x3dbl_1", c, 64, 1, 1, 1, 0, 0), (p + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1),
                (p + ".branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0)]

    def Cb(p, c, c7):
        return [(p + ".branch1x1", c, 192, 1, 1, 1, 0, 0), (p + ".branch7x7_1", c, c7, 1, 1, 1, 0, 0), (p + ".branch7x7_2", c7, c7, 1, 7, 1, 0, 3),
                (p + ".branch7x7_3", c7, 192, 7, 1, 1, 3, 0), (p + ".branch7x7dbl_1", c, c7, 1, 1, 1, 0, 0), (p + ".branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0),
                (p + ".branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3), (p + ".branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0), (p + ".branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3),
                (p + ".branch_pool", c, 192, 1, 1, 1, 0, 0)]

    def D(p, c):
        return [(p + ".branch3x3_1", c, 192, 1, 1, 1, 0, 0), (p + ".branch3x3_2", 192, 320, 3, 3, 2, 0, 0), (p + ".branch7x7x3_1", c, 192, 1, 1, 1, 0, 0),
                (p + ".branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3), (p + ".branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0), (p + ".branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0)]

    def E(p, c):
        return [(p + ".branch1x1", c, 320, 1, 1, 1, 0, 0), (p + ".branch3x3_1", c, 384, 1, 1, 1, 0, 0), (p + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1),
                (p + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0), (p + ".branch3x3dbl_1", c, 448, 1, 1, 1, 0, 0), (p + ".branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1),
                (p + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1), (p + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0), (p + ".branch_pool", c, 192, 1, 1, 1, 0, 0)]
    stem = [("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0), ("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0), ("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1),
            ("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0), ("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0)]
    layers = (stem + A("Mixed_5b", 192, 32) + A("Mixed_5c", 256, 64) + A("Mixed_5d", 288, 64) + B("Mixed_6a", 288) + Cb("Mixed_6b", 768, 128) +
              Cb("Mixed_6c", 768, 160) + Cb("Mixed_6d", 768, 160) + Cb("Mixed_6e", 768, 192) + D("Mixed_7a", 768) + E("Mixed_7b", 1280) + E("Mixed_7c", 2048))
    return {l[0]: l for l in layers}


SPEC = _spec()


def synthetic_state_dict(seed=0):
    """Seeded random weights under torchvision's inception_v3 state_dict names (94 BasicConv2d + fc), for throughput measurements
    when the pretrained FID weights (reference src/metrics/inception_net.py:13,130, downloaded at run time) are not available.
    Same values as the test oracle's generator for the same seed (same draw order), without importing it."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (_, cin, cout, kh, kw, _, _, _) in SPEC.items():
        fan = cin * kh * kw
        sd[name + ".conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / fan)
        sd[name + ".bn.weight"] = 1.0 + 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_var"] = 0.5 + torch.rand(cout, generator=g)
        sd[name + ".bn.num_batches_tracked"] = torch.tensor(0)
    sd["fc.weight"] = torch.randn(1008, 2048, generator=g) * math.sqrt(1.0 / 2048)
    sd["fc.bias"] = 0.01 * torch.randn(1008, generator=g)
    return sd


# ---- the pin of the published FID network -------------------------------------------------------------------------
# reference src/metrics/inception_net.py:13,117-130: torchvision inception_v3(num_classes=1008, aux_logits=False) patched with the FID blocks,
# then `load_state_dict(load_state_dict_from_url(FID_WEIGHTS_URL))`. The file cannot be fetched here, but everything that identifies it can be
# enforced: its name carries the first 8 hex digits of its sha256 (the torch.hub convention `<name>-<sha256 prefix>.pth`, which
# load_state_dict_from_url(check_hash=True) verifies), and a strict load needs exactly these tensors with exactly these shapes.
FID_WEIGHTS_URL = "https://github.com/mseitzer/pytorch-fid/releases/download/fid_weights/pt_inception-2015-12-05-6726825d.pth"
FID_WEIGHTS_FILE = "pt_inception-2015-12-05-6726825d.pth"
FID_WEIGHTS_SHA256_PREFIX = "6726825d"


def inception_manifest():
    """{state_dict key: shape} of the FID InceptionV3: 94 BasicConv2d (conv weight without bias + BatchNorm2d(eps 1e-3) weight / bias / running
    statistics) and the 1008-way fc. `num_batches_tracked` entries are optional (a checkpoint converted from TensorFlow has none and torch's
    strict load tolerates their absence for such BatchNorm modules)."""
    m = {}
    for name, (_, cin, cout, kh, kw, _, _, _) in SPEC.items():
        m[name + ".conv.weight"] = (cout, cin, kh, kw)
        for t in ("weight", "bias", "running_mean", "running_var"):
            m[f"{name}.bn.{t}"] = (cout,)
    m["fc.weight"] = (1008, 2048)
    m["fc.bias"] = (1008,)
    return m


def validate_inception_state_dict(sd):
    """What `inception.load_state_dict(state_dict)` (strict) enforces in the reference: every expected tensor present with its shape, floating
    point, nothing else in the file. Raises RuntimeError naming the offending keys."""
    man = inception_manifest()
    keys = {k for k in sd if not k.endswith("num_batches_tracked")}
    missing = sorted(set(man) - keys)
    unexpected = sorted(keys - set(man))
    wrong = sorted(k for k in man if k in sd and (tuple(sd[k].shape) != man[k] or not torch.is_floating_point(sd[k])))
    if missing or unexpected or wrong:
        def head(v):
            return ", ".join(v[:4]) + (f" (+{len(v) - 4} more)" if len(v) > 4 else "")
        raise RuntimeError("not an FID InceptionV3 state_dict (" + FID_WEIGHTS_FILE + "): "
                           + (f"missing {len(missing)}: {head(missing)}; " if missing else "")
                           + (f"unexpected {len(unexpected)}: {head(unexpected)}; " if unexpected else "")
                           + (f"wrong shape / dtype {len(wrong)}: {head(wrong)}" if wrong else ""))
    return True


def load_fid_weights(path, check_hash=True):
    """torch.load of the published FID weights with the hash check torch.hub applies to `<name>-<sha256 prefix>.pth` files and the strict
    structural check; returns (state_dict, sha256 hex)."""
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    digest = h.hexdigest()
    if check_hash and not digest.startswith(FID_WEIGHTS_SHA256_PREFIX):
        raise RuntimeError(f"{path}: sha256 {digest[:16]}... does not start with {FID_WEIGHTS_SHA256_PREFIX} -- not {FID_WEIGHTS_FILE}")
    sd = torch.load(path, map_location="cpu")
    validate_inception_state_dict(sd)
    return sd, digest


class InceptionV3:
    """FID InceptionV3 (torchvision structure + the reference's FID patches, src/metrics/inception_net.py:135-249),
    inference only, BN folded into the convolutions at load time. `state_dict` uses torchvision's key names, i.e. the
    reference's `pt_inception-2015-12-05-6726825d.pth` loads as is."""

    def __init__(self, state_dict, device, dtype=torch.float32, f32_mode="exact"):
        """f32_mode (dtype fp32 only): "exact" = fp32 MFMA; "bf16x3" = fp32 tensors, every convolution's operands split into two bf16 terms in registers and
        contracted with three bf16 MFMAs per k-tile (functional.f32_mode): ~2^-16 relative per product, measured 3e-6 on the pool3 features against the oracle;
        "bf16x6" = three bf16 terms (exact split) and six MFMAs per k-tile, in the convolutions and the final linear layer: fp32-grade arithmetic on the bf16
        matrix pipe (measured figures: profiles/f32_modes_bench.txt)."""
        self.device, self.dtype = device, dtype
        if f32_mode not in F.f32_mode.MODES:
            raise ValueError(f"InceptionV3: f32_mode {f32_mode!r}")
        self.f32_mode = f32_mode if dtype == torch.float32 else "exact"
        self.w, self.b = {}, {}
        with torch.no_grad():
            for name, (_, cin, cout, kh, kw, stride, ph, pw) in SPEC.items():
                w = state_dict[name + ".conv.weight"].to(device=device, dtype=torch.float32)
                assert tuple(w.shape) == (cout, cin, kh, kw), f"{name}: weight shape {tuple(w.shape)}"
                g, be = state_dict[name + ".bn.weight"].to(device).float(), state_dict[name + ".bn.bias"].to(device).float()
                mu, var = state_dict[name + ".bn.running_mean"].to(device).float(), state_dict[name + ".bn.running_var"].to(device).float()
                scale = g / torch.sqrt(var + BN_EPS)
                self.w[name] = (w * scale.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous().to(dtype)   # [Cout][R][S][Cin]
                self.b[name] = (be - mu * scale).contiguous()
            self.fc_w = state_dict["fc.weight"].to(device=device, dtype=torch.float32).contiguous()
            self.fc_b = state_dict["fc.bias"].to(device=device, dtype=torch.float32).contiguous()

    # -- building blocks ---------------------------------------------------------------------------------------
    def _bc(self, x, name, out=None, coff=0):
        _, cin, cout, kh, kw, stride, ph, pw = SPEC[name]
        return F.conv2d_raw(x, self.w[name].data_ptr(), cin, cout, kh, kw, stride, ph, pw, 0, L.EPI_RELU, bias=self.b[name], out=out, out_coff=coff)

    def _pool(self, x, k, stride, pad, mode, out=None, coff=0):
        N, H, W, Cc = x.shape
        OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        if out is None:
            out = torch.empty((N, OH, OW, Cc), dtype=x.dtype, device=x.device)
        L.call("sg_pool2d", L.dt(x), L.ptr(x), L.ptr(out), N, H, W, Cc, k, stride, pad, mode, out.shape[-1], coff, L.stream())
        return out

    def _cat(self, x, ch, stride=1):
        N, H, W, _ = x.shape
        if stride == 2:
            H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        return torch.empty((N, H, W, ch), dtype=x.dtype, device=x.device)

    def _A(self, x, p, pf):
        o = self._cat(x, 64 + 64 + 96 + pf)
        self._bc(x, p + ".branch1x1", o, 0)
        self._bc(self._bc(x, p + ".branch5x5_1"), p + ".branch5x5_2", o, 64)
        self._bc(self._bc(self._bc(x, p + ".branch3x3dbl_1"), p + ".branch3x3dbl_2"), p + ".branch3x3dbl_3", o, 128)
        self._bc(self._pool(x, 3, 1, 1, 2), p + ".branch_pool", o, 224)
        return o

    def _B(self, x, p):
        cin = x.shape[3]
        o = self._cat(x, 384 + 96 + cin, stride=2)
        self._bc(x, p + ".branch3x3", o, 0)
        self._bc(self._bc(self._bc(x, p + ".branch3x3dbl_1"), p + ".branch3x3dbl_2"), p + ".branch3x3dbl_3", o, 384)
        self._pool(x, 3, 2, 0, 0, o, 480)
        return o

    def _C(self, x, p):
        o = self._cat(x, 768)
        self._bc(x, p + ".branch1x1", o, 0)
        self._bc(self._bc(self._bc(x, p + ".branch7x7_1"), p + ".branch7x7_2"), p + ".branch7x7_3", o, 192)
        t = x
        for i in range(1, 5):
            t = self._bc(t, p + f".branch7x7dbl_{i}")
        self._bc(t, p + ".branch7x7dbl_5", o, 384)
        self._bc(self._pool(x, 3, 1, 1, 2), p + ".branch_pool", o, 576)
        return o

    def _D(self, x, p):
        cin = x.shape[3]
        o = self._cat(x, 320 + 192 + cin, stride=2)
        self._bc(self._bc(x, p + ".branch3x3_1"), p + ".branch3x3_2", o, 0)
        t = x
        for i in range(1, 4):
            t = self._bc(t, p + f".branch7x7x3_{i}")
        self._bc(t, p + ".branch7x7x3_4", o, 320)
        self._pool(x, 3, 2, 0, 0, o, 512)
        return o

    def _E(self, x, p, pool_mode):
        o = self._cat(x, 2048)
        self._bc(x, p + ".branch1x1", o, 0)
        t = self._bc(x, p + ".branch3x3_1")
        self._bc(t, p + ".branch3x3_2a", o, 320)
        self._bc(t, p + ".branch3x3_2b", o, 704)
        t = self._bc(self._bc(x, p + ".branch3x3dbl_1"), p + ".branch3x3dbl_2")
        self._bc(t, p + ".branch3x3dbl_3a", o, 1088)
        self._bc(t, p + ".branch3x3dbl_3b", o, 1472)
        self._bc(self._pool(x, 3, 1, 1, pool_mode), p + ".branch_pool", o, 1856)
        return o

    @torch.no_grad()
    def forward_nhwc(self, x):
        """x: [B,299,299,3] NHWC in the compute dtype, values in [-1,1] -> (pool3 features [B,2048], logits [B,1008]), fp32."""
        if self.f32_mode != "exact":
            with F.f32_mode(self.f32_mode):
                return self._forward_nhwc(x)
        return self._forward_nhwc(x)

    def _forward_nhwc(self, x):
        x = self._bc(self._bc(self._bc(x, "Conv2d_1a_3x3"), "Conv2d_2a_3x3"), "Conv2d_2b_3x3")
        x = self._pool(x, 3, 2, 0, 0)
        x = self._bc(self._bc(x, "Conv2d_3b_1x1"), "Conv2d_4a_3x3")
        x = self._pool(x, 3, 2, 0, 0)
        x = self._A(x, "Mixed_5b", 32); x = self._A(x, "Mixed_5c", 64); x = self._A(x, "Mixed_5d", 64)
        x = self._B(x, "Mixed_6a")
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self._C(x, n)
        x = self._D(x, "Mixed_7a")
        x = self._E(x, "Mixed_7b", 2)   # average pool without padded zeros (count_include_pad=False)
        x = self._E(x, "Mixed_7c", 0)   # max pool
        N, H, W, Cc = x.shape
        feat = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
        L.call("sg_global_avgpool", L.dt(x), L.ptr(x), L.ptr(feat), N, H * W, Cc, L.stream())
        logits = torch.empty((N, 1008), dtype=torch.float32, device=x.device)
        F.gemm_raw(L.F32, self.fc_w, 0, 2048, feat, 0, 2048, logits, 1008, 1008, N, 2048, bias=self.fc_b)
        return feat, logits


# ---- DINO ViT backbone (eval_backbone "DINO_torch") ---------------------------------------------------------------------------------------------------
# reference src/metrics/preparation.py:69-74: vit_small(patch_size=8, num_classes=1000, num_last_blocks=4) with the published DINO backbone and linear-
# classifier weights (src/utils/misc.py:632-691). The two files cannot be fetched here and carry no hash in their names; what identifies them -- the file
# names and a strict structural check -- is enforced, and their sha256 digests are reported for the user to compare.
DINO_WEIGHTS_URL = "https://dl.fbaipublicfiles.com/dino/dino_deitsmall8_pretrain/"
DINO_BACKBONE_FILE = "dino_deitsmall8_pretrain.pth"
DINO_LINEAR_FILE = "dino_deitsmall8_linearweights.pth"
DINO_PUBLISHED_GEOMETRY = (384, 12, 8, 785, 1000)       # dino_manifest arguments of vit_small(patch_size=8, num_classes=1000) at 224 x 224
LN_EPS = 1e-6                 # reference src/metrics/vit.py:237 (partial(nn.LayerNorm, eps=1e-6))
VIT_HEAD_DIM = 64             # every DINO ViT (tiny 192 / 3, small 384 / 6, base 768 / 12); the fused attention kernel is built for it

_BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias",
                 "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def dino_manifest(embed, depth, patch, tokens, classes, hidden=None, num_last_blocks=4):
    """{state_dict key: shape} of the reference's VisionTransformer with a linear head over the class tokens of the last `num_last_blocks` blocks."""
    hidden = 4 * embed if hidden is None else hidden
    m = {"cls_token": (1, 1, embed), "pos_embed": (1, tokens, embed), "patch_embed.proj.weight": (embed, 3, patch, patch), "patch_embed.proj.bias": (embed,),
         "norm.weight": (embed,), "norm.bias": (embed,), "linear.weight": (classes, num_last_blocks * embed), "linear.bias": (classes,)}
    shapes = {"norm1.weight": (embed,), "norm1.bias": (embed,), "attn.qkv.weight": (3 * embed, embed), "attn.qkv.bias": (3 * embed,),
              "attn.proj.weight": (embed, embed), "attn.proj.bias": (embed,), "norm2.weight": (embed,), "norm2.bias": (embed,),
              "mlp.fc1.weight": (hidden, embed), "mlp.fc1.bias": (hidden,), "mlp.fc2.weight": (embed, hidden), "mlp.fc2.bias": (embed,)}
    for i in range(depth):
        for k in _BLOCK_PARAMS:
            m[f"blocks.{i}.{k}"] = shapes[k]
    return m


def validate_dino_state_dict(sd, num_heads=None, num_last_blocks=4):
    """Reads the geometry off the tensor shapes and enforces what a strict load of the reference's model would: every expected tensor present with its
    shape, floating point, nothing else. Returns dict(embed, depth, heads, patch, tokens, grid, classes, hidden, num_last_blocks); raises RuntimeError
    naming the offending keys. num_heads: default embed / 64 (all DINO ViTs); any value that does not give head dimension 64 is refused."""
    def bad(msg):
        raise RuntimeError("not a DINO ViT state_dict (" + DINO_BACKBONE_FILE + " + " + DINO_LINEAR_FILE + "): " + msg)
    for k in ("cls_token", "pos_embed", "patch_embed.proj.weight", "linear.weight"):
        if k not in sd:
            bad(f"missing {k}")
        if not torch.is_tensor(sd[k]) or not torch.is_floating_point(sd[k]):
            bad(f"{k} is not a floating-point tensor")
    if sd["cls_token"].dim() != 3 or sd["pos_embed"].dim() != 3 or sd["patch_embed.proj.weight"].dim() != 4 or sd["linear.weight"].dim() != 2:
        bad("wrong rank of cls_token / pos_embed / patch_embed.proj.weight / linear.weight")
    embed = int(sd["cls_token"].shape[-1])
    tokens = int(sd["pos_embed"].shape[1])
    patch = int(sd["patch_embed.proj.weight"].shape[-1])
    classes = int(sd["linear.weight"].shape[0])
    depth = 0
    while f"blocks.{depth}.norm1.weight" in sd:
        depth += 1
    heads = embed // VIT_HEAD_DIM if num_heads is None else int(num_heads)
    if heads < 1 or heads * VIT_HEAD_DIM != embed:
        bad(f"embed {embed} with {heads} heads: the head dimension must be {VIT_HEAD_DIM}")
    grid = int(round(math.sqrt(max(tokens - 1, 0))))
    if tokens < 2 or grid * grid != tokens - 1:
        bad(f"pos_embed holds {tokens} tokens: 1 + a square patch grid expected")
    if depth < num_last_blocks:
        bad(f"{depth} blocks, fewer than num_last_blocks = {num_last_blocks}")
    hidden = int(sd["blocks.0.mlp.fc1.weight"].shape[0]) if "blocks.0.mlp.fc1.weight" in sd and sd["blocks.0.mlp.fc1.weight"].dim() == 2 else 4 * embed
    if embed % 64 or hidden % 64:
        bad(f"embed {embed} / hidden {hidden}: multiples of 64 expected")
    man = dino_manifest(embed, depth, patch, tokens, classes, hidden, num_last_blocks)
    missing = sorted(set(man) - set(sd))
    unexpected = sorted(set(sd) - set(man))
    wrong = sorted(k for k in man if k in sd and (tuple(sd[k].shape) != man[k] or not torch.is_floating_point(sd[k])))
    if missing or unexpected or wrong:
        def head(v):
            return ", ".join(v[:4]) + (f" (+{len(v) - 4} more)" if len(v) > 4 else "")
        bad((f"missing {len(missing)}: {head(missing)}; " if missing else "") + (f"unexpected {len(unexpected)}: {head(unexpected)}; " if unexpected else "")
            + (f"wrong shape / dtype {len(wrong)}: {head(wrong)}" if wrong else ""))
    return dict(embed=embed, depth=depth, heads=heads, patch=patch, tokens=tokens, grid=grid, classes=classes, hidden=hidden, num_last_blocks=num_last_blocks)


def _sha256(path):
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def load_dino_weights(backbone_path, linear_path, checkpoint_key="teacher"):
    """The two published files -> one state_dict under the reference's names, with the layout handling of src/utils/misc.py:632-691: the backbone
    optionally under `checkpoint_key`, `module.` / `backbone.` prefixes stripped, tensors the model does not own (a training checkpoint's projection
    head) dropped as the reference's non-strict load drops them; the classifier under "state_dict" with `module.linear.` stripped. There is no
    download. Returns (state_dict, (sha256 backbone, sha256 linear), pinned); pinned: both files carry the published names AND the merged dict is
    exactly the ViT-S/8 manifest (DINO_PUBLISHED_GEOMETRY). No digest of the published files is known offline, so the flag is name- and shape-based
    only: compare the returned digests with your download to be sure."""
    import os
    for what, path, name in (("weights_path", backbone_path, DINO_BACKBONE_FILE), ("linear_weights_path", linear_path, DINO_LINEAR_FILE)):
        if path is None or not os.path.isfile(path):
            raise RuntimeError(f"{what}={path!r}: DINO_torch needs both {DINO_BACKBONE_FILE} and {DINO_LINEAR_FILE} (from {DINO_WEIGHTS_URL}); there is no "
                               "network access here")
    bb = torch.load(backbone_path, map_location="cpu")
    if checkpoint_key is not None and checkpoint_key in bb:
        bb = bb[checkpoint_key]
    bb = {k.replace("module.", "").replace("backbone.", ""): v for k, v in bb.items()}
    lin = torch.load(linear_path, map_location="cpu")["state_dict"]
    lin = {k.replace("module.linear.", ""): v for k, v in lin.items()}
    if set(lin) != {"weight", "bias"}:
        raise RuntimeError(f"{linear_path}: a linear classifier (weight, bias) expected under 'state_dict', found {sorted(lin)[:4]}")
    own = ("cls_token", "pos_embed", "patch_embed.", "blocks.", "norm.")
    sd = {k: v for k, v in bb.items() if k.startswith(own)}
    sd["linear.weight"], sd["linear.bias"] = lin["weight"], lin["bias"]
    geo = validate_dino_state_dict(sd)
    published = dino_manifest(*DINO_PUBLISHED_GEOMETRY)
    pinned = (os.path.basename(backbone_path) == DINO_BACKBONE_FILE and os.path.basename(linear_path) == DINO_LINEAR_FILE
              and geo["num_last_blocks"] == 4 and {k: tuple(v.shape) for k, v in sd.items()} == published)
    return sd, (_sha256(backbone_path), _sha256(linear_path)), pinned


class DINOViT:
    """The reference's VisionTransformer forward (src/metrics/vit.py:198-224), inference only: patch embedding, `depth` pre-norm blocks on an fp32
    residual stream, and as output the class tokens of the last four blocks, each through the final norm, concatenated (+ the linear head on them).
    `state_dict` uses the reference's key names; the geometry is read from the shapes (validate_dino_state_dict).

    dtype=torch.bfloat16: the fused path -- per block LayerNorm -> bf16, qkv GEMM (bias), sg_mha_fwd on the packed qkv, proj GEMM (+= residual),
    LayerNorm, fc1 GEMM (bias + GELU), fc2 GEMM (+= residual): 7 launches, nothing elementwise in between.
    dtype=torch.float32: the same graph on the exact-fp32 sg_gemm, scores per head as batched sg_gemm + sg_softmax_rows + sg_gemm and an fp32 GELU
    pass: the exact path (and the A/B partner of the fused one); not built for speed.
    f32_mode (dtype fp32 only, as InceptionV3's): "exact", or a functional.f32_mode name applied around the forward -- "bf16x6" puts the sg_gemm launches of
    the graph on the bf16 matrix pipe at fp32 accuracy, those with all-vector operands (the linear layers, q k^T; P V only when the token count is a multiple
    of 4, and the 3-channel patch embedding never: they keep the exact MFMA); "bf16x3" is convolution-only and changes nothing here."""

    def __init__(self, state_dict, device, dtype=torch.float32, num_heads=None, f32_mode="exact"):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"DINOViT: dtype {dtype}")
        if f32_mode not in F.f32_mode.MODES:
            raise ValueError(f"DINOViT: f32_mode {f32_mode!r}")
        self.f32_mode = f32_mode if dtype == torch.float32 else "exact"
        self.geometry = g = validate_dino_state_dict(state_dict, num_heads=num_heads)
        if not L.lib().sg_mha_fwd_ok(1, g["tokens"], g["heads"], g["embed"] // g["heads"]):
            raise RuntimeError(f"DINOViT: no attention kernel for {g}")
        self.device, self.dtype = torch.device(device), dtype
        L.require_gpu(self.device)
        f32 = lambda k: state_dict[k].detach().to(device=self.device, dtype=torch.float32).contiguous()
        wt = lambda k: state_dict[k].detach().to(device=self.device, dtype=torch.float32).to(dtype).contiguous()
        with torch.no_grad():
            self.patch_w = state_dict["patch_embed.proj.weight"].detach().to(device=self.device, dtype=torch.float32).permute(0, 2, 3, 1).contiguous().to(dtype)
            self.patch_b = f32("patch_embed.proj.bias")
            self.cls, self.pos = f32("cls_token").view(-1), f32("pos_embed").view(g["tokens"], g["embed"])
            self.blocks = []
            for i in range(g["depth"]):
                p = f"blocks.{i}."
                self.blocks.append({k: (wt(p + k) if k.endswith("weight") and "norm" not in k else f32(p + k)) for k in _BLOCK_PARAMS})
            self.norm_w, self.norm_b = f32("norm.weight"), f32("norm.bias")
            self.lin_w, self.lin_b = f32("linear.weight"), f32("linear.bias")
        self.scale = float(VIT_HEAD_DIM) ** -0.5

    def _ln(self, x, rows, pitch, w, b, out, ldo):
        L.call("sg_layernorm_rows", L.dt(out), L.ptr(x), pitch, L.ptr(w), L.ptr(b), L.ptr(out), ldo, rows, self.geometry["embed"], LN_EPS, L.stream())

    def _linear_f32(self, x, w, b, out, M, N, K, res=None):
        F.gemm_raw(L.F32, w, 0, K, x, 0, K, out, N, N, M, K, bias=b, res=res, ldr=N if res is not None else 0)

    def _attention_f32(self, qkv, att, B):
        g = self.geometry
        N, C, H, D = g["tokens"], g["embed"], g["heads"], VIT_HEAD_DIM
        S = torch.empty((B, N, N), dtype=torch.float32, device=qkv.device)
        P = torch.empty_like(S)
        base = L.ptr(qkv)
        for h in range(H):
            q, k, v = base + 4 * (h * D), base + 4 * (C + h * D), base + 4 * (2 * C + h * D)
            F.gemm_raw(L.F32, k, 0, 3 * C, q, 0, 3 * C, S, N, N, N, D, batch=B, p_bs=N * 3 * C, q_bs=N * 3 * C, out_bs=N * N, alpha=self.scale)
            L.call("sg_softmax_rows", L.F32, L.ptr(S), L.ptr(P), B * N, N, L.stream())
            F.gemm_raw(L.F32, v, 1, 3 * C, P, 0, N, L.ptr(att) + 4 * h * D, C, D, N, N, batch=B, p_bs=N * 3 * C, q_bs=N * N, out_bs=N * C)

    @torch.no_grad()
    def forward_nhwc(self, x):
        """x: [B, res, res, 3] NHWC in the compute dtype, normalised -> (embed [B, 4 * C], logits [B, classes]), fp32. Only the native grid is
        served (the identity branch of interpolate_pos_encoding, vit.py:165); any other input size raises."""
        if self.f32_mode != "exact":
            with F.f32_mode(self.f32_mode):
                return self._forward_nhwc(x)
        return self._forward_nhwc(x)

    def _forward_nhwc(self, x):
        g = self.geometry
        C, N, Hd, p, nlb = g["embed"], g["tokens"], g["hidden"], g["patch"], g["num_last_blocks"]
        B = x.shape[0]
        if x.dtype != self.dtype or tuple(x.shape[1:]) != (g["grid"] * p, g["grid"] * p, 3):
            raise ValueError(f"DINOViT: input {tuple(x.shape)} {x.dtype}; [B, {g['grid'] * p}, {g['grid'] * p}, 3] {self.dtype} expected "
                             "(position-embedding interpolation for other sizes is not implemented)")
        bf = self.dtype == torch.bfloat16
        dev = x.device
        patches = F.conv2d_raw(x.contiguous(), self.patch_w.data_ptr(), 3, C, p, p, stride=p, epi_flags=L.EPI_OUT_F32 if bf else 0, bias=self.patch_b)
        M = B * N
        xs = torch.empty((M, C), dtype=torch.float32, device=dev)
        L.call("sg_vit_tokens", L.ptr(patches), L.ptr(self.cls), L.ptr(self.pos), L.ptr(xs), B, N, C, L.stream())
        y = torch.empty((M, C), dtype=self.dtype, device=dev)
        qkv = torch.empty((M, 3 * C), dtype=self.dtype, device=dev)
        att = torch.empty((M, C), dtype=self.dtype, device=dev)
        hid = torch.empty((M, Hd), dtype=self.dtype, device=dev)
        embed = torch.empty((B, nlb * C), dtype=torch.float32, device=dev)
        st = L.stream()
        for i, w in enumerate(self.blocks):
            self._ln(xs, M, C, w["norm1.weight"], w["norm1.bias"], y, C)
            if bf:
                L.call("sg_tok_gemm", 0, L.ptr(y), C, L.ptr(w["attn.qkv.weight"]), L.ptr(w["attn.qkv.bias"]), L.ptr(qkv), 3 * C, M, 3 * C, C, st)
                L.call("sg_mha_fwd", L.ptr(qkv), L.ptr(att), B, N, g["heads"], VIT_HEAD_DIM, self.scale, st)
                L.call("sg_tok_gemm", 2, L.ptr(att), C, L.ptr(w["attn.proj.weight"]), L.ptr(w["attn.proj.bias"]), L.ptr(xs), C, M, C, C, st)
            else:
                self._linear_f32(y, w["attn.qkv.weight"], w["attn.qkv.bias"], qkv, M, 3 * C, C)
                self._attention_f32(qkv, att, B)
                self._linear_f32(att, w["attn.proj.weight"], w["attn.proj.bias"], xs, M, C, C, res=xs)
            self._ln(xs, M, C, w["norm2.weight"], w["norm2.bias"], y, C)
            if bf:
                L.call("sg_tok_gemm", 1, L.ptr(y), C, L.ptr(w["mlp.fc1.weight"]), L.ptr(w["mlp.fc1.bias"]), L.ptr(hid), Hd, M, Hd, C, st)
                L.call("sg_tok_gemm", 2, L.ptr(hid), Hd, L.ptr(w["mlp.fc2.weight"]), L.ptr(w["mlp.fc2.bias"]), L.ptr(xs), C, M, C, Hd, st)
            else:
                self._linear_f32(y, w["mlp.fc1.weight"], w["mlp.fc1.bias"], hid, M, Hd, C)
                L.call("sg_gelu_f32", L.ptr(hid), L.ptr(hid), M * Hd, st)
                self._linear_f32(hid, w["mlp.fc2.weight"], w["mlp.fc2.bias"], xs, M, C, Hd, res=xs)
            j = i - (g["depth"] - nlb)
            if j >= 0:      # the class-token rows only (row pitch N * C) through the final norm, into their slice of the concatenation
                L.call("sg_layernorm_rows", L.F32, L.ptr(xs), N * C, L.ptr(self.norm_w), L.ptr(self.norm_b), L.ptr(embed) + 4 * j * C, nlb * C, B, C, LN_EPS, st)
        logits = torch.empty((B, g["classes"]), dtype=torch.float32, device=dev)
        F.gemm_raw(L.F32, self.lin_w, 0, nlb * C, embed, 0, nlb * C, logits, g["classes"], g["classes"], B, nlb * C, bias=self.lin_b)
        return embed, logits


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # reference src/metrics/preparation.py:70-71 (every torch backbone)


def _ms_args(mean, std, channels):
    """host float arrays for the *_ms entry points; None -> the (0.5, 0.5) entry point is called instead"""
    if mean is None and std is None:
        return None
    if mean is None or std is None or len(mean) != channels or len(std) != channels:
        raise ValueError(f"mean and std must both be given, one value per channel ({channels})")
    import ctypes
    arr = ctypes.c_float * channels
    return arr(*[float(v) for v in mean]), arr(*[float(v) for v in std])


def preprocess(x, dtype, quantize=True, size=299, want_uint8=False, mean=None, std=None):
    """ops.quantize_images + resize_images('legacy') + normalise on the device (reference utils/ops.py:251-263). mean / std: per-channel
    constants of (x / 255 - mean) / std; default (0.5, 0.5) as for InceptionV3_tf."""
    x = x.float().contiguous()
    N, Cc, H, W = x.shape
    out = torch.empty((N, size, size, Cc), dtype=dtype, device=x.device)
    q = torch.empty((N, Cc, H, W), dtype=torch.uint8, device=x.device) if want_uint8 else None
    ms = _ms_args(mean, std, Cc)
    if ms is None:
        L.call("sg_quantize_resize_normalize", L.dt(dtype), L.ptr(x), L.ptr(out), L.ptr(q), N, Cc, H, W, size, size, 1 if quantize else 0, L.stream())
    else:
        L.call("sg_quantize_resize_normalize_ms", L.dt(dtype), L.ptr(x), L.ptr(out), L.ptr(q), N, Cc, H, W, size, size, 1 if quantize else 0, ms[0], ms[1], L.stream())
    return (out, q) if want_uint8 else out


_PIL_FILTERS = {"bilinear": (1.0, lambda x: np.where(np.abs(x) < 1.0, 1.0 - np.abs(x), 0.0)),
                "bicubic": (2.0, None)}


def _bicubic(x, a=-0.5):
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def pil_coeffs(in_size, out_size, filt):
    """Pillow's precompute_coeffs (src/libImaging/Resample.c) for a full-image box: per output index the first source index, the number of
    taps and the normalised double coefficients; the support is the filter's, scaled by in / out when reducing (antialiasing)."""
    support, fn = _PIL_FILTERS[filt]
    fn = fn or _bicubic
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = fn((np.arange(xmax) + xmin - center + 0.5) * ss)
        ww = w.sum()
        if ww != 0.0:
            w = w / ww
        kk[xx, :xmax] = w
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


_PIL_CACHE = {}


def preprocess_pil(x, dtype, filt, quantize=True, size=299, mean=None, std=None):
    """ops.quantize_images + resize_images with a PIL resizer (reference utils/resize.py:39-78: 'clean' = bicubic, 'friendly' = bilinear for
    InceptionV3_tf and DINO_torch) + normalise, on the device. mean / std as in `preprocess`."""
    x = x.float().contiguous()
    N, Cc, H, W = x.shape
    key = (H, W, size, filt, str(x.device))
    if key not in _PIL_CACHE:
        bh, kh, nh = pil_coeffs(W, size, filt)
        bv, kv, nv = pil_coeffs(H, size, filt)
        to = lambda a: torch.from_numpy(a).to(x.device).contiguous()
        _PIL_CACHE[key] = (to(bh), to(kh), nh, to(bv), to(kv), nv)
    bh, kh, nh, bv, kv, nv = _PIL_CACHE[key]
    tmp = torch.empty((N, Cc, H, size), dtype=torch.float32, device=x.device)
    out = torch.empty((N, size, size, Cc), dtype=dtype, device=x.device)
    ms = _ms_args(mean, std, Cc)
    if ms is None:
        L.call("sg_pil_resize_normalize", L.dt(dtype), L.ptr(x), L.ptr(out), L.ptr(tmp), N, Cc, H, W, size, size, L.ptr(bh), L.ptr(kh), nh, L.ptr(bv), L.ptr(kv), nv,
               1 if quantize else 0, L.stream())
    else:
        L.call("sg_pil_resize_normalize_ms", L.dt(dtype), L.ptr(x), L.ptr(out), L.ptr(tmp), N, Cc, H, W, size, size, L.ptr(bh), L.ptr(kh), nh, L.ptr(bv), L.ptr(kv), nv,
               1 if quantize else 0, ms[0], ms[1], L.stream())
    return out


class LoadEvalModel:
    """reference src/metrics/preparation.py:43-122 for eval_backbone "InceptionV3_tf" (299 x 299, (0.5, 0.5) normalisation) and "DINO_torch" (ViT-S/8 at
    224 x 224, ImageNet mean / std) with the post-resizers "legacy" (torch bilinear), "clean" (PIL bicubic) and "friendly" (PIL bilinear for both
    backbones), reference src/utils/resize.py:49-69."""
    BACKBONES = ("InceptionV3_tf", "DINO_torch")
    RESIZERS = ("legacy", "clean", "friendly")

    def __init__(self, eval_backbone="InceptionV3_tf", post_resizer="legacy", world_size=1, distributed_data_parallel=False, device="cuda",
                 state_dict=None, dtype=torch.float32, weights_path=None, f32_mode="exact", linear_weights_path=None):
        """state_dict: tensors under the backbone's own names (torchvision's inception_v3 / the reference's vit.py), checked like the reference's strict
        load (anything else raises); weights_path: the published file itself (InceptionV3_tf: additionally checked against the sha256 prefix in its
        name; DINO_torch: the backbone file, with linear_weights_path the linear-classifier file).
        `self.weights_pinned` says which: True only for the published files -- FID / IS values from any other weights (the seeded random
        ones of bench.py and the tests) are NOT comparable with published numbers."""
        if eval_backbone not in self.BACKBONES or post_resizer not in self.RESIZERS:
            raise NotImplementedError(f"eval_backbone {eval_backbone!r} / post_resizer {post_resizer!r}: {' and '.join(self.BACKBONES)} with the "
                                      f"{' / '.join(self.RESIZERS)} resizers are on the hot path (SURVEY §2, DESIGN §7)")
        self.weights_pinned, self.weights_sha256 = False, None
        self.eval_backbone, self.post_resizer, self.device = eval_backbone, post_resizer, torch.device(device)
        self.dtype = dtype
        if eval_backbone == "DINO_torch":
            if weights_path is not None or linear_weights_path is not None:
                state_dict, self.weights_sha256, self.weights_pinned = load_dino_weights(weights_path, linear_weights_path)
            if state_dict is None:
                raise RuntimeError("pass the DINO ViT-S/8 weights (weights_path=.../" + DINO_BACKBONE_FILE + " and linear_weights_path=.../" + DINO_LINEAR_FILE +
                                   ", both from " + DINO_WEIGHTS_URL + ", or a merged state_dict); there is no network access here")
            self.res, self.mean, self.std = 224, IMAGENET_MEAN, IMAGENET_STD
            self.model = DINOViT(state_dict, self.device, dtype, f32_mode=f32_mode)      # f32_mode: DINOViT.__init__
            return
        if weights_path is not None:
            state_dict, self.weights_sha256 = load_fid_weights(weights_path)
            self.weights_pinned = True
        if state_dict is None:
            raise RuntimeError("pass the FID Inception weights (weights_path=.../" + FID_WEIGHTS_FILE + ", from " + FID_WEIGHTS_URL +
                               ", or its state_dict); there is no network access here")
        validate_inception_state_dict(state_dict)
        self.res, self.mean, self.std = 299, None, None
        self.model = InceptionV3(state_dict, self.device, dtype, f32_mode=f32_mode)      # f32_mode: InceptionV3.__init__

    def eval(self):
        pass

    @torch.no_grad()
    def get_outputs(self, x, quantize=False):
        """(features, logits), fp32: InceptionV3_tf [B, 2048] / [B, 1008]; DINO_torch [B, 4 * embed] / [B, 1000]"""
        if self.post_resizer == "legacy":
            return self.model.forward_nhwc(preprocess(x, self.dtype, quantize, self.res, mean=self.mean, std=self.std))
        return self.model.forward_nhwc(preprocess_pil(x, self.dtype, "bicubic" if self.post_resizer == "clean" else "bilinear", quantize, self.res,
                                                      mean=self.mean, std=self.std))


def softmax_rows(logits):
    p = torch.empty_like(logits)
    L.call("sg_softmax_rows", L.F32, L.ptr(logits), L.ptr(p), logits.shape[0], logits.shape[1], L.stream())
    return p


@torch.no_grad()
def generate_images_and_stack_features(generator, eval_model, num_generate, batch_size, z_dim, num_classes, quantize=True, world_size=1,
                                       DDP=False, device="cuda", moments=None, z_prior="gaussian", truncation_factor=-1.0, MODEL=None, latent_opt=None, langevin=None,
                                       y_sampler="totally_random"):
    """reference src/metrics/features.py:17-65. Returns (features [n, dim], probs [n, classes], labels list); dim / classes are the backbone's
    (InceptionV3_tf 2048 / 1008, DINO_torch 1536 / 1000).
    moments: optional `FeatureMoments` accumulator fed on the device. It receives exactly the rows the reference keeps
    (`fake_feats[:num_generate]` of the rank-major gathered stack, src/metrics/fid.py:68-69): the over-generated tail --
    ceil(num_generate / batch) batches, `num_batches // world_size + 1` per rank under DDP -- is NOT accumulated.
    z_prior / truncation_factor / MODEL (InfoGAN codes behind z): the reference's evaluation-time sampling (src/utils/sample.py:90-118 with is_train=False).
    latent_opt: LOGAN at evaluation time (src/utils/sample.py:96,123-135 with LOSS.lo_steps4eval): dict(discriminator=, lo_rate=, lo_steps=, lo_alpha=, lo_beta=) -- the
    latents take their step along d D(G(z)) / dz (the one place of this function that runs with gradients enabled) before the images are generated.
    langevin: RUN.langevin_sampling (src/utils/sample.py:136-148,195-216): dict(discriminator=, langevin_rate=, langevin_noise_std=, langevin_decay=, langevin_decay_steps=,
    langevin_steps=) -- losses.langevin_sampling on the drawn latents.
    y_sampler: "totally_random", or an int -- every label is that class and nothing is drawn for the labels (src/utils/sample.py:56-57; intra-class FID)."""
    from .worker import sample_zy, sample_latents
    plain = z_prior == "gaussian" and truncation_factor == -1.0 and getattr(MODEL, "info_type", "N/A") == "N/A" and latent_opt is None and langevin is None
    num_batches = int(math.ceil(float(num_generate) / float(batch_size)))
    rank = 0
    if DDP:
        num_batches = num_batches // world_size + 1
        if world_size > 1:
            import torch.distributed as dist
            rank = dist.get_rank()
    # rows of this rank sit at [rank * per_rank, (rank + 1) * per_rank) of the gathered stack; the first num_generate survive
    per_rank = num_batches * batch_size
    keep = max(0, min(per_rank, num_generate - rank * per_rank))
    feats, probs, labels = [], [], []
    for b in range(num_batches):
        if plain:
            zs, ys = sample_zy(batch_size, z_dim, num_classes, device, y_sampler=y_sampler)
        else:
            zs, ys = sample_latents(batch_size, z_dim, num_classes, device, z_prior=z_prior, truncation_factor=truncation_factor, MODEL=MODEL, y_sampler=y_sampler)
        if latent_opt is not None:
            from .losses import latent_optimise
            with torch.enable_grad():
                zs, _ = latent_optimise(zs=zs, fake_labels=ys, generator=generator, discriminator=latent_opt["discriminator"], batch_size=zs.shape[0],
                                        lo_rate=latent_opt["lo_rate"], lo_steps=latent_opt["lo_steps"], lo_alpha=latent_opt["lo_alpha"], lo_beta=latent_opt["lo_beta"],
                                        eval=True, cal_trsp_cost=False, device=device)
            zs = zs.detach()
        if langevin is not None:          # src/utils/sample.py:136-148 (RUN.langevin_sampling; exclusive with latent optimisation, src/config.py:650-651)
            from .losses import langevin_sampling
            with torch.enable_grad():
                zs = langevin_sampling(zs=zs, z_dim=z_dim, fake_labels=ys, generator=generator, discriminator=langevin["discriminator"], batch_size=zs.shape[0],
                                       langevin_rate=langevin["langevin_rate"], langevin_noise_std=langevin["langevin_noise_std"], langevin_decay=langevin["langevin_decay"],
                                       langevin_decay_steps=langevin["langevin_decay_steps"], langevin_steps=langevin["langevin_steps"], device=device)
            zs = zs.detach()
        fake = generator(zs, ys, eval=True)
        f, logit = eval_model.get_outputs(fake, quantize=quantize)
        if moments is not None:
            take = max(0, min(batch_size, keep - b * batch_size))
            if take:
                moments.add(f[:take])
        feats.append(f)
        probs.append(softmax_rows(logit))
        labels.append(ys)
    feats, probs, labels = torch.cat(feats, 0), torch.cat(probs, 0), torch.cat(labels, 0)
    if DDP and world_size > 1:
        import torch.distributed as dist
        def gather(t):
            out = [torch.zeros_like(t) for _ in range(world_size)]
            dist.all_gather(out, t)
            return torch.cat(out, 0)
        feats, probs, labels = gather(feats), gather(probs), gather(labels)
    return feats, probs, list(labels.detach().cpu().numpy())


class FeatureMoments:
    """sum f and sum f f^T in fp64 on the device (replaces np.mean / np.cov over gathered features, fid.py:96-97); in
    data-parallel runs the two accumulators are all-reduced instead of gathering 50k x dim floats per rank (dim: 2048 for InceptionV3_tf, 1536 for
    DINO_torch -- any width)."""

    def __init__(self, dim, device):
        self.dim, self.n = dim, 0
        self.s1 = torch.zeros(dim, dtype=torch.float64, device=device)
        self.s2 = torch.zeros(dim, dim, dtype=torch.float64, device=device)

    def add(self, f):
        f = f.float().contiguous()
        L.call("sg_feat_moments_accumulate", L.ptr(f), f.shape[0], self.dim, L.ptr(self.s1), L.ptr(self.s2), L.stream())
        self.n += f.shape[0]

    def finalize(self, group=None):
        n = self.n
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(self.s1, group=group); dist.all_reduce(self.s2, group=group)
            t = torch.tensor([n], dtype=torch.float64, device=self.s1.device); dist.all_reduce(t, group=group); n = int(t.item())
        mu = (self.s1 / n).cpu().numpy()
        s2 = self.s2.cpu().numpy()
        sigma = (s2 - n * np.outer(mu, mu)) / (n - 1)      # np.cov(rowvar=False): unbiased
        return mu, sigma


def calculate_moments(feats, num_generate=None):
    f = feats[:num_generate] if num_generate else feats
    m = FeatureMoments(f.shape[1], f.device)
    for i in range(0, f.shape[0], 4096):
        m.add(f[i:i + 4096])
    return m.finalize()


def frechet_inception_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """reference src/metrics/fid.py:34-62 (host fp64, scipy.linalg.sqrtm)."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def _nuclear_norm_sweeps(B, ne, max_sweeps, tol):
    """Sum of the singular values of the [ne][ne] fp64 device matrix B (ne even; B is overwritten): one sg_jacobi_sweep launch train and one read-back of the
    convergence measure per sweep, then sg_row_norm_sum. Returns (value, sweeps run)."""
    offd = torch.zeros(1, dtype=torch.float64, device=B.device)
    sweeps = 0
    for _ in range(max_sweeps):
        L.call("sg_jacobi_sweep", L.ptr(B), ne, L.ptr(offd), L.stream())
        sweeps += 1
        if float(offd.item()) < tol:
            break
    else:
        if float(offd.item()) > 1e-8:       # (the sum of the singular values is second-order accurate in this measure)
            raise RuntimeError(f"one-sided Jacobi did not converge in {max_sweeps} sweeps (off-diagonal measure {float(offd.item()):.2e})")
    nuc = torch.zeros(1, dtype=torch.float64, device=B.device)
    L.call("sg_row_norm_sum", L.ptr(B), ne, L.ptr(nuc), L.stream())
    return float(nuc.item()), sweeps


def frechet_inception_distance_device(mu1, sigma1, mu2, sigma2, device=None, max_sweeps=40, tol=1e-12):
    """The same distance with tr sqrtm(S1 S2) computed on the GPU in fp64 (csrc/linalg.hip): Cholesky factors, B = L2^T L1, one-sided
    Jacobi sweeps until the rows of B are orthogonal to `tol`, sum of their norms (= sum of sqrt of the eigenvalues of S1 S2).
    When a covariance is not positive definite (fewer samples than dimensions) the host formula above -- the reference's own route,
    eps branch included -- is used instead. Returns a python float."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    n = s1.shape[0]
    ne = n + (n & 1)                                    # the tournament pairs rows: pad an odd dimension with one zero row / column of B
    L1 = torch.from_numpy(s1).to(dev).contiguous().clone()
    L2 = torch.from_numpy(s2).to(dev).contiguous().clone()
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    L.call("sg_chol_lower", L.ptr(L1), n, L.ptr(flags), L.stream())
    L.call("sg_chol_lower", L.ptr(L2), n, L.ptr(flags) + 4, L.stream())
    if int(flags.abs().sum().item()) != 0:
        return float(frechet_inception_distance(mu1, s1, mu2, s2))
    B = torch.empty((n, n), dtype=torch.float64, device=dev)
    L.call("sg_dgemm_tn", L.ptr(L2), L.ptr(L1), L.ptr(B), n, L.stream())
    if ne != n:
        Bp = torch.zeros((ne, ne), dtype=torch.float64, device=dev)
        Bp[:n, :n] = B
        B = Bp
    nuc, _ = _nuclear_norm_sweeps(B, ne, max_sweeps, tol)
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * nuc)


# ---------------------------------------------------------------------------------------------------------
# the Frechet distance of small sample sets, many at a time (csrc/frechet_small.hip) -- intra-class FID
# ---------------------------------------------------------------------------------------------------------
def _host_ptr(a):
    return a.ctypes.data


SQUARE_ROUTE_MAX = 4096      # largest side of a cross-Gram matrix the padded square route takes: 128 MiB of fp64 and 4095 launches per Jacobi sweep


def takes_sample_route(na, nb, dim):
    """Whether a pair of sets with na and nb samples of width dim goes through the sample route (csrc/frechet_small.hip) in frechet_distance_from_features and
    intra_class_frechet. It does when (1) min(na, nb) <= dim -- a covariance is singular, the moment route would fall back to the host -- and (2) the
    min x max cross-Gram matrix either fits the in-LDS kernel (sg_seg_nuclear_fits) or has max(na, nb) <= SQUARE_ROUTE_MAX: beyond the LDS budget the matrix is
    padded to a max x max square, so a few fakes against a large real set (2000 against 50000) would mean a 20 GB matrix and 49999 launches per sweep; such a
    pair keeps the moment route (and its ~10 s of host time when a covariance is singular). Runs on the host."""
    r, c = int(min(na, nb)), int(max(na, nb))
    return r <= dim and (bool(L.lib().sg_seg_nuclear_fits(r, c)) or c <= SQUARE_ROUTE_MAX)


def _frechet_segments(fa, sega, fb, segb, names, max_sweeps, tol, workspace_bytes, stats=None):
    """Frechet distance of K pairs of row segments (fa rows sega[k]:sega[k+1] against fb rows segb[k]:segb[k+1]; fp32 contiguous device tensors, host int64 offsets)
    from the samples themselves: |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 |A B^T|_*. Classes are taken in chunks whose workspace (two [k][C] means and the
    cross-Gram matrices, fp64) stays under workspace_bytes (one class at least). Matrices within sg_seg_nuclear_fits take ONE in-LDS launch per chunk; the others
    are padded to an even square for sg_jacobi_sweep. names[k]: what to call pair k in an error. stats: optional dict that receives lists `sweeps`, `route`."""
    K, C = len(sega) - 1, fa.shape[1]
    dev = fa.device
    na, nb = np.diff(sega), np.diff(segb)
    for k in range(K):
        if na[k] < 2 or nb[k] < 2:
            raise ValueError(f"{names[k]}: {int(na[k])} and {int(nb[k])} samples; the Frechet distance needs at least 2 on both sides")
    r, c = np.minimum(na, nb), np.maximum(na, nb)
    cost = 8 * (2 * C + r * c)
    fits = L.lib().sg_seg_nuclear_fits
    out = np.empty(K, dtype=np.float64)
    k0 = 0
    while k0 < K:
        k1, used = k0 + 1, int(cost[k0])
        while k1 < K and used + int(cost[k1]) <= workspace_bytes:
            used += int(cost[k1])
            k1 += 1
        kc = k1 - k0
        sa, sb = np.ascontiguousarray(sega[k0:k1 + 1]), np.ascontiguousarray(segb[k0:k1 + 1])
        moff = np.zeros(kc + 1, dtype=np.int64)
        moff[1:] = np.cumsum(r[k0:k1] * c[k0:k1])
        mu = torch.empty((2, kc, C), dtype=torch.float64, device=dev)
        tr = torch.empty((2, kc), dtype=torch.float64, device=dev)
        M = torch.empty(int(moff[kc]), dtype=torch.float64, device=dev)
        st = L.stream()
        L.call("sg_seg_moments", L.ptr(fa), _host_ptr(sa), kc, C, L.ptr(mu[0]), L.ptr(tr[0]), st)
        L.call("sg_seg_moments", L.ptr(fb), _host_ptr(sb), kc, C, L.ptr(mu[1]), L.ptr(tr[1]), st)
        L.call("sg_seg_cross_gram", L.ptr(fa), _host_ptr(sa), L.ptr(mu[0]), L.ptr(fb), _host_ptr(sb), L.ptr(mu[1]), kc, C, L.ptr(M), _host_ptr(moff), st)
        rows, cols = r[k0:k1].astype(np.int32), c[k0:k1].astype(np.int32)
        lds = np.array([bool(fits(int(rows[i]), int(cols[i]))) for i in range(kc)])
        nuc = np.empty(kc, dtype=np.float64)
        swp = np.zeros(kc, dtype=np.int64)
        idx = np.nonzero(lds)[0]
        if len(idx):
            d_nuc = torch.empty((2, len(idx)), dtype=torch.float64, device=dev)
            d_swp = torch.empty(len(idx), dtype=torch.int32, device=dev)
            mo, ro, co = np.ascontiguousarray(moff[idx]), np.ascontiguousarray(rows[idx]), np.ascontiguousarray(cols[idx])
            L.call("sg_seg_nuclear_norm", L.ptr(M), _host_ptr(mo), _host_ptr(ro), _host_ptr(co), len(idx), max_sweeps, float(tol),
                   L.ptr(d_nuc[0]), L.ptr(d_nuc[1]), L.ptr(d_swp), st)
            h = d_nuc.cpu().numpy()
            nuc[idx], swp[idx] = h[0], d_swp.cpu().numpy()
            bad = np.nonzero(~(h[1] <= max(tol, 1e-8)))[0]      # (as the square route: a measure between tol and 1e-8 after max_sweeps is accepted)
            if len(bad):
                i = int(idx[bad[0]])
                raise RuntimeError(f"{names[k0 + i]}: one-sided Jacobi did not converge in {max_sweeps} sweeps (off-diagonal measure {float(h[1][bad[0]]):.2e})")
        for i in np.nonzero(~lds)[0]:
            ri, ci = int(rows[i]), int(cols[i])
            ne = ci + (ci & 1)
            B = torch.zeros((ne, ne), dtype=torch.float64, device=dev)
            B[:ri, :ci] = M[int(moff[i]):int(moff[i + 1])].view(ri, ci)
            nuc[i], swp[i] = _nuclear_norm_sweeps(B, ne, max_sweeps, tol)
        d2 = ((mu[0] - mu[1]) ** 2).sum(1)
        out[k0:k1] = (d2 + tr[0] + tr[1]).cpu().numpy() - 2.0 * nuc
        if stats is not None:
            stats.setdefault("sweeps", []).extend(int(v) for v in swp)
            stats.setdefault("route", []).extend("lds" if v else "square" for v in lds)
        k0 = k1
    return out


def _device_features(f, dev=None):
    """fp32 contiguous [n, dim] on `dev` (default: where f lives if that is a GPU, else the current GPU)"""
    f = torch.as_tensor(f)
    if dev is None:
        dev = f.device if f.is_cuda else torch.device("cuda", torch.cuda.current_device())
    f = f.to(device=torch.device(dev), dtype=torch.float32).contiguous()
    if f.dim() != 2:
        raise ValueError(f"features: a [n, dim] matrix expected, got {tuple(f.shape)}")
    return f


@torch.no_grad()
def frechet_distance_from_features(fa, fb, max_sweeps=40, tol=1e-12, device=None):
    """Frechet distance between the Gaussians fitted to two feature sets [na, dim], [nb, dim] (np.mean / np.cov of each, reference src/metrics/fid.py:94-98, then
    fid.py:34-62). min(na, nb) <= dim -- at least one covariance is singular, where the moment route below falls back to the host --: the sample route, from the
    centred rows themselves (csrc/frechet_small.hip), unless the larger set has more than SQUARE_ROUTE_MAX = 4096 rows and the cross-Gram matrix is beyond the
    LDS budget (takes_sample_route says which). Otherwise: the moments on the device and frechet_inception_distance_device. Returns a python float."""
    fa = _device_features(fa, device)
    fb = _device_features(fb, fa.device)
    na, nb, dim = fa.shape[0], fb.shape[0], fa.shape[1]
    if fb.shape[1] != dim:
        raise ValueError(f"feature widths differ: {dim} and {fb.shape[1]}")
    if takes_sample_route(na, nb, dim):
        seg = lambda n: np.array([0, n], dtype=np.int64)
        return float(_frechet_segments(fa, seg(na), fb, seg(nb), ["the pair of sets"], max_sweeps, tol, 1 << 62)[0])
    m1, s1 = calculate_moments(fa)
    m2, s2 = calculate_moments(fb)
    return frechet_inception_distance_device(m1, s1, m2, s2, device=fa.device, max_sweeps=max_sweeps, tol=tol)


def _class_counts(labels, n_rows, num_classes, what):
    """host labels [n] (int64) and the per-class counts; nothing here touches the device unless the labels live there"""
    lab = torch.as_tensor(labels).reshape(-1).cpu().numpy().astype(np.int64)
    if lab.shape[0] != n_rows:
        raise ValueError(f"{what}: {n_rows} feature rows and {lab.shape[0]} labels")
    if lab.size and (lab.min() < 0 or lab.max() >= num_classes):
        raise ValueError(f"{what}: labels outside [0, {num_classes})")
    return lab, np.bincount(lab, minlength=num_classes).astype(np.int64)


def _class_sorted(feats, lab, counts):
    """rows sorted by class (stable) and the int64 row offsets [num_classes + 1] of the classes"""
    order = torch.from_numpy(np.argsort(lab, kind="stable")).to(feats.device)
    seg = np.zeros(len(counts) + 1, dtype=np.int64)
    seg[1:] = np.cumsum(counts)
    return feats.index_select(0, order).contiguous(), seg


@torch.no_grad()
def intra_class_frechet(real_feats, real_labels, fake_feats, fake_labels, num_classes, max_sweeps=40, tol=1e-12, workspace_bytes=1 << 30, stats=None, device=None):
    """Per class the Frechet distance between that class's real and fake features (what reference src/worker.py:1380-1465 computes class by class with np.cov and
    scipy.linalg.sqrtm): float64 array [num_classes]. The rows are sorted by class once; all classes with min(n_real, n_fake) <= dim and at most
    SQUARE_ROUTE_MAX = 4096 samples a side (takes_sample_route) -- every class of every dataset the reference evaluates -- go through the batched sample route in chunks of at most workspace_bytes of fp64 workspace, the others through the moment
    route one by one. A class with fewer than 2 samples on either side raises ValueError naming it; a Jacobi measure above 1e-8 after max_sweeps raises
    RuntimeError. stats: optional dict, receives the sweeps and the route ("lds" / "square") of every sample-route class. device: where to compute (default: the
    features' GPU, else the current one)."""
    real_feats, fake_feats = torch.as_tensor(real_feats), torch.as_tensor(fake_feats)
    if real_feats.dim() != 2 or fake_feats.dim() != 2 or real_feats.shape[1] != fake_feats.shape[1]:
        raise ValueError(f"features: [n, dim] matrices of one width expected, got {tuple(real_feats.shape)} and {tuple(fake_feats.shape)}")
    dim = real_feats.shape[1]
    la, na = _class_counts(real_labels, real_feats.shape[0], num_classes, "real")
    lb, nb = _class_counts(fake_labels, fake_feats.shape[0], num_classes, "fake")
    for k in range(num_classes):
        if na[k] < 2 or nb[k] < 2:
            raise ValueError(f"class {k}: {int(na[k])} real and {int(nb[k])} fake samples; intra-class FID needs at least 2 of each")
    fa = _device_features(real_feats, device)
    fb = _device_features(fake_feats, fa.device)
    fa, sega = _class_sorted(fa, la, na)
    fb, segb = _class_sorted(fb, lb, nb)
    out = np.empty(num_classes, dtype=np.float64)
    small = np.array([takes_sample_route(na[k], nb[k], dim) for k in range(num_classes)])
    if small.all():
        out[:] = _frechet_segments(fa, sega, fb, segb, [f"class {k}" for k in range(num_classes)], max_sweeps, tol, workspace_bytes, stats)
    else:
        for k in range(num_classes):        # (some class keeps the moment route: class by class, each on its own route)
            a, b = fa[sega[k]:sega[k + 1]], fb[segb[k]:segb[k + 1]]
            if small[k]:
                out[k] = _frechet_segments(a, np.array([0, na[k]], dtype=np.int64), b, np.array([0, nb[k]], dtype=np.int64), [f"class {k}"], max_sweeps, tol,
                                           workspace_bytes, stats)[0]
            else:
                out[k] = frechet_distance_from_features(a, b, max_sweeps, tol, device=fa.device)
    return out


def calculate_intra_class_fid(generator, eval_model, real_feats, real_labels, num_classes, batch_size, z_dim, quantize=True, trim_last_batch=False,
                              world_size=1, DDP=False, device="cuda", z_prior="gaussian", truncation_factor=-1.0, MODEL=None, latent_opt=None, langevin=None,
                              max_sweeps=40, tol=1e-12, workspace_bytes=1 << 30):
    """reference src/worker.py:1380-1465 (`-ifid`): for every class c, n_c = that class's real samples; ceil(n_c / batch_size) batches of fakes with every label c
    (y_sampler=c), the first n_c rows kept; FID between the two; the mean over the classes. real_feats / real_labels: the eval model's features of the real
    images and their class labels (the reference recomputes them class by class from a per-class sampler: the same rows). Returns (mean, per_class float64
    [num_classes]). The feature extraction is the reference's loop (generate_images_and_stack_features and its sampling keywords); all the distances are then
    taken together on the device (intra_class_frechet).
    trim_last_batch: generate only the n_c % batch_size rows that are kept in the last batch, instead of a full batch whose tail is dropped (draws fewer latents
    than the reference, so a seeded run differs from it).
    Single process: world_size > 1 raises NotImplementedError (the reference gathers the ranks' features; here one process generates every class)."""
    if world_size > 1 or DDP:
        raise NotImplementedError("calculate_intra_class_fid runs in one process (world_size 1)")
    _, counts = _class_counts(real_labels, torch.as_tensor(real_feats).shape[0], num_classes, "real")
    for c in range(num_classes):
        if counts[c] < 2:
            raise ValueError(f"class {c}: {int(counts[c])} real samples; intra-class FID needs at least 2")
    kw = dict(quantize=quantize, device=device, z_prior=z_prior, truncation_factor=truncation_factor, MODEL=MODEL, latent_opt=latent_opt, langevin=langevin)
    feats, labels = [], []
    for c in range(num_classes):
        n = int(counts[c])
        full = (n // batch_size) * batch_size if trim_last_batch else n
        if full:
            f, _, _ = generate_images_and_stack_features(generator, eval_model, full, batch_size, z_dim, num_classes, y_sampler=c, **kw)
            feats.append(f[:full])
        if n - full:
            f, _, _ = generate_images_and_stack_features(generator, eval_model, n - full, n - full, z_dim, num_classes, y_sampler=c, **kw)
            feats.append(f)
        labels.append(torch.full((n,), c, dtype=torch.long))
    per_class = intra_class_frechet(real_feats, real_labels, torch.cat(feats, 0), torch.cat(labels, 0), num_classes, max_sweeps, tol, workspace_bytes)
    return float(per_class.mean()), per_class


def calculate_kl_div(ps, splits):
    """reference src/metrics/ins.py:28-42 (device tensors in, numpy scalars out)."""
    scores = []
    n = ps.shape[0]
    with torch.no_grad():
        for j in range(splits):
            part = ps[(j * n // splits):((j + 1) * n // splits), :]
            kl = part * (torch.log(part) - torch.log(torch.unsqueeze(torch.mean(part, 0), 0)))
            scores.append(torch.exp(torch.mean(torch.sum(kl, 1))).unsqueeze(0))
        scores = torch.cat(scores, 0)
        return torch.mean(scores).detach().cpu().numpy(), torch.std(scores).detach().cpu().numpy()


def top_k_accuracy(probs, labels, k, c0=1, ncls=1000):
    """Top-k accuracy over probs[:, c0:c0+ncls] with sklearn's tie rule, decided on the device (bit-exact integer
    logic; reference ins.py:75-76 slices classes 1..1000 and offsets the TF label by +1 -> pass 0-based class here)."""
    probs = probs.float().contiguous()
    lab = torch.as_tensor(labels, device=probs.device).long().contiguous()
    hits = torch.empty(probs.shape[0], dtype=torch.uint8, device=probs.device)
    L.call("sg_topk_hits", L.ptr(probs) + 4 * c0, probs.shape[1], ncls, L.ptr(lab), k, probs.shape[0], L.ptr(hits), L.stream())
    return float(hits.float().mean().item())


def load_ImageNet_label_dict(label_table_path):
    """reference src/utils/misc.py:582-595 (TF-Inception branch): `folder -> line index` of the reference's
    `src/utils/tf_imagenet_folder_label_pairs.txt` (1000 lines `n02119789 1 kit_fox`; the file stays in the StudioGAN checkout -- pass
    its path)."""
    d, label = {}, 0
    with open(label_table_path, "r") as f:
        for line in f:
            if not line.strip():
                continue
            d[line.split(" ")[0]] = label
            label += 1
    return d


def convert_labels(labels, class_to_idx, folder_label_dict):
    """loader label -> folder name -> TF-Inception class index (reference src/metrics/ins.py:48-49,68-70)."""
    loader_label_folder_dict = {v: k for k, v in class_to_idx.items()}
    return [folder_label_dict[loader_label_folder_dict[int(l)]] for l in labels]


def eval_features(probs, labels, num_features, split, is_acc, class_to_idx=None, folder_label_dict=None, topk_fn=None, is_torch_backbone=False):
    """reference src/metrics/ins.py:45-79 on ImageNet: IS over the first num_features rows; top-1 / top-5 of the remapped labels. TF-Inception
    (the default): against probs[:, 1:1001] (the reference passes `[i + 1 for i in converted]` with that slice to sklearn, which
    maps label i + 1 to column i: the same decision as testing 0-based class i here). is_torch_backbone (ins.py:57-66, DINO_torch and the other
    torch backbones): the classes are columns 0..999, no offset. The accuracy itself runs on the device (`top_k_accuracy`: sklearn's tie rule,
    bit-exact)."""
    topk_fn = topk_fn or top_k_accuracy
    probs, labels = probs[:num_features], labels[:num_features]
    m_scores, m_std = calculate_kl_div(probs, splits=split)
    top1, top5 = "N/A", "N/A"
    if is_acc:
        converted = convert_labels(labels, class_to_idx, folder_label_dict)
        c0 = 0 if is_torch_backbone else 1
        top1 = topk_fn(probs, converted, 1, c0, 1000)
        top5 = topk_fn(probs, converted, 5, c0, 1000)
    return m_scores, m_std, top1, top5


# ---------------------------------------------------------------------------------------------------------
# precision / recall / density / coverage on the device (reference src/metrics/prdc.py:87-168)
# ---------------------------------------------------------------------------------------------------------
def _sq_dist_block(xb, y, y_sq, out):
    """out[r][c] = |y_c|^2 - 2 x_r . y_c for a row block xb of X (exact-fp32 MFMA GEMM; |x_r|^2 is added by the consumer kernels)."""
    rows, C = xb.shape
    F.gemm_raw(L.F32, y, 0, C, xb, 0, C, out, y.shape[0], y.shape[0], rows, C, bias=y_sq, alpha=-2.0)
    return out


def _kth_nn_sq(feats, k, block=4096):
    """squared distance of every row to its k-th nearest neighbour, the row itself included (prdc.py:128-140 with k = nearest_k + 1)."""
    n, C = feats.shape
    sq = torch.empty(n, dtype=torch.float32, device=feats.device)
    L.call("sg_row_sqnorm", L.ptr(feats), n, C, L.ptr(sq), L.stream())
    out = torch.empty(n, dtype=torch.float32, device=feats.device)
    buf = torch.empty((min(block, n), n), dtype=torch.float32, device=feats.device)
    for r0 in range(0, n, block):
        xb = feats[r0:r0 + block]
        d = _sq_dist_block(xb, feats, sq, buf[:xb.shape[0]])
        L.call("sg_kth_smallest_rows", L.ptr(d), n, xb.shape[0], n, k, L.ptr(sq[r0:r0 + block]), L.ptr(out[r0:r0 + block]), L.stream())
    return out, sq


@torch.no_grad()
def compute_prdc(real_features, fake_features, nearest_k, block=4096):
    """reference src/metrics/prdc.py:143-168 `compute_prdc`: dict(precision, recall, density, coverage). Features: [N, dim] tensors
    (any float dtype / device; computed in fp32 on the GPU). Three blocked fp32 GEMMs + streaming row reductions replace
    sklearn.metrics.pairwise_distances(n_jobs=8) + np.argpartition over N x N float64 matrices; decisions are taken on squared
    distances (monotone), the manifold radii are the (nearest_k + 1)-th smallest self-inclusive distances exactly as in the reference."""
    assert 1 <= nearest_k < 16, "nearest_k + 1 <= 16 neighbours are kept per lane"
    dev = torch.device("cuda", torch.cuda.current_device()) if not (torch.is_tensor(real_features) and real_features.is_cuda) else real_features.device
    real = torch.as_tensor(real_features).to(device=dev, dtype=torch.float32).contiguous()
    fake = torch.as_tensor(fake_features).to(device=dev, dtype=torch.float32).contiguous()
    nr, nf = real.shape[0], fake.shape[0]
    r2_real, sq_real = _kth_nn_sq(real, nearest_k + 1, block)
    r2_fake, sq_fake = _kth_nn_sq(fake, nearest_k + 1, block)
    col_cnt = torch.zeros(nf, dtype=torch.int32, device=dev)
    row_any = torch.empty(nr, dtype=torch.uint8, device=dev)
    row_min = torch.empty(nr, dtype=torch.float32, device=dev)
    buf = torch.empty((min(block, nr), nf), dtype=torch.float32, device=dev)
    for r0 in range(0, nr, block):
        xb = real[r0:r0 + block]
        d = _sq_dist_block(xb, fake, sq_fake, buf[:xb.shape[0]])
        L.call("sg_prdc_rows", L.ptr(d), nf, xb.shape[0], nf, L.ptr(sq_real[r0:r0 + block]), L.ptr(r2_real[r0:r0 + block]), L.ptr(r2_fake), L.ptr(col_cnt),
               L.ptr(row_any[r0:r0 + block]), L.ptr(row_min[r0:r0 + block]), L.stream())
    cnt = col_cnt.double()
    precision = float((cnt > 0).double().mean())
    recall = float(row_any.double().mean())
    density = float(cnt.mean() / float(nearest_k))
    coverage = float((row_min < r2_real).double().mean())
    return dict(precision=precision, recall=recall, density=density, coverage=coverage)


def calculate_pr_dc(real_feats, fake_feats, num_generate, nearest_k):
    """reference src/metrics/prdc.py:66-84 with the features already extracted (the fake stack is truncated to num_generate first)."""
    m = compute_prdc(real_feats, fake_feats[:num_generate], nearest_k)
    return m["precision"], m["recall"], m["density"], m["coverage"]
