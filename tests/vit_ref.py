"""Plain-torch functional restatement of the ViT forward behind eval_backbone "DINO_torch" (reference src/metrics/vit.py), written from the
mathematics: patch embedding, pre-norm transformer blocks, class tokens of the last blocks through the final norm, linear head. Works in any
float dtype (the GPU tests run it in fp64 on the CPU as their oracle); tests/make_golden_vit.py pins it bit for bit to the reference's module."""
import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-6
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

SMALL = dict(embed=128, depth=5, heads=2, patch=8, img=32, classes=10, num_last_blocks=4)          # 17 tokens: the committed fixture
VIT_S8 = dict(embed=384, depth=12, heads=6, patch=8, img=224, classes=1000, num_last_blocks=4)     # 785 tokens: DINO_torch


def tokens_of(geo):
    return 1 + (geo["img"] // geo["patch"]) ** 2


def random_state_dict(seed, geo):
    """Seeded weights under the reference's key names that EXERCISE the kernels: query / key weights scaled so that a score row spreads over
    several units (the reference's 0.02 initialisation gives a near-uniform softmax and would hide an attention bug), non-zero biases,
    LayerNorm gains away from 1, non-zero cls_token / pos_embed."""
    g = torch.Generator().manual_seed(seed)
    C, hidden, p, nlb = geo["embed"], 4 * geo["embed"], geo["patch"], geo["num_last_blocks"]
    rn = lambda *s: torch.randn(*s, generator=g)
    gain = lambda: 0.6 + 0.8 * torch.rand(C, generator=g)
    sd = {"cls_token": 0.5 * rn(1, 1, C), "pos_embed": 0.5 * rn(1, tokens_of(geo), C),
          "patch_embed.proj.weight": rn(C, 3, p, p) / math.sqrt(3 * p * p), "patch_embed.proj.bias": 0.2 * rn(C)}
    for i in range(geo["depth"]):
        b = f"blocks.{i}."
        qkv = rn(3 * C, C) / math.sqrt(C)
        qkv[:2 * C] *= math.sqrt(3.0)          # scores = q . k / 8 with std ~ 3 * gain^2
        sd[b + "norm1.weight"], sd[b + "norm1.bias"] = gain(), 0.2 * rn(C)
        sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"] = qkv, 0.2 * rn(3 * C)
        sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"] = rn(C, C) / math.sqrt(C), 0.2 * rn(C)
        sd[b + "norm2.weight"], sd[b + "norm2.bias"] = gain(), 0.2 * rn(C)
        sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"] = rn(hidden, C) / math.sqrt(C), 0.2 * rn(hidden)
        sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"] = rn(C, hidden) / math.sqrt(hidden), 0.2 * rn(C)
    sd["norm.weight"], sd["norm.bias"] = gain(), 0.2 * rn(C)
    sd["linear.weight"], sd["linear.bias"] = rn(geo["classes"], nlb * C) / math.sqrt(nlb * C), 0.1 * rn(geo["classes"])
    return sd


def attention(qkv, heads):
    """qkv [B, N, 3 * C] packed as (3, heads, C / heads) along the last axis -> softmax(q k^T / sqrt(d)) v, [B, N, C]"""
    B, N, C3 = qkv.shape
    C = C3 // 3
    d = C // heads
    qkv = qkv.reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    a = (q @ k.transpose(-2, -1)) * d ** -0.5
    a = a.softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(B, N, C)


def vit_forward(sd, x, heads, num_last_blocks=4, eps=LN_EPS):
    """x [B, 3, H, W] normalised images, H = W = grid * patch -> (embed [B, num_last_blocks * C], logits [B, classes])"""
    C = sd["cls_token"].shape[-1]
    p = sd["patch_embed.proj.weight"].shape[-1]
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    t = torch.cat((sd["cls_token"].expand(x.shape[0], -1, -1), t), dim=1)
    assert t.shape[1] == sd["pos_embed"].shape[1], "native patch grid only"
    t = t + sd["pos_embed"]
    depth = 0
    while f"blocks.{depth}.norm1.weight" in sd:
        depth += 1
    outs = []
    for i in range(depth):
        b = f"blocks.{i}."
        y = F.layer_norm(t, (C,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], eps)
        y = attention(F.linear(y, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]), heads)
        t = t + F.linear(y, sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
        y = F.layer_norm(t, (C,), sd[b + "norm2.weight"], sd[b + "norm2.bias"], eps)
        y = F.gelu(F.linear(y, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"]))
        t = t + F.linear(y, sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"])
        if depth - i <= num_last_blocks:
            outs.append(F.layer_norm(t, (C,), sd["norm.weight"], sd["norm.bias"], eps)[:, 0])
    embed = torch.cat(outs, dim=-1)
    return embed, F.linear(embed, sd["linear.weight"], sd["linear.bias"])


def vit_forward_f64(sd, x, heads, num_last_blocks=4):
    sd64 = {k: v.double() for k, v in sd.items()}
    e, l = vit_forward(sd64, x.double(), heads, num_last_blocks)
    return e, l


def small_input(seed=1, batch=3, geo=SMALL):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 3, geo["img"], geo["img"], generator=g)
