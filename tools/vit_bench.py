"""DINO ViT-S/8 feature extraction (metrics.DINOViT, eval_backbone "DINO_torch") on seeded weights and images resident in HBM:
    python tools/vit_bench.py [--batches 64,256] [--rounds 5] [--iters 3] [--no-fp32]
1. samples/s of the fused bf16 path and the composed fp32 path, interleaved in ONE process over several rounds (median and min of the per-round times,
   device-synchronised around every timed region);
2. a per-kernel table for one bf16 forward at the first batch size: every launch family timed on its own over the real shapes -- ms per forward,
   algorithmic TF/s for the GEMMs and attention, algorithmic GB/s for LayerNorm / tokens. Consecutive launches of a family walk through SETS separate sets
   of activation buffers (together several times the 256 MiB Infinity Cache), so a launch finds none of its activations on chip and the GB/s column is an
   HBM figure (inside a forward a consumer may find part of what its producer just wrote in the cache: the sum of the families is an upper bound).
Inputs are Gaussian images of the normalised range and seeded Gaussian weights (synthetic_state_dict): never zeros (they would collapse the softmax work
and flatter the clocks). There is no fallback: without a GPU the tool fails."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import studiogan_amd  # noqa: E402,F401
from studiogan_amd import metrics as M, _lib as L, functional as F  # noqa: E402


SETS = 6


def synthetic_state_dict(seed=0, embed=384, depth=12, patch=8, img=224, classes=1000, num_last_blocks=4):
    """Seeded random ViT weights under the reference's names, for throughput measurements when the published files are not available. Query / key
    weights are scaled so that the softmax rows are far from uniform (the 0.02 initialisation would make attention an average)."""
    g = torch.Generator().manual_seed(seed)
    tokens, hidden = 1 + (img // patch) ** 2, 4 * embed
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"cls_token": 0.5 * rn(1, 1, embed), "pos_embed": 0.5 * rn(1, tokens, embed),
          "patch_embed.proj.weight": rn(embed, 3, patch, patch) / math.sqrt(3 * patch * patch), "patch_embed.proj.bias": 0.1 * rn(embed)}
    for i in range(depth):
        p = f"blocks.{i}."
        qkv = rn(3 * embed, embed) / math.sqrt(embed)
        qkv[:2 * embed] *= math.sqrt(3.0)
        sd[p + "norm1.weight"], sd[p + "norm1.bias"] = 0.75 + 0.5 * torch.rand(embed, generator=g), 0.1 * rn(embed)
        sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"] = qkv, 0.1 * rn(3 * embed)
        sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = rn(embed, embed) / math.sqrt(embed), 0.1 * rn(embed)
        sd[p + "norm2.weight"], sd[p + "norm2.bias"] = 0.75 + 0.5 * torch.rand(embed, generator=g), 0.1 * rn(embed)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(hidden, embed) / math.sqrt(embed), 0.1 * rn(hidden)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(embed, hidden) / math.sqrt(hidden), 0.1 * rn(embed)
    sd["norm.weight"], sd["norm.bias"] = 0.75 + 0.5 * torch.rand(embed, generator=g), 0.1 * rn(embed)
    sd["linear.weight"], sd["linear.bias"] = rn(classes, num_last_blocks * embed) / math.sqrt(num_last_blocks * embed), 0.01 * rn(classes)
    return sd


def timed(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_table(model, B, iters):
    g = model.geometry
    C, N, Hd, H, depth = g["embed"], g["tokens"], g["hidden"], g["heads"], g["depth"]
    M_, dev, bf = B * N, model.device, torch.bfloat16
    st = L.stream()
    w = model.blocks[depth // 2]
    side = g["grid"] * g["patch"]
    sets = [dict(xs=torch.randn(M_, C, device=dev), y=torch.randn(M_, C, device=dev).to(bf), qkv=torch.randn(M_, 3 * C, device=dev).to(bf),
                 att=torch.randn(M_, C, device=dev).to(bf), hid=torch.randn(M_, Hd, device=dev).to(bf), img=torch.randn(B, side, side, 3, device=dev).to(bf),
                 patches=torch.randn(B, N - 1, C, device=dev), emb=torch.empty(B, 4 * C, device=dev)) for _ in range(SETS)]
    per_set = sum(t.numel() * t.element_size() for t in sets[0].values())
    T = lambda i: sets[i % SETS]

    def gemm(epi, a, lda, wk, bk, out, ldo, n, k):
        return lambda i: L.call("sg_tok_gemm", epi, L.ptr(T(i)[a]), lda, L.ptr(w[wk]), L.ptr(w[bk]), L.ptr(T(i)[out]), ldo, M_, n, k, st)
    rows = [
        ("patch conv 8x8/8 (generic engine)", 1, lambda i: F.conv2d_raw(T(i)["img"], model.patch_w.data_ptr(), 3, C, g["patch"], g["patch"], stride=g["patch"], epi_flags=L.EPI_OUT_F32,
                                                                         bias=model.patch_b, out=T(i)["patches"].view(B, g["grid"], g["grid"], C)),
         2.0 * B * (N - 1) * C * 3 * g["patch"] ** 2, 2.0 * B * side * side * 3 + 4.0 * B * (N - 1) * C),
        ("sg_vit_tokens", 1, lambda i: L.call("sg_vit_tokens", L.ptr(T(i)["patches"]), L.ptr(model.cls), L.ptr(model.pos), L.ptr(T(i)["xs"]), B, N, C, st), 0.0, 4.0 * (B * (N - 1) * C + M_ * C)),
        ("sg_layernorm_rows -> bf16", 2 * depth, lambda i: model._ln(T(i)["xs"], M_, C, w["norm1.weight"], w["norm1.bias"], T(i)["y"], C), 0.0, 6.0 * M_ * C),
        ("sg_tok_gemm qkv (bias)", depth, gemm(0, "y", C, "attn.qkv.weight", "attn.qkv.bias", "qkv", 3 * C, 3 * C, C), 2.0 * M_ * 3 * C * C, 2.0 * M_ * 4 * C),
        ("sg_mha_fwd", depth, lambda i: L.call("sg_mha_fwd", L.ptr(T(i)["qkv"]), L.ptr(T(i)["att"]), B, N, H, 64, model.scale, st), 4.0 * B * H * N * N * 64, 2.0 * M_ * 4 * C),
        ("sg_tok_gemm proj (+= residual)", depth, gemm(2, "att", C, "attn.proj.weight", "attn.proj.bias", "xs", C, C, C), 2.0 * M_ * C * C, 2.0 * M_ * C + 8.0 * M_ * C),
        ("sg_tok_gemm fc1 (bias + GELU)", depth, gemm(1, "y", C, "mlp.fc1.weight", "mlp.fc1.bias", "hid", Hd, Hd, C), 2.0 * M_ * Hd * C, 2.0 * M_ * (C + Hd)),
        ("sg_tok_gemm fc2 (+= residual)", depth, gemm(2, "hid", Hd, "mlp.fc2.weight", "mlp.fc2.bias", "xs", C, C, Hd), 2.0 * M_ * Hd * C, 2.0 * M_ * Hd + 8.0 * M_ * C),
        ("final norm of the class rows", 4, lambda i: L.call("sg_layernorm_rows", L.F32, L.ptr(T(i)["xs"]), N * C, L.ptr(model.norm_w), L.ptr(model.norm_b), L.ptr(T(i)["emb"]), 4 * C, B, C,
                                                             M.LN_EPS, st), 0.0, 8.0 * B * C),
    ]
    print(f"per-kernel table, one bf16 forward at B = {B} ({M_} token rows); each family timed alone, {iters} launches rotating over {SETS} buffer sets "
          f"of {per_set / 2 ** 20:.0f} MiB each (operands never cache-resident)")
    print(f"{'kernel':36s} {'calls':>5s} {'ms/call':>9s} {'ms/fwd':>9s} {'TF/s':>8s} {'GB/s':>8s}")
    total = 0.0
    for name, calls, fn, flops, nbytes in rows:
        for i in range(SETS):
            fn(i)
        ms = timed(fn, iters)
        total += ms * calls
        tf = f"{flops / ms / 1e9:8.1f}" if flops else f"{'':8s}"
        print(f"{name:36s} {calls:5d} {ms:9.4f} {ms * calls:9.3f} {tf} {nbytes / ms / 1e6:8.0f}")
    print(f"{'sum of the families':36s} {'':5s} {'':9s} {total:9.3f}   -> {B / total * 1e3:.0f} img/s if nothing else cost time")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-fp32", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vit_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    sd = synthetic_state_dict(0)
    models = {"bf16": M.DINOViT(sd, dev, torch.bfloat16)}
    if not args.no_fp32:
        models["fp32"] = M.DINOViT(sd, dev, torch.float32)
    gflop = 45.0
    print(f"device: {torch.cuda.get_device_name(0)}; ViT-S/8 at 224^2, 785 tokens, ~{gflop:.0f} GFLOP per image")
    for B in [int(b) for b in args.batches.split(",")]:
        torch.manual_seed(B)
        x = torch.randn(B, 224, 224, 3, device=dev)
        xin = {"bf16": x.to(torch.bfloat16), "fp32": x}
        times = {k: [] for k in models}
        for k, m in models.items():       # warm every shape of the timed window
            m.forward_nhwc(xin[k])
        for _ in range(args.rounds):
            for k, m in models.items():   # interleaved: both paths see the same clocks and neighbours
                times[k].append(timed(lambda i: m.forward_nhwc(xin[k]), args.iters if k == "bf16" else 1))
        for k, t in times.items():
            med, mn = statistics.median(t), min(t)
            print(f"B={B:4d} {k}: median {med:9.2f} ms  min {mn:9.2f} ms  -> {B / med * 1e3:9.0f} img/s (median)  {B / mn * 1e3:9.0f} img/s (best)  "
                  f"{gflop * B / med:8.1f} TF/s end to end")
    kernel_table(models["bf16"], int(args.batches.split(",")[0]), 24)


if __name__ == "__main__":
    main()
