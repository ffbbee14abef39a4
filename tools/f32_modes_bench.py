"""The three fp32 arithmetic modes of the generic engine side by side (functional.f32_mode: exact = v_mfma_f32_32x32x2_f32, bf16x3 and bf16x6 = operands split
into two / three bf16 terms, three / six bf16 MFMAs per k-tile), in ONE process, interleaved in ABBA order (exact, bf16x3, bf16x6, bf16x6, bf16x3, exact per round)
so that clock drift and other tenants of the box hit every mode alike:
  (a) the Inception-like layer shapes of tests/test_kernels_gpu.py F32_SPLIT_CASES at batch 64, forward and weight gradient
  (b) the InceptionV3 forward at 299 x 299, B = 64 (seeded synthetic weights)
  (c) the fp32 DINO ViT-S/8 forward at 224 x 224, B = 16 (seeded random weights)
Prints per workload and mode: ms (median of the rounds' event-timed means) and algorithmic TFLOP/s; plus the distance of each split mode's Inception / DINO
output from the exact mode's. bf16x3 is convolution-only: in (c) it reaches nothing (the 3-channel patch embedding misses the all-vector path), the row is
there as the second "exact" measurement it is.
    python tools/f32_modes_bench.py [--rounds 3] > profiles/f32_modes_bench.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from studiogan_amd import functional as F, _lib as L, metrics as M  # noqa: E402

MODES = ("exact", "bf16x3", "bf16x6")
ABBA = MODES + MODES[::-1]
# N, Cin, Cout, H, W, R, S, stride, (ph, pw): tests/test_kernels_gpu.py F32_SPLIT_CASES; N is replaced by the batch
LAYERS = [(2, 64, 96, 17, 17, 3, 3, 1, (1, 1)), (2, 192, 32, 9, 9, 1, 1, 1, (0, 0)), (1, 128, 160, 17, 17, 1, 7, 1, (0, 3)), (1, 160, 192, 17, 17, 7, 1, 1, (3, 0)),
          (2, 48, 64, 13, 13, 5, 5, 1, (2, 2)), (2, 288, 384, 17, 17, 3, 3, 2, (0, 0)), (1, 384, 384, 8, 8, 3, 3, 1, (1, 1))]
INCEPTION_GFLOP = 11.4       # InceptionV3 at 299 x 299, 2 * MACs per image (tools/fid_leg.py)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def abba(fn, iters, rounds):
    """{mode: median over 2 * rounds samples of the mean ms of `iters` calls}; every mode warmed up first"""
    ms = {m: [] for m in MODES}
    for m in MODES:
        with F.f32_mode(m):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for m in ABBA:
            with F.f32_mode(m):
                ms[m].append(timed(fn, iters))
    return {m: statistics.median(v) for m, v in ms.items()}


def abba_models(models, x, iters, rounds):
    """abba() for evaluation models, each of which applies the mode of its name itself (and has run once already)"""
    ms = {m: [] for m in MODES}
    for _ in range(rounds):
        for m in ABBA:
            ms[m].append(timed(lambda: models[m].forward_nhwc(x), iters))
    return {m: statistics.median(v) for m, v in ms.items()}


def split_launches_of(model, x):
    """launches of one forward that take the bf16x6 path (sg_f32_split_launches)"""
    n0 = L.lib().sg_f32_split_launches(6)
    model.forward_nhwc(x)
    torch.cuda.synchronize()
    return L.lib().sg_f32_split_launches(6) - n0


def row(name, ms, gflop):
    cells = "  ".join(f"{m} {ms[m]:9.4f} ms {gflop / ms[m]:7.1f} TF/s" for m in MODES)
    print(f"{name:58s} {cells}  | x3/exact {ms['exact'] / ms['bf16x3']:5.2f}x  x6/exact {ms['exact'] / ms['bf16x6']:5.2f}x", flush=True)


def dino_state_dict(seed, geo):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in M.dino_manifest(geo["embed"], geo["depth"], geo["patch"], geo["tokens"], geo["classes"]).items():
        if "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif k.endswith("weight") and len(shape) >= 2:
            fan = 1
            for s in shape[1:]:
                fan *= s
            sd[k] = torch.randn(shape, generator=g) * fan ** -0.5
        else:
            sd[k] = 0.1 * torch.randn(shape, generator=g)
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="batch of the layer shapes and of the Inception forward")
    ap.add_argument("--dino-batch", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}; rounds {args.rounds} x ABBA ({' '.join(ABBA)}); ms = median of {2 * args.rounds} event-timed means", flush=True)
    g = torch.Generator().manual_seed(0)
    print(f"# (a) layer shapes at batch {args.batch}: N, Cin, Cout, H, W, R, S, stride, pad")
    for case in LAYERS:
        _, Cin, Cout, H, W, R, S, stride, (ph, pw) = case
        N = args.batch
        x = torch.randn(N, H, W, Cin, generator=g).to(dev)
        w = (torch.randn(Cout, R, S, Cin, generator=g) * 0.2).to(dev)
        Ho, Wo = (H + 2 * ph - R) // stride + 1, (W + 2 * pw - S) // stride + 1
        dy = torch.randn(N, Ho, Wo, Cout, generator=g).to(dev)
        dw = torch.zeros(Cout, R, S, Cin, device=dev)
        gflop = 2.0 * N * Ho * Wo * Cout * R * S * Cin / 1e9
        out = torch.empty(N, Ho, Wo, Cout, device=dev)
        row(f"fwd   {(N,) + case[1:]}", abba(lambda: F.conv2d_raw(x, w.data_ptr(), Cin, Cout, R, S, stride, ph, pw, out=out), 20, args.rounds), gflop)
        row(f"wgrad {(N,) + case[1:]}", abba(lambda: F.conv2d_wgrad_raw(x, dy, dw.data_ptr(), Cin, Cout, R, S, Ho, Wo, stride, ph, pw), 20, args.rounds), gflop)

    def distance(outs, names):
        for i, n in enumerate(names):
            ref = outs["exact"][i]
            print("#     " + n + ": distance to the exact mode's output, of its range: " +
                  "  ".join(f"{m} {float((outs[m][i] - ref).abs().max() / ref.abs().max()):.2e}" for m in MODES[1:]), flush=True)

    print(f"# (b) InceptionV3 forward, 299 x 299, B = {args.batch}, fp32 tensors")
    xi = (torch.rand(args.batch, 299, 299, 3, generator=g) * 2 - 1).to(dev)
    sd = M.synthetic_state_dict(0)
    models = {m: M.InceptionV3(sd, dev, torch.float32, f32_mode=m) for m in MODES}
    distance({m: models[m].forward_nhwc(xi) for m in MODES}, ("pool3 features", "logits"))
    print(f"#     bf16x6: {split_launches_of(models['bf16x6'], xi)} of the forward's 95 contraction launches (94 convolutions + fc) take the split path; "
          "the rest (3 input channels) keep the exact MFMA", flush=True)
    ms = abba_models(models, xi, 3, args.rounds)
    row(f"InceptionV3 forward B={args.batch}", ms, INCEPTION_GFLOP * args.batch)
    print("#     samples/s: " + "  ".join(f"{m} {args.batch / ms[m] * 1e3:8.1f}" for m in MODES), flush=True)
    del models, xi

    B = args.dino_batch
    print(f"# (c) DINO ViT-S/8 forward, 224 x 224, B = {B}, fp32 tensors")
    geo = dict(embed=384, depth=12, patch=8, tokens=785, classes=1000)
    sd = dino_state_dict(1, geo)
    C, N, D = geo["embed"], geo["tokens"], geo["depth"]
    gflop = B * (D * (2.0 * N * 12 * C * C + 4.0 * N * N * C) + 2.0 * (N - 1) * 3 * 64 * C + 2.0 * 4 * C * geo["classes"]) / 1e9
    xd = torch.randn(B, 224, 224, 3, generator=g).to(dev)
    models = {m: M.DINOViT(sd, dev, torch.float32, f32_mode=m) for m in MODES}
    distance({m: models[m].forward_nhwc(xd) for m in MODES}, ("embedding", "logits"))
    heads = C // 64
    print(f"#     bf16x6: {split_launches_of(models['bf16x6'], xd)} of the forward's {D * (4 + 2 * heads) + 2} contraction launches take the split path; the "
          f"{D * heads} P V products ({N} tokens: not a multiple of 4) and the 3-channel patch embedding keep the exact MFMA "
          f"({100.0 * (D * 2.0 * N * N * C + 2.0 * (N - 1) * 192 * C) * B / 1e9 / gflop:.0f} % of the FLOPs)", flush=True)
    ms = abba_models(models, xd, 2, args.rounds)
    row(f"DINO ViT-S/8 forward B={B}", ms, gflop)
    print("#     images/s: " + "  ".join(f"{m} {B / ms[m] * 1e3:8.1f}" for m in MODES), flush=True)


if __name__ == "__main__":
    main()
