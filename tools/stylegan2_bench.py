"""StyleGAN2 generator: what the fused up = 2 layer tail (csrc/style_fir.hip) and the grouped style affines (sg_linear_group_scaled) are worth.
    python tools/stylegan2_bench.py [--batch 32] [--rounds 3] [--iters 5] [--window-ms 200] [--parts layer,cifar,g256] [--out profiles/stylegan2_gen_bench.txt]
Three parts, every contender of a part in one process, taking turns inside every round:
  layer   one up = 2 synthesis layer (modulated convolution, FIR, noise, bias, lrelu, clamp 256) at the widths of a StyleGAN2-256 synthesis network, batch
          --batch, bf16 and fp32, per-sample noise: `fused` = style_ops.modulated_conv2d_act (transposed convolution + ONE sg_fir_bias_act_nhwc),
          `chain` = modulated_conv2d + bias_act (transposed convolution, NHWC->NCHW copy, sg_upfirdn2d, noise add, NCHW->NHWC copy, sg_bias_act);
          forward, and forward + backward (dx, dweight, dstyles, dnoise, dbias). `tail` = the fused kernel's forward launch alone on a given core, with the
          bytes it must move (core in, activation out) over its time.
  cifar   Generator forward and forward + backward (all parameter gradients and dz) at the CIFAR10 configuration: 32^2, 512 channels, w_dim 512, two
          mapping layers, 10 classes, batch 64, fp32
  g256    the same at 256^2 (channel_base 16384, eight mapping layers, unconditional), batch 32, the four highest resolutions in bf16, conv_clamp 256
each network with the fused tail on / off and the grouped affines on / off (SynthesisBlock.fused_resample, SynthesisNetwork.grouped_styles): `off / off` is the
layer-by-layer evaluation. Timing as tools/modconv_bench.py: device events around a window of back-to-back calls after 3 warm-up calls, a window of at least
--iters calls and --window-ms of work, --rounds rounds in alternating order, the median reported. There is no fallback: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import studiogan_amd  # noqa: E402,F401
from studiogan_amd.backbones.stylegan2 import Generator  # noqa: E402
from studiogan_amd.style_ops import upfirdn2d as U  # noqa: E402
from studiogan_amd.style_ops.bias_act import bias_act  # noqa: E402
from studiogan_amd.style_ops.fir_bias_act import fir_nhwc_raw  # noqa: E402
from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d, modulated_conv2d_act  # noqa: E402

SQRT2 = 2 ** 0.5


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def contest(fns, a):
    """median ms per call of every contender: warm-up, window calibration, then --rounds rounds in alternating order"""
    n_it = {}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()      # an error of this contender surfaces here, under its name
        n_it[k] = max(a.iters, min(5000, int(a.window_ms / max(timed(fn, a.iters), 1e-3)) + 1))
    t = {k: [] for k in fns}
    order = list(fns)
    for r in range(a.rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            t[k].append(timed(fns[k], n_it[k]))
    return {k: statistics.median(v) for k, v in t.items()}, n_it


def layer_part(a, dev, say):
    say(f"## one up = 2 layer, batch {a.batch}: ms per call; ratio = chain / fused (> 1: the fused tail is faster)")
    say(f"{'shape':>12s} {'dtype':>5s} | {'fused fwd':>9s} {'chain fwd':>9s} {'ratio':>6s} | {'fused f+b':>9s} {'chain f+b':>9s} {'ratio':>6s} | {'tail fwd':>8s} {'GB/s':>6s}")
    f = U.setup_filter([1, 3, 3, 1], device=dev)
    for shape in a.layer_shapes.split(","):
        C, H = (int(v) for v in shape.split("x"))
        N, Ho = a.batch, 2 * H
        for dtype in (torch.bfloat16, torch.float32):
            g = torch.Generator(device=dev).manual_seed(C * 1000 + H)
            x = torch.randn(N, C, H, H, generator=g, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
            w = torch.randn(C, C, 3, 3, generator=g, device=dev)
            s = 1 + torch.randn(N, C, generator=g, device=dev)
            noise = torch.randn(N, 1, Ho, Ho, generator=g, device=dev)
            bias = torch.randn(C, generator=g, device=dev)
            gy = torch.randn(N, C, Ho, Ho, generator=g, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
            kw = dict(up=2, padding=1, resample_filter=f, flip_weight=False)
            epi = dict(act="lrelu", gain=SQRT2, clamp=256)
            leaves = [t.clone().requires_grad_(True) for t in (x, w, s, noise, bias)]

            def fused(x, w, s, nz, b):
                return modulated_conv2d_act(x, w, s, noise=nz, bias=b, **epi, **kw)

            def chain(x, w, s, nz, b):
                y = modulated_conv2d(x, w, s, noise=nz, **kw)
                return bias_act(y, b.to(y.dtype), **epi)

            def fwd(op):
                def run():
                    with torch.no_grad():
                        return op(x, w, s, noise, bias)
                return run

            def fb(op):
                return lambda: torch.autograd.grad(op(*leaves), leaves, gy)

            core = torch.randn(N, 2 * H + 1, 2 * H + 1, C, generator=g, device=dev).to(dtype)
            nz32 = noise.contiguous()

            def tail():
                return fir_nhwc_raw(core, f, (1, 1, 1, 1), False, 4.0, nz32, Ho * Ho, bias, "lrelu", 0.2, SQRT2, 256.0)

            ref = fwd(chain)().float()
            err = float((fwd(fused)().float() - ref).abs().max() / ref.abs().max())
            assert err < (5e-2 if dtype == torch.bfloat16 else 1e-4), (shape, dtype, err)      # the two compute the same function, at the size that is timed
            m, n_it = contest({"fused fwd": fwd(fused), "chain fwd": fwd(chain), "fused f+b": fb(fused), "chain f+b": fb(chain), "tail": tail}, a)
            nbytes = (core.numel() + N * Ho * Ho * C) * core.element_size() + noise.numel() * 4
            say(f"{shape + 'up':>12s} {'bf16' if dtype == torch.bfloat16 else 'fp32':>5s} | {m['fused fwd']:9.3f} {m['chain fwd']:9.3f} {m['chain fwd'] / m['fused fwd']:6.2f} | "
                f"{m['fused f+b']:9.3f} {m['chain f+b']:9.3f} {m['chain f+b'] / m['fused f+b']:6.2f} | {m['tail']:8.3f} {nbytes / m['tail'] / 1e6:6.0f}"
                f"   (fused vs chain forward: {err:.1e} of range; calls per window {'/'.join(str(v) for v in n_it.values())})")
            del leaves, x, gy, ref, core
            torch.cuda.empty_cache()


def network_part(name, a, dev, say, batch, kwargs, note):
    model = types.SimpleNamespace(info_type="N/A")
    G = Generator(MODEL=model, **kwargs).to(dev)
    with torch.no_grad():      # a trained generator has noise: strength 0 would still run every launch, nonzero keeps the numbers honest
        for n_, p in G.named_parameters():
            if n_.endswith("noise_strength"):
                p.fill_(0.1)
    g = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(batch, G.z_dim, generator=g, device=dev)
    c = torch.eye(max(G.c_dim, 1), device=dev)[torch.arange(batch, device=dev) % max(G.c_dim, 1)][:, :G.c_dim]
    params = [p for p in G.parameters()]
    gy = torch.randn(batch, 3, G.img_resolution, G.img_resolution, generator=g, device=dev)

    def setup(fused, grouped):
        G.synthesis.grouped_styles = grouped
        for b in G.synthesis.blocks():
            b.fused_resample = fused

    def fwd(fused, grouped):
        def run():
            setup(fused, grouped)
            with torch.no_grad():
                return G(z, c, noise_mode="random")
        return run

    def fb(fused, grouped):
        def run():
            setup(fused, grouped)
            zl = z.clone().requires_grad_(True)
            return torch.autograd.grad(G(zl, c, noise_mode="random"), [zl] + params, gy, allow_unused=True)
        return run

    combos = [(True, True), (False, True), (True, False), (False, False)]
    label = lambda fu, gr: f"tail {'on ' if fu else 'off'} affines {'on ' if gr else 'off'}"      # noqa: E731
    fns = {}
    for fu, gr in combos:
        fns[label(fu, gr) + " fwd"] = fwd(fu, gr)
        fns[label(fu, gr) + " f+b"] = fb(fu, gr)
    m, n_it = contest(fns, a)
    say(f"## {name}: Generator, batch {batch}, {note}: ms per call; ratio = (off, off) / this row")
    say(f"{'fused tail':>10s} {'grouped affines':>15s} | {'forward':>8s} {'ratio':>6s} | {'fwd+bwd':>8s} {'ratio':>6s} | calls per window")
    base_f, base_b = m[label(False, False) + " fwd"], m[label(False, False) + " f+b"]
    for fu, gr in combos:
        tf, tb = m[label(fu, gr) + " fwd"], m[label(fu, gr) + " f+b"]
        say(f"{'on' if fu else 'off':>10s} {'on' if gr else 'off':>15s} | {tf:8.3f} {base_f / tf:6.2f} | {tb:8.3f} {base_b / tb:6.2f} | "
            f"{n_it[label(fu, gr) + ' fwd']}/{n_it[label(fu, gr) + ' f+b']}")
    del G, params
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--parts", default="layer,cifar,g256")
    ap.add_argument("--layer-shapes", default="512x16,512x32,256x64,128x128")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stylegan2_gen_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/stylegan2_bench.py --batch {a.batch} --rounds {a.rounds} --iters {a.iters} --window-ms {a.window_ms:g} --parts {a.parts}    ({torch.cuda.get_device_name(0)})")
    say("# median over rounds of event-timed windows; the contenders of a part alternate inside a round")
    parts = a.parts.split(",")
    if "layer" in parts:
        layer_part(a, dev, say)
    syn = lambda base, res, clamp: {"channel_base": base, "channel_max": 512, "num_fp16_res": res, "conv_clamp": clamp}      # noqa: E731
    if "cifar" in parts:
        network_part("cifar", a, dev, say, 64, dict(z_dim=512, c_dim=10, w_dim=512, img_resolution=32, img_channels=3, mapping_kwargs={"num_layers": 2},
                                                    synthesis_kwargs=syn(32768, 0, None)), "32^2, 512 channels, fp32")
    if "g256" in parts:
        network_part("g256", a, dev, say, 32, dict(z_dim=512, c_dim=0, w_dim=512, img_resolution=256, img_channels=3, mapping_kwargs={"num_layers": 8},
                                                   synthesis_kwargs=syn(16384, 4, 256)), "256^2, bf16 blocks from 32^2 up, conv_clamp 256")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
