"""StyleGAN3: what the one-launch backward of the filtered leaky ReLU (csrc/style.hip sg_filtered_lrelu_gate / sg_filtered_lrelu_bwd) is worth.
    python tools/stylegan3_bench.py [--rounds 3] [--iters 5] [--window-ms 200] [--parts op,net] [--out profiles/stylegan3_bench.txt]
Two parts, every contender of a part in one process, taking turns inside every round:
  op    style_ops.filtered_lrelu at every distinct layer geometry of the StyleGAN3-T synthesis network at 32^2 (the CIFAR10 configuration, batch 32) and at
        256^2 (batch 8), fp32 and bf16: the backward alone (dx, db from a kept forward) and forward + backward. `fused` = the gate-writing forward and ONE
        sg_filtered_lrelu_bwd; `chain` = filtered_lrelu._FUSED_BWD[0] = False: the plain forward, then the four-launch operator chain re-run under autograd and
        differentiated, the route every backward took before the fused kernel existed.
  net   Generator forward and forward + backward (every parameter gradient and dz) at the same two configurations (fp32 at 32^2; the four highest resolutions
        in bf16 with conv_clamp 256 at 256^2), `fused` against `chain`; and the share of the fused step spent in the layout copies between the channels-last
        convolution and the plane-wise (NCHW) filtered leaky ReLU: per layer the four copies of a step (convolution input and output forward, the two
        gradients backward) and the zero padding of the full convolution, timed in isolation on tensors of the layer's shapes, summed over the layers.
Timing as tools/stylegan2_bench.py: device events around a window of back-to-back calls after 3 warm-up calls, a window of at least --iters calls and
--window-ms of work, --rounds rounds in alternating order, the median reported. There is no fallback: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import studiogan_amd  # noqa: E402,F401
from studiogan_amd.backbones.stylegan3 import Generator  # noqa: E402
from studiogan_amd.style_ops import filtered_lrelu as FL  # noqa: E402

CONFIGS = {     # name: (img_resolution, batch, c_dim, num_fp16_res, conv_clamp)
    "t32": (32, 32, 10, 0, None),
    "t256": (256, 8, 0, 4, 256),
}


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
    return {k: statistics.median(v) for k, v in t.items()}


def generator(name, dev):
    res, batch, c_dim, nfp16, clamp = CONFIGS[name]
    model = types.SimpleNamespace(info_type="N/A")
    G = Generator(z_dim=512, c_dim=c_dim, w_dim=512, img_resolution=res, img_channels=3, MODEL=model, mapping_kwargs={"num_layers": 2},
                  synthesis_kwargs={"channel_base": 32768, "channel_max": 512, "num_fp16_res": nfp16, "conv_clamp": clamp}).to(dev)
    return G, batch


def with_route(fused, fn):
    def run():
        FL._FUSED_BWD[0] = fused
        try:
            return fn()
        finally:
            FL._FUSED_BWD[0] = True
    return run


def with_cap(cap, fn):
    """the fused backward with another cap on its dx tile edge (csrc/style.hip sg_filtered_lrelu_bwd_tile)"""
    from studiogan_amd import _lib as L

    def run():
        old = L.lib().sg_filtered_lrelu_bwd_tile(cap)
        try:
            return fn()
        finally:
            L.lib().sg_filtered_lrelu_bwd_tile(old)
    return run


def op_part(a, dev, say):
    say("## filtered_lrelu per layer geometry: ms per call; ratio = chain / fused (> 1: the one-launch backward is faster)")
    say("## bwd t12 / t8: the fused backward with its dx tile edge capped at 12 / 8 instead of 16 (smaller tiles: more workgroups per CU, more halo)")
    say(f"{'net':5s} {'layer x [N, C, H, W]':26s} {'up/taps':8s} {'dn/taps':8s} {'dtype':5s} {'bwd fused':>10s} {'bwd chain':>10s} {'ratio':>6s} "
        f"{'f+b fused':>10s} {'f+b chain':>10s} {'ratio':>6s} {'bwd t12':>9s} {'bwd t8':>9s}")
    for name in CONFIGS:
        G, batch = generator(name, dev)
        seen = set()
        for lname in G.synthesis.layer_names:
            m = getattr(G.synthesis, lname)
            side = int(m.in_size[0]) + m.conv_kernel - 1
            key = (m.out_channels, side, m.up_factor, m.down_factor, m.up_taps, m.down_taps, tuple(m.padding))
            if key in seen or m.is_torgb:
                continue
            seen.add(key)
            for dtype in (torch.float32, torch.bfloat16):
                x = torch.randn(batch, m.out_channels, side, side, device=dev).to(dtype).requires_grad_(True)
                b = torch.randn(m.out_channels, device=dev).to(dtype).requires_grad_(True)
                kw = dict(fu=m.up_filter, fd=m.down_filter, b=b, up=m.up_factor, down=m.down_factor, padding=m.padding, gain=2 ** 0.5, slope=0.2, clamp=256.0)
                fns = {}
                for route, fused in (("fused", True), ("chain", False)):
                    y = with_route(fused, lambda: FL.filtered_lrelu(x, **kw))()
                    gy = torch.randn_like(y)
                    fns["bwd " + route] = with_route(fused, lambda y=y, gy=gy: torch.autograd.grad(y, [x, b], gy, retain_graph=True))
                    fns["f+b " + route] = with_route(fused, lambda gy=gy: torch.autograd.grad(FL.filtered_lrelu(x, **kw), [x, b], gy))
                    if fused:
                        fns["bwd t12"], fns["bwd t8"] = with_cap(12, fns["bwd fused"]), with_cap(8, fns["bwd fused"])
                t = contest(fns, a)
                say(f"{name:5s} {str([batch, m.out_channels, side, side]):26s} {m.up_factor}/{m.up_taps:<6d} {m.down_factor}/{m.down_taps:<6d} "
                    f"{'fp32' if dtype == torch.float32 else 'bf16':5s} {t['bwd fused']:10.4f} {t['bwd chain']:10.4f} {t['bwd chain'] / t['bwd fused']:6.2f} "
                    f"{t['f+b fused']:10.4f} {t['f+b chain']:10.4f} {t['f+b chain'] / t['f+b fused']:6.2f} {t['bwd t12']:9.4f} {t['bwd t8']:9.4f}")
        del G


def copy_ms(G, batch, dev, a):
    """the layout copies and the zero padding of one forward + backward, layer by layer, in isolation"""
    total = 0.0
    for lname in G.synthesis.layer_names:
        m = getattr(G.synthesis, lname)
        dtype = torch.bfloat16 if m.use_fp16 else torch.float32
        hi, k = int(m.in_size[0]), m.conv_kernel
        xin = torch.randn(batch, m.in_channels, hi, hi, device=dev).to(dtype)                                   # NCHW, from the previous layer
        xpad = torch.nn.functional.pad(xin, [k // 2] * 4)
        yout = torch.randn(batch, hi + k - 1, hi + k - 1, m.out_channels, device=dev).to(dtype).permute(0, 3, 1, 2)      # channels-last, from the convolution
        gy = yout.contiguous()                                                                                  # NCHW, from the filtered leaky ReLU's backward
        gin = torch.randn(batch, hi + 2 * (k // 2), hi + 2 * (k // 2), m.in_channels, device=dev).to(dtype).permute(0, 3, 1, 2)
        fns = {"pad": lambda: torch.nn.functional.pad(xin, [k // 2] * 4) if k > 1 else None,
               "x to nhwc": lambda: xpad.permute(0, 2, 3, 1).contiguous(),
               "y to nchw": lambda: yout.contiguous(),
               "gy to nhwc": lambda: gy.permute(0, 2, 3, 1).contiguous(),
               "gx to nchw": lambda: gin.contiguous()}
        t = contest(fns, a)
        total += sum(t.values())
    return total


def net_part(a, dev, say):
    say("## Generator: ms per call; ratio = chain / fused; copies = NCHW <-> channels-last copies and zero padding of one fused forward + backward, timed in isolation")
    say(f"{'net':5s} {'batch':>5s} {'fwd':>9s} {'f+b fused':>10s} {'f+b chain':>10s} {'ratio':>6s} {'copies':>9s} {'share of fused f+b':>19s}")
    for name in CONFIGS:
        G, batch = generator(name, dev)
        z = torch.randn(batch, 512, device=dev, requires_grad=True)
        c = torch.eye(max(G.c_dim, 1), device=dev)[torch.arange(batch) % max(G.c_dim, 1)][:, :G.c_dim]
        params = [z] + list(G.parameters())
        gy = torch.randn(batch, 3, G.img_resolution, G.img_resolution, device=dev)

        def fwd():
            with torch.no_grad():
                return G(z, c)

        def step():
            return torch.autograd.grad(G(z, c), params, gy, allow_unused=True)
        t = contest({"fwd": fwd, "fused": with_route(True, step), "chain": with_route(False, step)}, a)
        cp = copy_ms(G, batch, dev, a)
        say(f"{name:5s} {batch:5d} {t['fwd']:9.3f} {t['fused']:10.3f} {t['chain']:10.3f} {t['chain'] / t['fused']:6.2f} {cp:9.3f} {cp / t['fused']:18.1%}")
        del G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--parts", default="op,net")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stylegan3_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stylegan3_bench: needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/stylegan3_bench.py on {torch.cuda.get_device_name(0)}: rounds {a.rounds}, window {a.window_ms} ms")
    torch.manual_seed(0)
    for part in a.parts.split(","):
        {"op": op_part, "net": net_part}[part](a, dev, say)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
