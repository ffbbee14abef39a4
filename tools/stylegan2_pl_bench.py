"""Path-length regularisation through the StyleGAN2 generator: what the two new launches are worth, and what a lazy-PLR step costs.
    python tools/stylegan2_pl_bench.py [--batch 16] [--rounds 3] [--iters 5] [--window-ms 200] [--parts jvp,gate,cifar,g256] [--out profiles/stylegan2_pl_bench.txt]
Every contender of a part in one process, taking turns inside every round:
  jvp     the forward-mode tangent of the modulated convolution at the layer shapes of tools/modconv_bench.py (channels x map, 3 x 3, demodulation, per-sample
          noise; one up = 2 layer), batch --batch, fp32 and bf16: `jvp` = ONE sg_modconv2d_jvp launch; `comp` = the composition it replaces, an elementwise
          combine of the operand (vs x + s vx, torch), sg_modconv2d_fwd, and an axpy with the stored y (e (y - noise), torch); `fwd` = sg_modconv2d_fwd on the same
          x, for the expectation from bytes: the forward launch plus one more operand read and one read of y.
  gate    the second-order pass of the fused up = 2 layer tail (lrelu, gain sqrt 2, clamp 256, 4 x 4 low-pass pad 1, gain 4) on the [2H + 1]^2 core: `gate` = ONE
          sg_fir_bias_act_nhwc_gate launch on the cotangent and the kept y; `chain` = the plain FIR launch and sg_bias_act in gradient mode on (FIR(v), y);
          `fwd` = the forward launch sg_fir_bias_act_nhwc. Bytes the algorithm needs: read v and y once, write once; share of the HBM copy ceiling (--hbm-tbs).
  cifar   Generator at the CIFAR10 configuration (32^2, 512 channels, fp32), batch 32 = half of 64: one lazy-PLR step (losses.stylegan_g_reg_step: mapping,
          synthesis, the latents' gradient with a graph, the loss's backward into every parameter) against a plain forward + backward (every parameter gradient
          of <img, gy>) at the same batch. A/B/B/A order inside a round.
  g256    the same at 256^2: channel_base 16384, batch 16, bf16 blocks from 32^2 up, conv_clamp 256
Timing as tools/stylegan2_bench.py: device events around a window of back-to-back calls after 3 warm-up calls, a window of at least --iters calls and
--window-ms of work, --rounds rounds, the median reported. There is no fallback: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import studiogan_amd  # noqa: E402,F401
from stylegan2_bench import contest, timed  # noqa: E402
from studiogan_amd import _lib as L  # noqa: E402
from studiogan_amd import losses  # noqa: E402
from studiogan_amd.backbones.stylegan2 import Generator  # noqa: E402
from studiogan_amd.style_ops import upfirdn2d as U  # noqa: E402
from studiogan_amd.style_ops.bias_act import activation_funcs  # noqa: E402
from studiogan_amd.style_ops.fir_bias_act import fir_gate_raw, fir_nhwc_raw  # noqa: E402
from studiogan_amd.style_ops.modulated_conv2d import _jvp_raw, _modconv_raw  # noqa: E402

SQRT2 = 2 ** 0.5


def _dt(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def jvp_part(a, dev, say):
    say(f"## forward-mode tangent of the modulated convolution, batch {a.batch}: ms per call; ratio = comp / jvp (> 1: the one launch is faster); fwd = "
        "sg_modconv2d_fwd on the same x; bytes = jvp's over fwd's from the shapes (one more operand read, one read of y)")
    say(f"{'shape':>10s} {'dtype':>5s} | {'jvp':>8s} {'comp':>8s} {'ratio':>6s} | {'fwd':>8s} {'jvp/fwd':>8s} {'bytes':>6s} |")
    for shape in a.shapes.split(","):
        up = 2 if shape.endswith("up") else 1
        C, H = (int(v) for v in shape.replace("up", "").split("x"))
        N, Ho = a.batch, (2 * H + 1 if up == 2 else H)
        mode = "same" if up == 1 else "up2"
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device=dev).manual_seed(C * 1000 + H)
            r = lambda *s: torch.randn(*s, generator=g, device=dev)      # noqa: E731
            x, vx = r(N, H, H, C).to(dtype), r(N, H, H, C).to(dtype)
            w = r(C, C, 3, 3) / (3 * C ** 0.5)
            wimg = w.permute(0, 2, 3, 1).contiguous().to(dtype)
            s, vs = 1 + r(N, C), r(N, C)
            Q = w.square().sum(dim=(2, 3))
            d = (s.square() @ Q.t() + 1e-8).rsqrt()
            e = -(d * d) * ((s * vs) @ Q.t())
            nz = r(N, 1, H, H) if up == 1 else None
            ns = H * H if up == 1 else 0
            y = _modconv_raw(x, wimg, C, 3, mode, pre=s, post=d, noise=nz, noise_stride=ns)

            def jvp():
                return _jvp_raw(x, vx, wimg, C, 3, mode, s, vs, d, y, e, nz, ns)

            def comp():
                m = x * vs.to(dtype)[:, None, None, :] + vx * s.to(dtype)[:, None, None, :]
                t = _modconv_raw(m, wimg, C, 3, mode, post=d)
                u = y if nz is None else y - nz.reshape(N, H, H, 1).to(dtype)
                return t + e.to(dtype)[:, None, None, :] * u

            def fwd():
                return _modconv_raw(x, wimg, C, 3, mode, pre=s, post=d, noise=nz, noise_stride=ns)

            ref = comp().float()
            err = float((jvp().float() - ref).abs().max() / ref.abs().max())
            assert err < (5e-2 if dtype == torch.bfloat16 else 1e-4), (shape, dtype, err)      # the two compute the same function, at the size that is timed
            m, n_it = contest({"jvp": jvp, "comp": comp, "fwd": fwd}, a)
            b_fwd = x.numel() + wimg.numel() + y.numel()
            b_jvp = 2 * x.numel() + wimg.numel() + 2 * y.numel()
            say(f"{shape:>10s} {_dt(dtype):>5s} | {m['jvp']:8.3f} {m['comp']:8.3f} {m['comp'] / m['jvp']:6.2f} | {m['fwd']:8.3f} {m['jvp'] / m['fwd']:8.2f} "
                f"{b_jvp / b_fwd:6.2f} |   (jvp vs comp: {err:.1e} of range; calls per window {'/'.join(str(n) for n in n_it.values())})")
            del x, vx, y, ref
            torch.cuda.empty_cache()


def gate_part(a, dev, say):
    say(f"## second-order pass of the up = 2 layer tail (lrelu, sqrt 2, clamp 256, 4x4 low-pass pad 1, gain 4), batch {a.batch}: ms per call; ratio = chain / gate "
        "(> 1: the gate launch is faster); fwd = sg_fir_bias_act_nhwc on a core of the same shape")
    say(f"{'shape':>10s} {'dtype':>5s} | {'gate':>8s} {'chain':>8s} {'ratio':>6s} | {'fwd':>8s} {'gate/fwd':>8s} | {'GB/s':>6s} {'of HBM':>6s}")
    f = U.setup_filter([1, 3, 3, 1], device=dev)
    f2d = (torch.outer(f, f) if f.dim() == 1 else f).contiguous()
    pad, epi = (1, 1, 1, 1), ("lrelu", 0.2, SQRT2, 256.0)
    for shape in a.tail_shapes.split(","):
        C, H = (int(v) for v in shape.split("x"))
        N, Hc, Ho = a.batch, 2 * H + 1, 2 * H
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device=dev).manual_seed(C * 1000 + H)
            core = torch.randn(N, Hc, Hc, C, generator=g, device=dev).to(dtype)
            v = torch.randn(N, Hc, Hc, C, generator=g, device=dev).to(dtype)
            nz, bias = torch.randn(N, 1, Ho, Ho, generator=g, device=dev), torch.randn(C, generator=g, device=dev)
            y = fir_nhwc_raw(core, f2d, pad, False, 4.0, nz, Ho * Ho, bias, *epi)

            def gate():
                return fir_gate_raw(v, y, f2d, pad, False, 4.0, None, 0, None, *epi)

            def chain():
                t = fir_nhwc_raw(v, f2d, pad, False, 4.0)
                out = torch.empty_like(t)
                L.call("sg_bias_act", L.dt(t), L.ptr(t), None, None, L.ptr(y), None, L.ptr(out), t.numel(), 1, 1, 1, activation_funcs["lrelu"].cuda_idx,
                       0.2, SQRT2, 256.0, L.stream())
                return out

            def fwd():
                return fir_nhwc_raw(core, f2d, pad, False, 4.0, nz, Ho * Ho, bias, *epi)

            ref = chain().float()
            err = float((gate().float() - ref).abs().max() / ref.abs().max())
            assert err < (5e-2 if dtype == torch.bfloat16 else 1e-4), (shape, dtype, err)
            m, n_it = contest({"gate": gate, "chain": chain, "fwd": fwd}, a)
            nbytes = (v.numel() + 2 * y.numel()) * v.element_size()
            gbs = nbytes / m["gate"] / 1e6
            say(f"{shape + 'up':>10s} {_dt(dtype):>5s} | {m['gate']:8.3f} {m['chain']:8.3f} {m['chain'] / m['gate']:6.2f} | {m['fwd']:8.3f} {m['gate'] / m['fwd']:8.2f} | "
                f"{gbs:6.0f} {gbs / (a.hbm_tbs * 1e3):6.2f}   (gate vs chain: {err:.1e} of range; calls per window {'/'.join(str(n) for n in n_it.values())})")
            del core, v, y, ref
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
    labels = torch.arange(batch, device=dev) % max(G.c_dim, 1)
    c = torch.nn.functional.one_hot(labels, G.c_dim) if G.c_dim else None
    params = list(G.parameters())
    gy = torch.randn(batch, 3, G.img_resolution, G.img_resolution, generator=g, device=dev)
    reg = losses.PathLengthRegularizer(dev, pl_weight=2, pl_no_weight_grad=True)

    def fb():
        return torch.autograd.grad(G(z, c, noise_mode="random"), params, gy, allow_unused=True)

    def plr():
        for p in params:
            p.grad = None
        return losses.stylegan_g_reg_step(G, z, labels, reg, 4)

    value = float(plr())
    assert value == value and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    # step-level A/B in ABBA order: the two windows of each contender inside a round sit symmetrically around the round's middle
    for fn in (fb, plr):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    n_it = {k: max(a.iters, min(5000, int(a.window_ms / max(timed(fn, a.iters), 1e-3)) + 1)) for k, fn in (("f+b", fb), ("plr", plr))}
    t = {"f+b": [], "plr": []}
    for _ in range(a.rounds):
        for k, fn in (("f+b", fb), ("plr", plr), ("plr", plr), ("f+b", fb)):
            t[k].append(timed(fn, n_it[k]))
    m = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / m[k] for k, v in t.items()}
    say(f"## {name}: Generator, batch {batch}, {note}: ms per call, ABBA windows; PLR / f+b = what a lazy-PLR step costs in plain forward + backward passes")
    say(f"{'fwd+bwd':>8s} {'spread':>7s} | {'PLR step':>8s} {'spread':>7s} | {'PLR / f+b':>9s} | calls per window")
    say(f"{m['f+b']:8.3f} {spread['f+b']:7.1%} | {m['plr']:8.3f} {spread['plr']:7.1%} | {m['plr'] / m['f+b']:9.2f} | {n_it['f+b']}/{n_it['plr']}   (scaled loss {value:.4e})")
    for p in params:
        p.grad = None
    del G, params
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--parts", default="jvp,gate,cifar,g256")
    ap.add_argument("--shapes", default="512x16,512x32,512x64,256x128,128x256,512x16up")
    ap.add_argument("--tail-shapes", default="512x16,512x32,256x64,128x128")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="the HBM copy ceiling the gate's bytes/s are held against")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stylegan2_pl_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/stylegan2_pl_bench.py --batch {a.batch} --rounds {a.rounds} --iters {a.iters} --window-ms {a.window_ms:g} --parts {a.parts}    ({torch.cuda.get_device_name(0)})")
    say("# median over rounds of event-timed windows; the contenders of a part alternate inside a round")
    parts = a.parts.split(",")
    if "jvp" in parts:
        jvp_part(a, dev, say)
    if "gate" in parts:
        gate_part(a, dev, say)
    syn = lambda base, res, clamp: {"channel_base": base, "channel_max": 512, "num_fp16_res": res, "conv_clamp": clamp}      # noqa: E731
    if "cifar" in parts:
        network_part("cifar", a, dev, say, 32, dict(z_dim=512, c_dim=10, w_dim=512, img_resolution=32, img_channels=3, mapping_kwargs={"num_layers": 2},
                                                    synthesis_kwargs=syn(32768, 0, None)), "32^2, 512 channels, fp32")
    if "g256" in parts:
        network_part("g256", a, dev, say, 16, dict(z_dim=512, c_dim=0, w_dim=512, img_resolution=256, img_channels=3, mapping_kwargs={"num_layers": 8},
                                                   synthesis_kwargs=syn(16384, 4, 256)), "256^2, bf16 blocks from 32^2 up, conv_clamp 256")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
