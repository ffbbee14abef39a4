"""R1 through the StyleGAN2 discriminator: what the fused second-order head (csrc/style_fir.hip sg_act_fir_nhwc_gate) is worth, and what a lazy-R1 step costs.
    python tools/stylegan2_r1_bench.py [--batch 32] [--rounds 3] [--iters 5] [--window-ms 200] [--parts gate,cifar,d256] [--out profiles/stylegan2_r1_bench.txt]
Every contender of a part in one process, taking turns inside every round:
  gate    the second-order pass of conv1's head (bias, lrelu, gain sqrt 2, clamp 256, 4x4 low-pass pad 2) at the widths of a 256^2 discriminator, batch --batch,
          fp32 and bf16: `gate` = ONE sg_act_fir_nhwc_gate launch on the cotangent v and the kept raw x; `chain` = the operators it replaces, sg_bias_act's
          gradient launch (v * da/dx from the kept activation), NHWC->NCHW, sg_upfirdn2d, NCHW->NHWC; `fwd` = the forward launch sg_act_fir_nhwc on the same x,
          for the expectation that the gate costs what the forward costs plus one more read. Bytes the algorithm needs: read v and x once, write y once; share =
          of the measured HBM copy ceiling (--hbm-tbs, 6.3 TB/s).
  cifar   Discriminator at the CIFAR10 configuration (32^2, `orig`, 512 channels, batch 64, fp32): one lazy-R1 step (forward with a gradient on the images,
          losses.stylegan_cal_r1_reg, backward into every parameter) against a plain forward + backward (the image gradient and every parameter gradient of
          sum(adv_output)), with fused_down on and off
  d256    the same at 256^2: `resnet`, channel_base 16384, batch 32, the four highest resolutions in bf16, conv_clamp 256
followed by the recorded role and entry of every convolution launch of one R1 step. Timing as tools/stylegan2_bench.py: device events around a window of
back-to-back calls after 3 warm-up calls, a window of at least --iters calls and --window-ms of work, --rounds rounds in alternating order, the median
reported. There is no fallback: without a GPU the tool fails."""
import argparse
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import studiogan_amd  # noqa: E402,F401
from stylegan2_bench import contest  # noqa: E402
from stylegan2_dis_bench import say_launches  # noqa: E402
from studiogan_amd import losses  # noqa: E402
from studiogan_amd.backbones.stylegan2_dis import Discriminator  # noqa: E402
from studiogan_amd.style_ops import conv2d_resample as CR  # noqa: E402
from studiogan_amd.style_ops import upfirdn2d as U  # noqa: E402
from studiogan_amd.style_ops.act_fir import act_fir, act_fir_nhwc_gate_raw  # noqa: E402
from studiogan_amd.style_ops.bias_act import bias_act  # noqa: E402

SQRT2 = 2 ** 0.5
CL = torch.channels_last


def _dt(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def gate_part(a, dev, say):
    say(f"## second-order pass of conv1's head (bias, lrelu, sqrt 2, clamp 256, 4x4 low-pass pad 2), batch {a.batch}: ms per call; ratio = chain / gate "
        "(> 1: the gate launch is faster); fwd = sg_act_fir_nhwc on the same x")
    say(f"{'shape':>10s} {'dtype':>5s} | {'gate':>8s} {'chain':>8s} {'ratio':>6s} | {'fwd':>8s} {'gate/fwd':>8s} | {'GB/s':>6s} {'of HBM':>6s}")
    f = U.setup_filter([1, 3, 3, 1], device=dev)
    f2d = torch.outer(f, f).contiguous() if f.dim() == 1 else f
    for shape in a.shapes.split(","):
        C, H = (int(v) for v in shape.split("x"))
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device=dev).manual_seed(C * 1000 + H)
            x = torch.randn(a.batch, C, H, H, generator=g, device=dev).to(dtype).contiguous(memory_format=CL)
            v = torch.randn(a.batch, C, H, H, generator=g, device=dev).to(dtype).contiguous(memory_format=CL)
            bias = torch.randn(C, generator=g, device=dev).bfloat16().float()       # (held by bf16: the chain rounds its bias to x's dtype, and a gate is a
            epi = dict(act="lrelu", gain=SQRT2, clamp=256)                          # jump, so a pre-activation moved across 0 is an O(1) difference)
            xh, vh = x.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1)
            assert xh.is_contiguous() and vh.is_contiguous()
            xg = x.detach().requires_grad_(True)
            act = bias_act(xg, bias.to(dtype), **epi)       # the chain keeps the activated map, as the layer-by-layer network does

            def gate():
                return act_fir_nhwc_gate_raw(vh, xh, f2d, (2, 2, 2, 2), 1, False, 1.0, bias, "lrelu", 0.2, SQRT2, 256.0)

            def chain():
                (gv,) = torch.autograd.grad(act, xg, v, retain_graph=True)          # sg_bias_act, gradient mode
                with torch.no_grad():
                    return U.upfirdn2d(gv.contiguous(), f, padding=[2, 2, 2, 2]).contiguous(memory_format=CL)

            def fwd():
                with torch.no_grad():
                    return act_fir(x, f, [2, 2, 2, 2], bias=bias, **epi)

            ref = chain().float()
            err = float((gate().permute(0, 3, 1, 2).float() - ref).abs().max() / ref.abs().max())
            assert err < (5e-2 if dtype == torch.bfloat16 else 1e-4), (shape, dtype, err)      # the two compute the same function, at the size that is timed
            m, n_it = contest({"gate": gate, "chain": chain, "fwd": fwd}, a)
            nbytes = (2 * x.numel() + a.batch * C * (H + 1) ** 2) * x.element_size()
            gbs = nbytes / m["gate"] / 1e6
            say(f"{shape:>10s} {_dt(dtype):>5s} | {m['gate']:8.3f} {m['chain']:8.3f} {m['chain'] / m['gate']:6.2f} | {m['fwd']:8.3f} {m['gate'] / m['fwd']:8.2f} | "
                f"{gbs:6.0f} {gbs / (a.hbm_tbs * 1e3):6.2f}   (gate vs chain: {err:.1e} of range; calls per window {'/'.join(str(n) for n in n_it.values())})")
            del x, v, xg, act, ref
            torch.cuda.empty_cache()


def network_part(name, a, dev, say, batch, kwargs, note):
    model = types.SimpleNamespace(info_type="N/A")
    Dn = Discriminator(c_dim=0, img_channels=3, d_cond_mtd="W/O", aux_cls_type="W/O", num_classes=10, normalize_d_embed=False, MODEL=model, **kwargs).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    img = torch.randn(batch, 3, Dn.img_resolution, Dn.img_resolution, generator=g, device=dev)
    label = torch.arange(batch, device=dev) % 10
    params = list(Dn.parameters())
    blocks = [getattr(Dn, f"b{r}") for r in Dn.block_resolutions]

    def setup(fused):
        for b in blocks:
            b.fused_down = fused

    def fb(fused):
        def run():
            setup(fused)
            il = img.clone().requires_grad_(True)
            return torch.autograd.grad(Dn(il, label)["adv_output"].sum(), [il] + params, allow_unused=True)
        return run

    def r1(fused):
        def run():
            setup(fused)
            for p in params:
                p.grad = None
            return losses.stylegan_d_reg_step(Dn, img, label, 10.0, 16)
        return run

    pen = {k: float(r1(k)()) for k in (True, False)}
    err = abs(pen[True] - pen[False]) / max(abs(pen[False]), 1e-30)
    m, n_it = contest({"on f+b": fb(True), "off f+b": fb(False), "on r1": r1(True), "off r1": r1(False)}, a)
    say(f"## {name}: Discriminator, batch {batch}, {note}: ms per call; R1 / f+b = what a lazy-R1 step costs in plain forward + backward passes")
    say(f"{'fused_down':>10s} | {'fwd+bwd':>8s} | {'R1 step':>8s} {'R1 / f+b':>8s} {'off / on':>8s} | calls per window")
    for k in ("on", "off"):
        say(f"{k:>10s} | {m[k + ' f+b']:8.3f} | {m[k + ' r1']:8.3f} {m[k + ' r1'] / m[k + ' f+b']:8.2f} {m['off r1'] / m[k + ' r1']:8.2f} | {n_it[k + ' f+b']}/{n_it[k + ' r1']}")
    say(f"   (scaled penalty on vs off: {err:.1e} relative; value {pen[True]:.4e})")
    say("   convolution launches of one R1 step, fused_down on:")
    with CR.record() as log:
        r1(True)()
    say_launches(say, log)
    for p in params:
        p.grad = None
    del Dn, params
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--parts", default="gate,cifar,d256")
    ap.add_argument("--shapes", default="128x256,256x128,512x64,512x32")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="the HBM copy ceiling the gate's bytes/s are held against")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stylegan2_r1_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/stylegan2_r1_bench.py --batch {a.batch} --rounds {a.rounds} --iters {a.iters} --window-ms {a.window_ms:g} --parts {a.parts}    ({torch.cuda.get_device_name(0)})")
    say("# median over rounds of event-timed windows; the contenders of a part alternate inside a round")
    parts = a.parts.split(",")
    if "gate" in parts:
        gate_part(a, dev, say)
    if "cifar" in parts:
        network_part("cifar", a, dev, say, 64, dict(img_resolution=32, architecture="orig", channel_base=32768, channel_max=512,
                                                    epilogue_kwargs={"mbstd_group_size": 32}), "32^2, orig, 512 channels, fp32")
    if "d256" in parts:
        network_part("d256", a, dev, say, 32, dict(img_resolution=256, architecture="resnet", channel_base=16384, channel_max=512, num_fp16_res=4, conv_clamp=256,
                                                   epilogue_kwargs={"mbstd_group_size": 4}), "256^2, resnet, bf16 blocks from 32^2 up, conv_clamp 256")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
