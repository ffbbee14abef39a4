"""StyleGAN2 discriminator: what the fused head of a down layer (csrc/style_fir.hip sg_act_fir_nhwc) and the minibatch-std kernel (csrc/mbstd.hip) are worth.
    python tools/stylegan2_dis_bench.py [--batch 32] [--rounds 3] [--iters 5] [--window-ms 200] [--parts head,layer,mbstd,cifar,d256] [--out profiles/stylegan2_dis_bench.txt]
Every contender of a part in one process, taking turns inside every round:
  head    conv1's head on a raw conv0 output (bias, lrelu, gain sqrt 2, clamp 256, 4x4 low-pass pad 2) at the widths of a 256^2 discriminator, batch --batch, fp32
          and bf16: `fused` = ONE sg_act_fir_nhwc launch, `chain` = sg_bias_act, NHWC->NCHW, sg_upfirdn2d, NCHW->NHWC (the copies are what the stride-2
          convolution behind it needs). Bytes the algorithm needs: read x once, write y once; share = of the measured HBM copy ceiling (--hbm-tbs, 6.3 TB/s).
  layer   the whole pair conv0 -> conv1 (down 2) of a block, forward and forward + backward (dx and all parameter gradients), fused against layer by layer,
          and the fused pair with every convolution pinned to sg_modconv2d_fwd (`modconv`: conv2d_resample.FORCE) against the dispatch. Under every row,
          the entry each convolution launch of the fused forward + backward took, as conv2d_resample.record() collected it while it ran
  mbstd   style_ops.minibatch_std against the torch composition of the same lines at 64 x 512 x 4 x 4, groups 4 and 32, forward and forward + backward
  cifar   Discriminator forward and forward + backward at the CIFAR10 configuration: 32^2, `orig`, 512 channels, batch 64, fp32
  d256    the same at 256^2: `resnet`, channel_base 16384, batch 32, the four highest resolutions in bf16, conv_clamp 256
each network with fused_down on / off (`off` is the layer-by-layer evaluation), followed by the recorded entry of every convolution launch of one forward + backward. Timing as tools/stylegan2_bench.py: device events around a window of
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
from studiogan_amd.backbones.stylegan2_dis import DConv2dLayer, Discriminator  # noqa: E402
from studiogan_amd.style_ops import conv2d_resample as CR  # noqa: E402
from studiogan_amd.style_ops import upfirdn2d as U  # noqa: E402
from studiogan_amd.style_ops.act_fir import act_fir  # noqa: E402
from studiogan_amd.style_ops.bias_act import bias_act  # noqa: E402
from studiogan_amd.style_ops.minibatch_std import minibatch_std  # noqa: E402

SQRT2 = 2 ** 0.5
CL = torch.channels_last


def _dt(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def say_launches(say, log):
    """one line per convolution launch, in launch order: what conv2d_resample.record() saw"""
    for role, entry, dt, N, Hs, Ws, C, Cout, k, mode in log:
        say(f"     {role:>5s} {k}x{k} {mode:>5s} {dt} [{N}, {Hs}, {Ws}, {C}] -> {Cout:4d} ch : {entry}")


def head_part(a, dev, say):
    say(f"## conv1's head (bias, lrelu, sqrt 2, clamp 256, 4x4 low-pass pad 2), batch {a.batch}: ms per call; ratio = chain / fused (> 1: the fused head is faster)")
    say(f"{'shape':>10s} {'dtype':>5s} | {'fused':>8s} {'chain':>8s} {'ratio':>6s} | {'GB/s':>6s} {'of HBM':>6s}")
    f = U.setup_filter([1, 3, 3, 1], device=dev)
    for shape in a.shapes.split(","):
        C, H = (int(v) for v in shape.split("x"))
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device=dev).manual_seed(C * 1000 + H)
            x = torch.randn(a.batch, C, H, H, generator=g, device=dev).to(dtype).contiguous(memory_format=CL)
            bias = torch.randn(C, generator=g, device=dev)
            epi = dict(act="lrelu", gain=SQRT2, clamp=256)

            def fused():
                with torch.no_grad():
                    return act_fir(x, f, [2, 2, 2, 2], bias=bias, **epi)

            def chain():
                with torch.no_grad():
                    return U.upfirdn2d(bias_act(x, bias.to(dtype), **epi), f, padding=[2, 2, 2, 2]).contiguous(memory_format=CL)

            ref = chain().float()
            err = float((fused().float() - ref).abs().max() / ref.abs().max())
            assert err < (5e-2 if dtype == torch.bfloat16 else 1e-4), (shape, dtype, err)      # the two compute the same function, at the size that is timed
            m, n_it = contest({"fused": fused, "chain": chain}, a)
            nbytes = (x.numel() + a.batch * C * (H + 1) ** 2) * x.element_size()
            gbs = nbytes / m["fused"] / 1e6
            say(f"{shape:>10s} {_dt(dtype):>5s} | {m['fused']:8.3f} {m['chain']:8.3f} {m['chain'] / m['fused']:6.2f} | {gbs:6.0f} {gbs / (a.hbm_tbs * 1e3):6.2f}"
                f"   (fused vs chain: {err:.1e} of range; calls per window {'/'.join(str(v) for v in n_it.values())})")
            del x, ref
            torch.cuda.empty_cache()


def layer_part(a, dev, say):
    say(f"## conv0 -> conv1 (down 2) of a block, batch {a.batch}: ms per call; ratio = layer by layer / fused; modconv = fused with every convolution on sg_modconv2d_fwd")
    say(f"{'shape':>10s} {'dtype':>5s} | {'fused fwd':>9s} {'layer fwd':>9s} {'ratio':>6s} {'modconv':>8s} | {'fused f+b':>9s} {'layer f+b':>9s} {'ratio':>6s} {'modconv':>8s}")
    for shape in a.shapes.split(","):
        C, H = (int(v) for v in shape.split("x"))
        Co = min(2 * C, 512)
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device=dev).manual_seed(C * 1000 + H + 1)
            conv0 = DConv2dLayer(C, C, 3, activation="lrelu", conv_clamp=256).to(dev)
            conv1 = DConv2dLayer(C, Co, 3, activation="lrelu", down=2, conv_clamp=256).to(dev)
            x = torch.randn(a.batch, C, H, H, generator=g, device=dev).to(dtype).contiguous(memory_format=CL)
            gy = torch.randn(a.batch, Co, H // 2, H // 2, generator=g, device=dev).to(dtype).contiguous(memory_format=CL)
            params = list(conv0.parameters()) + list(conv1.parameters())

            def fused(x):
                return conv1.finish(conv1.raw(conv0.raw(x), head=conv0.epilogue()))

            def layerwise(x):
                return conv1(conv0(x), fused=False)

            def pinned(run):
                def go():
                    CR.FORCE = CR.ENTRIES[1]
                    try:
                        return run()
                    finally:
                        CR.FORCE = None
                return go

            def fwd(op):
                def run():
                    with torch.no_grad():
                        return op(x)
                return run

            def fb(op):
                def run():
                    xl = x.clone().requires_grad_(True)
                    return torch.autograd.grad(op(xl), [xl] + params, gy)
                return run

            ref = fwd(layerwise)().float()
            err = float((fwd(fused)().float() - ref).abs().max() / ref.abs().max())
            assert err < (5e-2 if dtype == torch.bfloat16 else 1e-4), (shape, dtype, err)
            m, n_it = contest({"fused fwd": fwd(fused), "layer fwd": fwd(layerwise), "modconv fwd": pinned(fwd(fused)), "fused f+b": fb(fused),
                               "layer f+b": fb(layerwise), "modconv f+b": pinned(fb(fused))}, a)
            say(f"{shape:>10s} {_dt(dtype):>5s} | {m['fused fwd']:9.3f} {m['layer fwd']:9.3f} {m['layer fwd'] / m['fused fwd']:6.2f} {m['modconv fwd']:8.3f} | "
                f"{m['fused f+b']:9.3f} {m['layer f+b']:9.3f} {m['layer f+b'] / m['fused f+b']:6.2f} {m['modconv f+b']:8.3f}"
                f"   (fused vs layer forward: {err:.1e} of range; calls per window {'/'.join(str(v) for v in n_it.values())})")
            with CR.record() as log:
                fb(fused)()
            say_launches(say, log)
            del x, gy, ref, conv0, conv1, params
            torch.cuda.empty_cache()


def mbstd_torch(x, group, nch=1):
    N, C, H, W = x.shape
    G = N if group is None else min(group, N)
    y = x.reshape(G, -1, nch, C // nch, H, W)
    y = y - y.mean(dim=0)
    y = (y.square().mean(dim=0) + 1e-8).sqrt().mean(dim=[2, 3, 4])
    return torch.cat([x, y.reshape(-1, nch, 1, 1).repeat(G, 1, H, W)], dim=1)


def mbstd_part(a, dev, say):
    say("## minibatch_std at 64 x 512 x 4 x 4, fp32: ms per call; ratio = torch composition / kernel")
    say(f"{'group':>6s} | {'kernel fwd':>10s} {'torch fwd':>10s} {'ratio':>6s} | {'kernel f+b':>10s} {'torch f+b':>10s} {'ratio':>6s}")
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(64, 512, 4, 4, generator=g, device=dev).contiguous(memory_format=CL)
    gy = torch.randn(64, 513, 4, 4, generator=g, device=dev).contiguous(memory_format=CL)
    for group in (4, 32):
        def fwd(op):
            def run():
                with torch.no_grad():
                    return op(x, group, 1)
            return run

        def fb(op):
            def run():
                xl = x.clone().requires_grad_(True)
                return torch.autograd.grad(op(xl, group, 1), xl, gy)
            return run

        ref = fwd(mbstd_torch)()
        assert float((fwd(minibatch_std)() - ref).abs().max() / ref.abs().max()) < 1e-5
        m, _ = contest({"k fwd": fwd(minibatch_std), "t fwd": fwd(mbstd_torch), "k f+b": fb(minibatch_std), "t f+b": fb(mbstd_torch)}, a)
        say(f"{group:>6d} | {m['k fwd']:10.4f} {m['t fwd']:10.4f} {m['t fwd'] / m['k fwd']:6.2f} | {m['k f+b']:10.4f} {m['t f+b']:10.4f} {m['t f+b'] / m['k f+b']:6.2f}")


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

    def fwd(fused):
        def run():
            setup(fused)
            with torch.no_grad():
                return Dn(img, label)["adv_output"]
        return run

    def fb(fused):
        def run():
            setup(fused)
            il = img.clone().requires_grad_(True)
            return torch.autograd.grad(Dn(il, label)["adv_output"].sum(), [il] + params, allow_unused=True)
        return run

    ref = fwd(False)().float()
    err = float((fwd(True)().float() - ref).abs().max() / ref.abs().max())
    m, n_it = contest({"on fwd": fwd(True), "off fwd": fwd(False), "on f+b": fb(True), "off f+b": fb(False)}, a)
    say(f"## {name}: Discriminator, batch {batch}, {note}: ms per call; ratio = fused_down off / on")
    say(f"{'fused_down':>10s} | {'forward':>8s} {'ratio':>6s} | {'fwd+bwd':>8s} {'ratio':>6s} | calls per window")
    for k in ("on", "off"):
        say(f"{k:>10s} | {m[k + ' fwd']:8.3f} {m['off fwd'] / m[k + ' fwd']:6.2f} | {m[k + ' f+b']:8.3f} {m['off f+b'] / m[k + ' f+b']:6.2f} | {n_it[k + ' fwd']}/{n_it[k + ' f+b']}")
    say(f"   (adv_output on vs off: {err:.1e} of range)")
    say("   convolution launches of one forward + backward, fused_down on:")
    with CR.record() as log:
        fb(True)()
    say_launches(say, log)
    del Dn, params
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--parts", default="head,layer,mbstd,cifar,d256")
    ap.add_argument("--shapes", default="128x256,256x128,512x64,512x32")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="the HBM copy ceiling the head's bytes/s are held against")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stylegan2_dis_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/stylegan2_dis_bench.py --batch {a.batch} --rounds {a.rounds} --iters {a.iters} --window-ms {a.window_ms:g} --parts {a.parts}    ({torch.cuda.get_device_name(0)})")
    say("# median over rounds of event-timed windows; the contenders of a part alternate inside a round")
    parts = a.parts.split(",")
    if "head" in parts:
        head_part(a, dev, say)
    if "layer" in parts:
        layer_part(a, dev, say)
    if "mbstd" in parts:
        mbstd_part(a, dev, say)
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
