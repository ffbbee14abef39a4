"""StyleGAN2 modulated convolution: the fused operator (style_ops.modulated_conv2d, csrc/modconv.hip) against the route a user could assemble before it.
    python tools/modconv_bench.py [--batch 32] [--rounds 3] [--iters 5] [--window-ms 200] [--shapes 512x16,512x32,...] [--out profiles/modconv_bench.txt]
Shapes are the 3 x 3 layers of a StyleGAN2-256 synthesis network at batch 32 (channels x map, up = 1) and one up = 2 layer (512 -> 512, 16^2 -> 32^2), each in
bf16 and fp32, per-sample noise, demodulation on. Contenders, all in one process:
  fused    modulated_conv2d as a user calls it: per call it packs the weight image (flip, permute, cast), runs the two small kernels of Q and d, then the
           one sg_modconv2d_fwd launch; forward, and forward + backward (dx, dweight, dstyles, dnoise)
  kernel   the sg_modconv2d_fwd launch alone, on a weight image packed and a d computed beforehand (+ FIR and noise at up = 2): what 3-pass is given
  3-pass   what could be assembled before: broadcast multiply (torch), sg_conv2d_fwd through functional.conv2d_raw on the shared weight image, broadcast
           multiply-add with d and the noise (torch); forward only (there was no backward to assemble); the packed weight image and d are given to it
           for free, so its fair opponent is `kernel`, while `fused` is what the operator costs end to end
The reference's own route (per-sample weights [N, Cout, Cin, 3, 3], a grouped convolution with groups = N through MIOpen) is NOT a contender here: its
backward faulted inside MIOpen's solver search on the MI355X at 512 x 32^2 bf16 (profiles/modconv_bench.txt keeps the two rows measured before that).
Timing: device events around a window of back-to-back calls, after 3 warm-up calls per contender and shape; a window holds at least --iters calls and at
least --window-ms of work (calibrated per contender after the warm-up: a 0.1 ms call is timed over 2000 calls); --rounds rounds, the contenders taking turns
inside every round (alternating order), the median over rounds reported. The up = 2 rows include the FIR (style_ops.upfirdn2d) on every route.
There is no fallback: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import studiogan_amd  # noqa: E402,F401
from studiogan_amd import _lib as L  # noqa: E402
from studiogan_amd.functional._base import conv2d_raw  # noqa: E402
from studiogan_amd.style_ops import upfirdn2d as U  # noqa: E402
from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d, _modconv_raw  # noqa: E402


def dcoef(w, s):
    return (s.float().square() @ w.float().square().sum(dim=(2, 3)).t() + 1e-8).rsqrt()


def three_pass(x_nhwc, wimg, s, d, noise_nhwc, up, f):
    """x * s -> sg_conv2d_fwd -> * d (+ FIR at up = 2) + noise on NHWC tensors of the activation dtype; returns NCHW (a channels_last view at up = 1)"""
    N, H, W, C = x_nhwc.shape
    Cout = wimg.shape[0]
    xs = x_nhwc * s.to(x_nhwc.dtype)[:, None, None, :]
    if up == 1:
        u = conv2d_raw(xs, L.ptr(wimg), C, Cout, 3, 3, 1, 1, 1)
        return (u * d.to(u.dtype)[:, None, None, :] + noise_nhwc).permute(0, 3, 1, 2)
    u = conv2d_raw(xs, L.ptr(wimg), C, Cout, 3, 3, 2, 0, 0, pix_flags=L.PIX_TRANSPOSED, transposed_out_hw=(2 * H + 1, 2 * W + 1))
    u = u * d.to(u.dtype)[:, None, None, :]
    y = U.upfirdn2d(u.permute(0, 3, 1, 2), f, padding=[1, 1, 1, 1], gain=4)
    return y + noise_nhwc.permute(0, 3, 1, 2)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--shapes", default="512x16,512x32,512x64,256x128,128x256,512x16up")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "modconv_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/modconv_bench.py --batch {a.batch} --rounds {a.rounds} --iters {a.iters} --window-ms {a.window_ms:g}    ({torch.cuda.get_device_name(0)})")
    say("# ms per call, median over rounds of event-timed windows; contenders alternate inside a round. ratios = 3-pass / other (> 1: the other is faster)")
    say(f"{'shape':>14s} {'dtype':>5s} | {'fused fwd':>9s} {'kernel fwd':>10s} {'3-pass fwd':>10s} | {'3p/fused':>8s} {'3p/kernel':>9s} | {'fused f+b':>9s} | {'kernel TFLOP/s':>14s}")
    f = U.setup_filter([1, 3, 3, 1], device=dev)
    for shape in a.shapes.split(","):
        up = 2 if shape.endswith("up") else 1
        C, H = (int(v) for v in shape.replace("up", "").split("x"))
        N, Cout, Ho = a.batch, C, H * up
        for dtype in (torch.bfloat16, torch.float32):
            g = torch.Generator(device=dev).manual_seed(C * 1000 + H)
            x = torch.randn(N, C, H, H, generator=g, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
            w = torch.randn(Cout, C, 3, 3, generator=g, device=dev)
            s = 1 + torch.randn(N, C, generator=g, device=dev)
            noise = torch.randn(N, 1, Ho, Ho, generator=g, device=dev)
            gy = torch.randn(N, Cout, Ho, Ho, generator=g, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
            x_nhwc, noise_nhwc = x.permute(0, 2, 3, 1), noise.permute(0, 2, 3, 1).to(dtype)
            wimg = w.permute(0, 2, 3, 1).contiguous().to(dtype)          # up = 1: correlation; up = 2: flip_weight=False scatters the taps as given
            d = dcoef(w, s)
            leaves = [t.clone().requires_grad_(True) for t in (x, w, s, noise)]
            kw = dict(up=up, padding=1, resample_filter=f, flip_weight=(up == 1))

            def fused_fwd():
                with torch.no_grad():
                    return modulated_conv2d(x, w, s, noise=noise, **kw)

            def fused_fb():
                y = modulated_conv2d(leaves[0], leaves[1], leaves[2], noise=leaves[3], **kw)
                return torch.autograd.grad(y, leaves, gy)

            s32, nz = s.contiguous(), noise.contiguous()

            def kernel_fwd():
                with torch.no_grad():
                    if up == 1:
                        return _modconv_raw(x_nhwc, wimg, Cout, 3, "same", pre=s32, post=d, noise=nz, noise_stride=Ho * Ho).permute(0, 3, 1, 2)
                    u = _modconv_raw(x_nhwc, wimg, Cout, 3, "up2", pre=s32, post=d)
                    return U.upfirdn2d(u.permute(0, 3, 1, 2), f, padding=[1, 1, 1, 1], gain=4) + noise.to(dtype)

            def three_fwd():
                with torch.no_grad():
                    return three_pass(x_nhwc, wimg, s, d, noise_nhwc, up, f)

            # the two forwards compute the same function: checked at the size that is timed
            ref = three_fwd().float()
            err = max(float((fn().float() - ref).abs().max() / ref.abs().max()) for fn in (fused_fwd, kernel_fwd))
            assert err < (5e-2 if dtype == torch.bfloat16 else 1e-3), (shape, dtype, err)
            fns = {"fused fwd": fused_fwd, "kernel fwd": kernel_fwd, "3-pass fwd": three_fwd, "fused f+b": fused_fb}
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
            m = {k: statistics.median(v) for k, v in t.items()}
            flops = 2.0 * N * Cout * C * 9 * (H * H if up == 2 else Ho * Ho)
            say(f"{shape:>14s} {'bf16' if dtype == torch.bfloat16 else 'fp32':>5s} | {m['fused fwd']:9.3f} {m['kernel fwd']:10.3f} {m['3-pass fwd']:10.3f} | "
                f"{m['3-pass fwd'] / m['fused fwd']:8.2f} {m['3-pass fwd'] / m['kernel fwd']:9.2f} | {m['fused f+b']:9.3f} | {flops / m['kernel fwd'] / 1e9:14.1f}"
                f"   (fused / kernel vs 3-pass forward: {err:.1e} of range; calls per window {n_it['fused fwd']}/{n_it['kernel fwd']}/{n_it['3-pass fwd']}/{n_it['fused f+b']})")
            del leaves, x, gy, ref
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
