"""Times the eight elementwise entry points that have a scalar and a 16-byte path (csrc/elementwise.hip) in bf16, with device events, at shapes the
128-pixel BigGAN and BigGAN-deep networks launch them with at batch 256.

    python tools/ew_bench.py --json new1.json
    SG_LIBSGAMD=<library built from the parent commit> python tools/ew_bench.py --json parent1.json
    python tools/ew_bench.py --compare --parent parent1.json parent2.json parent3.json --new new1.json new2.json new3.json

One process is one round; run the two builds alternating. --compare prints, per entry point (its shapes' times summed), the median of either build's rounds
and the parent's own spread across its rounds (max - min), and fails where the new median exceeds the parent's by more than that spread.

The shapes, from the call sites (functional/pointwise.py AvgPool2Fn / ReluMaskFn, functional/conv.py SliceUpFn / CatConvFn and the ReLU mask of a data gradient,
functional/attention.py) and the block structure of the networks (ch = 96 for BigGAN-128, 128 for BigGAN-deep-128; the kernel names are in
profiles/r06_bench_biggan128_bs256_kerneltrace_zz.txt and profiles/r06_kerneltrace_extra_bigdeep128_bs256_bf16_zz.txt):
  avg-pool         [N, H, W, C] of the unpooled side: the discriminator's 8-channel image skip, and the block inputs of BigGAN-deep's discriminator
  max-pool         [N, 64, 64, C]: phi (C / 8, padded to 16 in D) and g (C / 2) of the 64 x 64 attention block of G (C = 192) and D (C = 96)
  relu_mask        n: hidden activations of BigGAN-deep's bottleneck blocks and BigGAN's discriminator blocks
  slice_up         [N, Hs, Ws, ld] -> C channels, x2: the channel-slice skip of BigGAN-deep's generator blocks
  copy_channels    rows x C of pitch C into pitch 2 C: the channel-concat skip of BigGAN-deep's discriminator blocks
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

B = 256
SHAPES = {      # the first shape of every entry point is also tools/ew_fold_check.py's workload-sized call
    "sg_avgpool2_fwd": [(B, 64, 64, 256), (B, 128, 128, 8), (B, 128, 128, 128)],
    "sg_avgpool2_bwd": [(B, 64, 64, 256), (B, 128, 128, 8), (B, 128, 128, 128)],
    "sg_maxpool2_fwd": [(B, 64, 64, 24), (B, 64, 64, 96), (B, 64, 64, 16), (B, 64, 64, 48)],
    "sg_maxpool2_bwd": [(B, 64, 64, 24), (B, 64, 64, 96), (B, 64, 64, 16), (B, 64, 64, 48)],
    "sg_relu_mask": [(B * 32 * 32 * 384,), (B * 64 * 64 * 192,), (B * 128 * 128 * 32,)],
    "sg_slice_up_fwd": [(B, 32, 32, 512, 256, 2), (B, 16, 16, 1024, 512, 2), (B, 64, 64, 256, 128, 2)],
    "sg_slice_up_bwd": [(B, 32, 32, 512, 256, 2), (B, 16, 16, 1024, 512, 2), (B, 64, 64, 256, 128, 2)],
    "sg_copy_channels": [(B * 32 * 32, 256, 256, 512), (B * 64 * 64, 128, 128, 256), (B * 16 * 16, 512, 512, 1024)],
}


def timeit(fn, window_ms=100.0):
    """device events around enough calls to fill `window_ms` (at least 10) -> ms per call"""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        fn()
    b.record()
    torch.cuda.synchronize()
    iters = max(10, int(window_ms / max(a.elapsed_time(b) / 3, 1e-3)))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def measure():
    import torch
    import studiogan_amd
    from ew_fold_check import bind_library, workload
    counted = bind_library()
    dev = torch.device("cuda:0")
    print("library:", studiogan_amd.LIB_PATH, "" if counted else "(no sg_ew_vec_launches)")
    res = {}
    for name, shapes in SHAPES.items():
        us = []
        for shape in shapes:
            call, ts = workload(name, shape, dev)
            us.append(1e3 * timeit(call))
            del call, ts
            torch.cuda.empty_cache()
            print(f"{name:18s} {str(shape):34s} {us[-1]:9.1f} us")
        res[name] = sum(us)
    return res


def compare(parent, new, shapes=SHAPES):
    """shapes: {entry point: its shapes}, the keys of the round files (tools/bn_bench.py passes its own)"""
    P, N = [json.load(open(f)) for f in parent], [json.load(open(f)) for f in new]
    assert len(P) >= 3 and len(N) >= 3, "at least three rounds of either build"
    print("shapes:")
    for name, shp in shapes.items():
        print(f"  {name:18s} {shp}")
    print(f"\nbf16, us per entry point (its shapes summed), {len(P)} rounds of the parent build and {len(N)} of the new one, alternating")
    print(f"{'entry point':18s} {'parent median':>14s} {'new median':>12s} {'parent spread (max - min)':>27s}")
    slow = []
    for name in shapes:
        p, n = [r[name] for r in P], [r[name] for r in N]
        pm, nm, spread = statistics.median(p), statistics.median(n), max(p) - min(p)
        over = nm > pm + spread
        slow += [name] * over
        print(f"{name:18s} {pm:14.1f} {nm:12.1f} {spread:27.1f}{'   SLOWER beyond the spread' if over else ''}")
    assert not slow, f"slower than the parent beyond its own spread: {slow}"
    print("no entry point is slower than the parent beyond the parent's own spread")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write this round's times here")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--parent", nargs="+", default=[])
    ap.add_argument("--new", nargs="+", default=[])
    a = ap.parse_args()
    if a.compare:
        compare(a.parent, a.new)
    else:
        res = measure()
        if a.json:
            json.dump(res, open(a.json, "w"))
