"""Batch-norm apply pass alone (csrc/norm.hip sg_bn_apply: y = relu(((x - mean) * invstd) * gain[n] + bias[n]), bf16, the conditional form of BigGAN's generator) on the
activation shapes of BigGAN-128's generator at batch 256, per SG_BN_APPLY variant ("<variant><blocks / 1024>", read once per process: this script re-runs itself per value).
    python tools/bn_bench.py [--variants 02,12,22,32,04,14]
GB/s = (read + write of the activation) / hipEvent time.

--entry-points times every streaming and reducing entry point of the file instead (ENTRY_POINTS below; bf16, the first three shapes, operands and calls of
tools/bn_fold_check.py), with device events over at least 100 ms of calls per shape, the default variant of sg_bn_apply. One process is one round:
    python tools/bn_bench.py --entry-points --json new1.json
    SG_LIBSGAMD=<library built from the parent commit> python tools/bn_bench.py --entry-points --json parent1.json
    python tools/bn_bench.py --compare --parent parent1.json parent2.json parent3.json --new new1.json new2.json new3.json
Run the two builds alternating. --compare is tools/ew_bench.py's: per entry point (its shapes' times summed) the median of either build's rounds and the parent's own
spread (max - min); it fails where the new median exceeds the parent's by more than that spread."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = [(256, 128 * 128, 96), (256, 64 * 64, 192), (256, 32 * 32, 384), (256, 16 * 16, 768), (256, 8 * 8, 1536), (256, 4 * 4, 1536)]
ENTRY_POINTS = ("sg_bn_partial_stats", "sg_bn_apply", "sg_bn_bwd_reduce", "sg_bn_bwd_apply_res", "sg_bn_bwd2_reduce", "sg_bn_bwd2_apply", "sg_cbn_bwd2_reduce", "sg_cbn_bwd2_apply")


def entry_points():
    """-> {entry point: us, its three shapes summed}"""
    import torch
    import studiogan_amd
    from ew_bench import timeit
    from bn_fold_check import Operands, workload
    dev = torch.device("cuda:0")
    print("library:", studiogan_amd.LIB_PATH)
    res = dict.fromkeys(ENTRY_POINTS, 0.0)
    for shape in SHAPES[:3]:
        o = Operands(shape, dev)
        for name in ENTRY_POINTS:
            call, _ = workload(name, o)
            us = 1e3 * timeit(call)
            res[name] += us
            print(f"{name:20s} {str(shape):18s} {us:9.1f} us")
        del o
        torch.cuda.empty_cache()
    return res


def child():
    import torch
    import studiogan_amd  # noqa: F401
    from studiogan_amd import _lib as L
    dev = torch.device("cuda:0")
    tot = 0.0
    line = []
    for (N, HW, C) in SHAPES:
        x = torch.randn(N, HW, C, device=dev).to(torch.bfloat16)
        y = torch.empty_like(x)
        mean, invstd = torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5
        gain, bias = torch.randn(N, C, device=dev), torch.randn(N, C, device=dev)

        def fn():
            L.call("sg_bn_apply", L.dt(torch.bfloat16), x.data_ptr(), y.data_ptr(), N, HW, C, mean.data_ptr(), invstd.data_ptr(), gain.data_ptr(), bias.data_ptr(), C, 1, L.stream())
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) / 20 * 1e3
        tot += us
        line.append(f"{us:7.1f} us {2.0 * x.numel() * 2 / us / 1e3:6.0f} GB/s")
    print(f"SG_BN_APPLY={os.environ.get('SG_BN_APPLY', '(default)'):10s} | " + " | ".join(line) + f" | sum {tot:7.1f} us")


if __name__ == "__main__":
    if os.environ.get("SG_BN_BENCH_CHILD") == "1":
        child()
    else:
        ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
        ap.add_argument("--variants", default="02,12,22,32,04,14,24,34")
        ap.add_argument("--entry-points", action="store_true", help="time every entry point of ENTRY_POINTS once (one round)")
        ap.add_argument("--json", help="write this round's times here")
        ap.add_argument("--compare", action="store_true")
        ap.add_argument("--parent", nargs="+", default=[])
        ap.add_argument("--new", nargs="+", default=[])
        args = ap.parse_args()
        if args.compare or args.entry_points:
            if args.compare:
                from ew_bench import compare
                compare(args.parent, args.new, {name: SHAPES[:3] for name in ENTRY_POINTS})
            else:
                res = entry_points()
                if args.json:
                    json.dump(res, open(args.json, "w"))
            sys.exit(0)
        print("shapes (N, HW, C): " + " ".join(str(s) for s in SHAPES))
        for v in args.variants.split(","):
            env = dict(os.environ, SG_BN_BENCH_CHILD="1", SG_BN_APPLY=v)
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
            out = [ln for ln in r.stdout.splitlines() if ln.startswith("SG_BN_APPLY")]
            print(out[0] if out else ("failed: " + r.stderr[-300:]))
