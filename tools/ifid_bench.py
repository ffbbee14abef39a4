"""Intra-class FID on the device: the batched small-sample route (metrics.intra_class_frechet, csrc/frechet_small.hip) against the route the package had before it
(per class: moments on the device, then metrics.frechet_inception_distance_device, which falls back to scipy.linalg.sqrtm on the host whenever a covariance is
singular -- always, with fewer samples than dimensions).
    python tools/ifid_bench.py [--shapes 1000x50x2048,10x1000x2048] [--old-classes 2] [--rounds 3] [--out profiles/ifid_bench.txt]
Shapes are classes x samples per class (both sides) x feature width: ImageNet-valid with InceptionV3 features, CIFAR10-test. Features are seeded ReLU-like
fp32 rows resident on the device (about half of them zero, a per-class shift: never all zeros). The batched route is timed end to end (class sort, moments,
cross-Gram, nuclear norms, read-back) over --rounds runs after one warm-up, device-synchronised; the old route is timed on the first --old-classes classes and
scaled to the class count (it is ~10 s of host time per class). Also reported: the Jacobi sweeps, the route of the nuclear norm and the LDS budget.
There is no fallback: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import studiogan_amd  # noqa: E402,F401
from studiogan_amd import metrics as M, _lib as L  # noqa: E402


def features(K, n, C, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    shift = torch.rand(K, 1, C, generator=g, device=dev) * 0.5 - 0.25
    f = torch.relu(torch.randn(K, n, C, generator=g, device=dev) + shift).reshape(K * n, C).contiguous()
    return f, torch.arange(K, device=dev).repeat_interleave(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x50x2048,10x1000x2048")
    ap.add_argument("--old-classes", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ifid_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    budget = L.lib().sg_seg_nuclear_lds_budget()
    say(f"# tools/ifid_bench.py  --shapes {a.shapes} --old-classes {a.old_classes} --rounds {a.rounds}    ({torch.cuda.get_device_name(0)})")
    say(f"LDS budget of sg_seg_nuclear_norm: {budget} bytes per workgroup (largest square: 126 x 126); larger matrices: padded square route (sg_jacobi_sweep)")
    wf, wl = features(4, 8, 64, 1, dev)
    M.intra_class_frechet(wf, wl, wf.flip(0), wl, 4)      # warm-up: module load
    for shape in a.shapes.split(","):
        K, n, C = (int(v) for v in shape.split("x"))
        fa, la = features(K, n, C, 11, dev)
        fb, lb = features(K, n, C, 12, dev)
        fb = fb * 1.2 + 0.1
        torch.cuda.synchronize()
        times, stats = [], {}
        for r in range(a.rounds + 1):
            stats = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            new = M.intra_class_frechet(fa, la, fb, lb, K, stats=stats)
            torch.cuda.synchronize()
            if r:
                times.append(time.perf_counter() - t0)
        t_new = statistics.median(times)
        ko = min(a.old_classes, K)
        old, t0 = [], time.perf_counter()
        for k in range(ko):
            m1, s1 = M.calculate_moments(fa[k * n:(k + 1) * n])
            m2, s2 = M.calculate_moments(fb[k * n:(k + 1) * n])
            old.append(M.frechet_inception_distance_device(m1, s1, m2, s2))
        t_old = (time.perf_counter() - t0) / ko
        rel = max(abs(new[k] - old[k]) / abs(old[k]) for k in range(ko))
        sw = np.array(stats["sweeps"])
        say()
        say(f"{K} classes x {n} samples x {C} features   (cross-Gram matrices {n} x {n}, route: {sorted(set(stats['route']))})")
        say(f"  batched sample route, all {K} classes : median {t_new * 1e3:10.1f} ms   (min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f} over {a.rounds} runs)"
            f"   = {t_new / K * 1e3:.3f} ms per class")
        say(f"  previous route (host sqrtm fallback)  : {t_old:10.2f} s per class over {ko} classes  -> {t_old * K:.0f} s for {K} classes (scaled)")
        say(f"  ratio                                 : {t_old * K / t_new:10.0f} x")
        say(f"  Jacobi sweeps                         : min {sw.min()}, median {int(np.median(sw))}, max {sw.max()} (cap 40)")
        say(f"  largest relative difference between the two routes over the {ko} classes: {rel:.2e} (the host route carries scipy's sqrtm error on a singular product)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
