"""Outputs of the batch-norm entry points (csrc/norm.hip: sg_bn_* / sg_cbn_*) across two builds of the library, bit for bit.

    SG_LIBSGAMD=<library built from the parent commit> python tools/bn_fold_check.py --save ref.pt
    python tools/bn_fold_check.py --against ref.pt

(a) The case table of tests/bn_checks.py in both dtypes (every case also checks itself against fp64 as in the test), further statistics cases of this tool, and
    the per-sample second-order stages (tests/logan_cbn_checks.py bn_product, both row layouts). Every buffer a case hands to bn_checks.guard and every tensor the
    end-to-end cases compare is kept, sentinel bytes included; --against asserts torch.equal on the stored bits. Every key carries which kernels ran: by how much each
    sg_bn_path_launches counter moved over the case, so two builds that dispatch differently do not compare.
    Where float or double atomics of MORE THAN TWO blocks meet at one address the result is not fixed between two runs of one build (two adds into a zeroed cell
    commute, three do not associate). Those cases are left out, by the grid rules of the host code restated in blocks_per_address(); the number left out is printed
    per check and has to stay below the number kept.
(b) The reductions at many-block geometries (rows = 4418, C = 64; N = 2, HW = 700, C = 64 and 128), streaming and generic kernel, on DYADIC inputs: multiples of 1/4,
    invstd and gains powers of two, so that every partial sum is exact in its accumulator and the result cannot depend on the order of the atomics. Asserted equal to
    the exact sum computed on the CPU, under whichever build runs; the sums are kept for --against too. Catches lost or doubled pixels at scale; blind to re-ordering,
    which is what (a) is for.
(c) One bf16 call per elementwise entry point (sg_bn_apply, sg_bn_bwd_apply_res, sg_bn_bwd2_apply, sg_cbn_bwd2_apply) at the first shape of tools/bn_bench.py, on
    seeded device-side inputs; outputs of 0.8 GB each are kept as their SHA-256."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

ELEMENTWISE = ("sg_bn_apply", "sg_bn_bwd_apply_res", "sg_bn_bwd2_apply", "sg_cbn_bwd2_apply")
REDUCTIONS = ("sg_bn_partial_stats", "sg_bn_bwd_reduce", "sg_bn_bwd2_reduce", "sg_cbn_bwd2_reduce")


def cdiv(a, b):
    return -(-a // b)


# ---- the grids of the accumulating kernels, from the host code of csrc/norm.hip ----------------------------------------------------------------------------------------
def stat_blocks(rows, C, V, stream):
    if stream:
        return cdiv(rows, max(cdiv(rows, 1024), 32 * (256 // (C // V))))
    return cdiv(rows, max(cdiv(rows, max(2048 // cdiv(C, 64), 1)), 64))


def reduce_blocks(N, HW, C, V, stream):
    if stream:
        return cdiv(HW, max(cdiv(HW, max(2048 // N, 1)), 8 * (256 // (C // V))))
    return cdiv(HW, max(cdiv(HW, max(2048 // (cdiv(C, 64) * N), 1)), 16))


def blocks_per_address(fn, spec, dtype):
    """the largest number of blocks that add into one address in any launch of the case (1: nothing is accumulated across blocks)"""
    import bn_checks as BC
    V = BC.V(dtype)
    if fn is BC.partial_case:
        return stat_blocks(spec["rows"], spec["C"], V, BC.want_path(spec, dtype) == "stream")
    if fn is BC.reduce_case:
        return reduce_blocks(spec["N"], spec["HW"], spec["C"], V, BC.want_path(spec, dtype) == "stream")
    if fn is BC.bwd2_pitch_case:
        return reduce_blocks(spec["N"], spec["HW"], spec["C"], V, False)
    if fn in (BC.e2e_rows_case, BC.e2e_chan_case):      # torch allocations are 16-byte aligned: the gates are the shape's
        N, H, W, C = spec["shape"]
        vec = C % V == 0
        n = [reduce_blocks(N, H * W, C, V, vec and C // V <= 256 and H * W >= 16), reduce_blocks(N, H * W, C, V, False)]
        if spec["ub"]:
            n.append(stat_blocks(N * H * W, C, V, vec and C // V <= 128 and N * H * W >= 4096))
        return max(n)
    return 1


def extra_cases():
    """statistics cases besides the table's, at most two blocks per address: generic kernel up to 128 rows, streaming kernel with at most four channel vectors"""
    import bn_checks as BC
    out = []
    for rows in (1, 64, 65, 128):
        for C in (6, 72):
            out.append((BC.partial_case, dict(rows=rows, C=C, path="generic"), True, False))
    out.append((BC.partial_case, dict(rows=128, C=64, ldx=65, path="generic"), True, False))
    out.append((BC.partial_case, dict(rows=128, C=64, shift={"x": 8}, path="generic"), True, False))
    for k in (1, 2, 3, 4):                     # C = k channel vectors of either dtype
        out.append((BC.partial_case, dict(rows=4096, C={"bf16": 8 * k, "fp32": 4 * k}, path="stream"), True, False))
    out.append((BC.partial_case, dict(rows=5000, C={"bf16": 8, "fp32": 4}, path="stream"), True, False))
    out.append((BC.reduce_case, dict(N=2, HW={"bf16": 512, "fp32": 256}, C=64, relu=1, path="stream"), True, False))      # gx = 2; bf16: two unrolled trips per block
    # end to end at shapes small enough for every reduction of the pass (most of the table's end-to-end shapes are not): appended to the table's shape lists, which
    # is where bn_checks.e2e_inputs looks a shape's seed up
    rows, chan = [(3, 4, 4, 8), (5, 3, 2, 72)], [(2, 4, 4, 8), (3, 3, 3, 6), (2, 5, 3, 72)]
    BC.ROWS_SHAPES += [s for s in rows if s not in BC.ROWS_SHAPES]
    BC.CHAN_SHAPES += [s for s in chan if s not in BC.CHAN_SHAPES]
    out += [(BC.e2e_rows_case, dict(shape=s, relu=relu, ub=ub, packed=(relu == ub)), True, False) for s in rows for relu in (0, 1) for ub in (0, 1)]
    out += [(BC.e2e_chan_case, dict(shape=s, relu=relu, ub=ub), True, False) for s in chan for relu, ub in BC.CHAN_GRID]
    out += [(BC.e2e_chan_case, dict(shape=chan[0], relu=1, ub=1, drop=drop), True, False) for drop in ("dy", "x")]
    return out


def per_dtype(spec, dtype):
    import bn_checks as BC
    return {k: (v[BC.DT_ID[dtype]] if isinstance(v, dict) and k != "shift" and k != "path" else v) for k, v in spec.items()}


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def counters():
    import bn_checks as BC
    lib = BC._L().lib()
    return {f"{e}.{k}": lib.sg_bn_path_launches(v) for e, ks in BC.PATHS.items() for k, v in ks.items()}


def moved(n0):
    n1 = counters()
    return " ".join(f"{k}+{n1[k] - n0[k]}" for k in n1 if n1[k] != n0[k]) or "no counted kernel"


def case_table(dev, outs):
    import bn_checks as BC
    import logan_cbn_checks as LC
    kept, left = {}, {}
    got = []
    guard0, compare0 = BC.guard, BC._compare

    def guard(buf, name):
        guard0(buf, name)
        got.append((name, buf.dev.cpu()))

    def compare(R, g, ref, bounds, bf16, keys):
        compare0(R, g, ref, bounds, bf16, keys)
        got.extend((k, g[k].detach().cpu()) for k in keys)

    BC.guard, BC._compare = guard, compare
    try:
        for case in list(BC.CASES) + extra_cases():
            fn = case[0]
            for dtype in (BC.DTYPES if case[2] else (torch.float32,)):
                spec = per_dtype(case[1], dtype)
                name = fn.__name__[:-5]
                if blocks_per_address(fn, spec, dtype) > 2:
                    left[name] = left.get(name, 0) + 1
                    continue
                kept[name] = kept.get(name, 0) + 1
                del got[:]
                n0 = counters()
                BC.run_case((fn, spec), dev, dtype)
                key = f"{BC.param_id(((fn, spec, case[2], False), dtype))} [{moved(n0)}]"
                assert key not in outs and got, key
                outs[key] = tuple(t for _, t in got)
    finally:
        BC.guard, BC._compare = guard0, compare0
    # the per-sample second-order stages: reduce (HW <= 32), finalize, apply, gain rows, behind functional.BNFn
    for shape in LC.BN_SHAPES + LC.BN_EXTRA_SHAPES:
        si = (LC.BN_SHAPES + LC.BN_EXTRA_SHAPES).index(shape)
        N, H, W, C = shape
        for bf16 in (False, True):
            for ci, (relu, ub, fl) in enumerate(LC.bn_grid(shape)):
                dtype = torch.bfloat16 if bf16 else torch.float32
                if blocks_per_address(BC.e2e_rows_case, dict(shape=shape, ub=ub), dtype) > 2:
                    left["cbn stages"] = left.get("cbn stages", 0) + 2
                    continue
                inp = LC.bn_inputs(shape, relu, ub, 100 * si + ci, bf16=bf16, **fl)
                for packed in (True, False):
                    kept["cbn stages"] = kept.get("cbn stages", 0) + 1
                    n0 = counters()
                    p = LC.bn_product(inp, relu, ub, packed, dev, bf16)
                    outs[f"cbn stages {shape} relu={relu} batch={ub} {fl or ''} {'packed' if packed else 'separate'} {'bf16' if bf16 else 'fp32'} [{moved(n0)}]"] = \
                        tuple(p[k].detach().cpu() for k in sorted(p))
    print("(a) cases kept / left out for more than two blocks per address:")
    for name in sorted(set(kept) | set(left)):
        print(f"    {name:14s} {kept.get(name, 0):4d} / {left.get(name, 0):3d}")
        assert left.get(name, 0) < kept.get(name, 0), f"{name}: more cases left out than kept"


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def dyadic(dev, outs):
    import bn_checks as BC
    L = BC._L()
    g = torch.Generator().manual_seed(5)
    quarter = lambda *s, lim=8: torch.randint(-lim, lim + 1, s, generator=g).double() / 4.0
    pow2 = lambda *s: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, s, generator=g)]
    p = L.ptr
    n = 0
    for dtype in BC.DTYPES:
        dn = BC.DT_ID[dtype]
        for shift in (0, 8):              # 8 bytes off a 16-byte boundary: the generic kernel
            rows, C = 4418, 64
            xv = quarter(rows, C)
            x = BC.Buf(dev, xv.to(dtype), shift)
            part = torch.zeros(2 * C, dtype=torch.float64, device=dev)
            n0 = counters()
            L.call("sg_bn_partial_stats", L.dt(dtype), x.ptr(), C, rows, C, p(part), L.stream())
            ref = torch.stack([xv.sum(0), (xv * xv).sum(0)], 1).reshape(-1)
            key = f"dyadic sg_bn_partial_stats rows={rows} C={C} {dn} [{moved(n0)}]"
            assert torch.equal(part.cpu(), ref), key
            outs[key] = (part.cpu(),)
            n += 1
            for C in (64, 128):
                N, HW = 2, 700
                xv, dyv, uv = quarter(N, HW, C), quarter(N, HW, C), quarter(N, HW, C)
                mean, invstd = quarter(C, lim=4), pow2(C)
                ga = pow2(N, C) * torch.where(torch.rand(N, C, generator=g) < 0.25, -1.0, 1.0)
                bi = quarter(N, C, lim=4)
                xh = (xv - mean) * invstd
                gm = torch.where(xh * ga[:, None, :] + bi[:, None, :] > 0, dyv, torch.zeros_like(dyv))
                ref2 = torch.stack([gm.sum(1), (gm * xh).sum(1)], 2)
                ref5 = torch.stack([uv.sum(1), (uv * xh).sum(1), gm.sum(1), (gm * xh).sum(1), (uv * gm).sum(1)], 2)
                # the per-channel pass: sample 0's rows for every sample
                xh0 = xh
                gm0 = torch.where(xh0 * ga[:1, None, :] + bi[:1, None, :] > 0, dyv, torch.zeros_like(dyv))
                ref5c = torch.stack([uv.sum(1), (uv * xh0).sum(1), gm0.sum(1), (gm0 * xh0).sum(1), (uv * gm0).sum(1)], 2)
                x, dy, u = BC.Buf(dev, xv.to(dtype), shift), BC.Buf(dev, dyv.to(dtype)), BC.Buf(dev, uv.to(dtype))
                md, sd, gd, bd = (t.float().contiguous().to(dev) for t in (mean, invstd, ga, bi))
                for name, args, k, ref in (("sg_bn_bwd_reduce", (x.ptr(), dy.ptr(), N, HW, C, p(md), p(sd), p(gd), p(bd), C, 1), 2, ref2),
                                           ("sg_cbn_bwd2_reduce", (x.ptr(), dy.ptr(), u.ptr(), N, HW, C, p(md), p(sd), p(gd), p(bd), C, 1), 5, ref5),
                                           ("sg_bn_bwd2_reduce", (x.ptr(), dy.ptr(), u.ptr(), N, HW, C, p(md), p(sd), p(gd), p(bd), 1), 5, ref5c)):
                    if shift and name != "sg_bn_bwd_reduce":
                        continue          # (the second-order reduces have one kernel)
                    sums = torch.zeros(N, C, k, dtype=torch.float32, device=dev)
                    n0 = counters()
                    L.call(name, L.dt(dtype), *args, p(sums), L.stream())
                    key = f"dyadic {name} N={N} HW={HW} C={C} {dn}{' x+8B' if shift else ''} [{moved(n0)}]"
                    assert torch.equal(sums.cpu().double(), ref), key
                    outs[key] = (sums.cpu(),)
                    n += 1
    print(f"(b) {n} many-block reductions on dyadic inputs equal the exact sums")


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------------------------------
class Operands:
    """seeded bf16 operands of one (N, HW, C) shape on the device, shared by the entry points (tools/bn_bench.py times them on the same ones)"""

    def __init__(self, shape, dev):
        N, HW, C = shape
        g = torch.Generator(device=dev).manual_seed(N + HW + C)
        rnd = lambda *s, dt=torch.float32: torch.randn(*s, generator=g, device=dev, dtype=dt)
        self.shape = shape
        self.x, self.dy, self.u = (rnd(N, HW, C, dt=torch.bfloat16) for _ in range(3))
        self.o1, self.o2 = torch.zeros_like(self.x), torch.zeros_like(self.x)
        self.mean, self.invstd = rnd(C), torch.rand(C, generator=g, device=dev) + 0.5
        self.gain, self.bias, self.A, self.B = rnd(N, C), rnd(N, C), rnd(N, C), rnd(N, C)
        self.chan = rnd(7 * C).double() * (0.1 * N * HW)
        self.part = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        self.sums = torch.zeros(N, C, 5, dtype=torch.float32, device=dev)


def workload(name, o):
    """one bf16 call of `name` on the operands o -> (the call as a closure, its output tensors)"""
    from studiogan_amd import _lib as L
    N, HW, C = o.shape
    bt, st, p = L.dt(torch.bfloat16), L.stream, L.ptr
    stat = (p(o.mean), p(o.invstd))
    rows, vecs = (p(o.gain), p(o.bias), C), (p(o.gain), p(o.bias))      # per-sample rows of pitch C; sample 0's rows as per-channel vectors
    cnt = float(N * HW)
    calls = {
        "sg_bn_partial_stats": (lambda: L.call(name, bt, p(o.x), C, N * HW, C, p(o.part), st()), (o.part,)),
        "sg_bn_apply": (lambda: L.call(name, bt, p(o.x), p(o.o1), N, HW, C, *stat, *rows, 1, st()), (o.o1,)),
        "sg_bn_bwd_reduce": (lambda: L.call(name, bt, p(o.x), p(o.dy), N, HW, C, *stat, *rows, 1, p(o.sums), st()), (o.sums,)),
        "sg_bn_bwd_apply_res": (lambda: L.call(name, bt, p(o.x), p(o.dy), p(o.o1), N, HW, C, *stat, *rows, 1, p(o.chan), cnt, 1, p(o.u), st()), (o.o1,)),
        "sg_bn_bwd2_reduce": (lambda: L.call(name, bt, p(o.x), p(o.dy), p(o.u), N, HW, C, *stat, *vecs, 1, p(o.sums), st()), (o.sums,)),
        "sg_bn_bwd2_apply": (lambda: L.call(name, bt, p(o.x), p(o.dy), p(o.u), p(o.o1), p(o.o2), N, HW, C, *stat, *vecs, 1, p(o.chan), cnt, 1, st()), (o.o1, o.o2)),
        "sg_cbn_bwd2_reduce": (lambda: L.call(name, bt, p(o.x), p(o.dy), p(o.u), N, HW, C, *stat, *rows, 1, p(o.sums), st()), (o.sums,)),
        "sg_cbn_bwd2_apply": (lambda: L.call(name, bt, p(o.x), p(o.dy), p(o.u), p(o.o1), p(o.o2), N, HW, C, *stat, p(o.gain), p(o.bias), p(o.A), p(o.B), C, 1,
                                             p(o.chan), cnt, 1, st()), (o.o1, o.o2)),
    }
    return calls[name]


def workloads(dev, outs):
    import bn_bench as BB
    o = Operands(BB.SHAPES[0], dev)
    for name in ELEMENTWISE:
        call, ts = workload(name, o)
        for t in ts:
            t.fill_(float("nan"))
        n0 = counters()
        call()
        torch.cuda.synchronize()
        outs[f"workload {name} {o.shape} bf16 [{moved(n0)}]"] = tuple(("sha256", hashlib.sha256(t.cpu().view(torch.int16).numpy().tobytes()).hexdigest(), tuple(t.shape)) for t in ts)
    print(f"(c) {len(ELEMENTWISE)} workload-sized calls at {o.shape}")


def same(a, b):
    if isinstance(a, tuple) and a and a[0] == "sha256":
        return a == b
    bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))      # (on the stored bits: a NaN equals itself)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--save")
    g.add_argument("--against")
    a = ap.parse_args()
    import studiogan_amd
    print("library:", studiogan_amd.LIB_PATH)
    dev = torch.device("cuda:0")
    outs = {}
    case_table(dev, outs)
    dyadic(dev, outs)
    workloads(dev, outs)
    n_t = sum(len(v) for v in outs.values())
    if a.save:
        torch.save(outs, a.save)
        print(f"saved {len(outs)} cases, {n_t} tensors, to {a.save}")
    else:
        ref = torch.load(a.against)
        assert ref.keys() == outs.keys(), f"the two runs cover different cases or took different kernels: {sorted(set(ref) ^ set(outs))[:6]}"
        bad = [k for k, ts in outs.items() if not (len(ts) == len(ref[k]) and all(same(t, r) for t, r in zip(ts, ref[k])))]
        for k in bad:
            print("DIFFERS", k)
        assert not bad, f"{len(bad)} of {len(outs)} cases differ from {a.against}"
        print(f"all {len(outs)} cases, {n_t} tensors, bit-identical to {a.against}")
