"""Outputs of the eight elementwise entry points with a scalar and a 16-byte path (csrc/elementwise.hip: sg_avgpool2_fwd / _bwd, sg_maxpool2_fwd / _bwd,
sg_relu_mask, sg_slice_up_fwd / _bwd, sg_copy_channels) across two builds of the library, bit for bit.

    SG_LIBSGAMD=<library built from the parent commit> python tools/ew_fold_check.py --save ref.pt
    python tools/ew_fold_check.py --against ref.pt

Runs the case table of tests/ew_checks.py in fp32 and bf16 (every case also checks itself against its exact restatement), each vector-path case a second time with
its first input 8 bytes off a 16-byte boundary, and one workload-sized bf16 call per entry point at the first shape tools/ew_bench.py times it at. --against
asserts torch.equal on every output, the max-pool index plane included.

Every key carries which path took the call: whether sg_ew_vec_launches() moved. A build from before the fold has no such counter (and _lib.lib() would refuse it
for the missing symbol: bind_library() binds what the library has); there the key is formed from the gate's documented rule instead -- bf16, channel count and
pitches multiples of 8, 16-byte aligned pointers, 8-byte aligned index plane -- which is what the case table's vec column and the aligned workload shapes state.
Two builds that dispatch differently therefore do not compare.

One input class is left out of the comparison: a SIGNALLING NaN in the max-pool backward's dy. The parent's scalar bf16 kernel sent dy through bf16 -> fp32 ->
bf16, which sets the quiet bit, while its 16-byte twin moved the stored bits; the folded kernel moves the bits on both paths (tests/ew_checks.py holds it to
that), so the case table runs here with its quiet NaNs only (snan=False)."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402


def bind_library():
    """-> True when the library has the counter. Otherwise binds every prototype the library does have, the way _lib.lib() would"""
    import studiogan_amd
    from studiogan_amd import _lib as L
    lib = ctypes.CDLL(studiogan_amd.LIB_PATH)
    if hasattr(lib, "sg_ew_vec_launches"):
        L.lib()
        return True
    lib.sg_last_error.restype = ctypes.c_char_p
    for name, args in L._PROTOS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, ctypes.c_int
    L._lib = lib
    return False


def workload(name, shape, dev):
    """one bf16 call of `name` at a shape of tools/ew_bench.py on seeded random operands -> (the call as a closure, its output tensors)"""
    from studiogan_amd import _lib as L
    g = torch.Generator(device=dev).manual_seed(len(name) + sum(shape))
    bt, st = L.dt(torch.bfloat16), L.stream
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.bfloat16)
    out = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
    p = L.ptr
    if name in ("sg_avgpool2_fwd", "sg_avgpool2_bwd"):
        N, H, W, C = shape
        a, b = (rnd(N, H, W, C), out(N, H // 2, W // 2, C)) if name.endswith("fwd") else (rnd(N, H // 2, W // 2, C), out(N, H, W, C))
        return (lambda: L.call(name, bt, p(a), p(b), N, H, W, C, st())), (b,)
    if name == "sg_maxpool2_fwd":
        N, H, W, C = shape
        x, y, idx = rnd(N, H, W, C), out(N, H // 2, W // 2, C), torch.zeros(N, H // 2, W // 2, C, dtype=torch.uint8, device=dev)
        return (lambda: L.call(name, bt, p(x), C, p(y), C, p(idx), N, H, W, C, st())), (y, idx)
    if name == "sg_maxpool2_bwd":
        N, H, W, C = shape
        dy, dx = rnd(N, H // 2, W // 2, C), out(N, H, W, C)
        idx = torch.randint(0, 4, (N, H // 2, W // 2, C), generator=g, device=dev).to(torch.uint8)
        return (lambda: L.call(name, bt, p(dy), C, p(idx), p(dx), C, N, H, W, C, st())), (dx,)
    if name == "sg_relu_mask":
        (n,) = shape
        dy, x, dx = rnd(n), rnd(n), out(n)
        return (lambda: L.call(name, bt, p(dy), p(x), p(dx), n, st())), (dx,)
    if name in ("sg_slice_up_fwd", "sg_slice_up_bwd"):
        N, Hs, Ws, ld, C, up = shape
        a, b = (rnd(N, Hs, Ws, ld), out(N, Hs * up, Ws * up, C)) if name.endswith("fwd") else (rnd(N, Hs * up, Ws * up, C), out(N, Hs, Ws, ld))
        return (lambda: L.call(name, bt, p(a), p(b), N, Hs, Ws, ld, C, up, st())), (b,)
    assert name == "sg_copy_channels"
    rows, C, lds, ldd = shape
    src, dst = rnd(rows, lds), out(rows, ldd)
    return (lambda: L.call(name, bt, p(src), lds, p(dst), ldd, rows, C, st())), (dst,)


def run(counted, dev=torch.device("cuda:0")):
    import ew_checks as EC
    import ew_bench as EB
    outs = {}
    path = lambda moved, rule: "vec" if (moved if counted else rule) else "scalar"
    for case in EC.CASES:
        op, spec, sh, vec = case
        for dtype in EC.DTYPES:
            for shift, rule in ((sh, vec and dtype == torch.bfloat16),) + ((({"in": 8}, False),) if vec else ()):
                moved, res = op(dev, dtype, shift, snan=False, **spec)
                outs[f"{EC.case_id((op, spec, shift, vec))} {str(dtype)[6:]} [{path(moved, rule)}]"] = tuple(res[k] for k in sorted(res))
    from studiogan_amd import _lib as L
    for name, shapes in EB.SHAPES.items():
        call, ts = workload(name, shapes[0], dev)
        n0 = L.lib().sg_ew_vec_launches() if counted else 0
        call()
        moved = L.lib().sg_ew_vec_launches() - n0 if counted else 0
        outs[f"workload {name} {shapes[0]} [{path(moved, True)}]"] = tuple(t.cpu() for t in ts)
    return outs


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--save")
    g.add_argument("--against")
    a = ap.parse_args()
    import studiogan_amd
    counted = bind_library()
    print("library:", studiogan_amd.LIB_PATH, "(counts its vector launches)" if counted else "(no sg_ew_vec_launches: paths by the gate's rule)")
    outs = run(counted)
    if a.save:
        torch.save(outs, a.save)
        print(f"saved {len(outs)} cases to {a.save}")
    else:
        ref = torch.load(a.against)
        assert ref.keys() == outs.keys(), f"the two runs cover different cases or took different paths: {sorted(set(ref) ^ set(outs))[:6]}"
        bad = 0
        bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t      # (on the stored bits: a NaN equals itself)
        for k, ts in outs.items():
            eq = len(ts) == len(ref[k]) and all(torch.equal(bits(t), bits(r)) for t, r in zip(ts, ref[k]))
            bad += not eq
            print(f"{k:100s} {'equal' if eq else 'DIFFERS'}")
        assert bad == 0, f"{bad} of {len(outs)} cases differ from {a.against}"
        print(f"all {len(outs)} cases bit-identical to {a.against}")
