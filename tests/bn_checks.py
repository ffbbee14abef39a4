"""Checks of the batch-norm kernels (csrc/norm.hip) on every path their entry points dispatch to, written once for both places they run: the GPU
(tests/test_bn_gpu.py) and the kernel sources on the CPU interpreter (tests/test_bn_cpu.py under hipemu.fullemu.Installed).

Stage-level cases run ONE kernel on GIVEN inputs: mean, invstd and the channel terms are arbitrary values, not the statistics of x, so that an error of one stage
cannot cancel in the next; the reference is an fp64 restatement on the same rounded inputs. Every output lives inside sentinel bytes (ew_checks.Buf) and the whole
buffer is read back. Every case names the kernel it expects (sg_bn_path_launches): that counter moves by exactly one, the others of the entry point not at all.

Bounds, none of them tuned on the code under test:
  statistics      from the documented summation: generic kernel (fp64 throughout) rows 2^-52 sum|term|; streaming kernel (fp32 sums of 32 terms flushed into fp64, one
                  rounding for the square) 34 2^-24 sum|term|. The data is chosen so that every row's share of either sum exceeds ten times the bound (asserted).
  finalize        mean and invstd: one fp32 rounding of an fp64 value, 2^-23 relative; the running statistics: three such roundings of their larger term.
  apply           (number of fp32 roundings in the expression) 2^-24 (|x - mean| invstd |gain| + |bias|) per element; bf16 outputs: plus 2^-8 |ref|.
  backward stages and the end-to-end outputs: the scheme of logan_cbn_checks. Per output, torch fp32 on the CPU against torch fp64 on the same inputs (max-abs error
                  over the tensor's max-abs), the largest over the cases of the check; 4x that for the atomics' summation order, floor 1e-6; bf16 tensors: 2^-8 |ref| per
                  element plus that bound times max|ref|. Computed again in every process; one run's values are recorded in profiles/bn_bounds.txt (write_bounds).
Exact checks: the kernels of one entry point write the SAME BYTES on identical logical inputs (streaming variants 0-3, the scalar kernel on a shifted pointer, the
generic 16-byte kernel), sg_bn_bwd2_reduce and sg_cbn_bwd2_reduce (one kernel, k_cbn_bwd2_reduce, at row pitch 0 / C / 2 C) on the same values, and forward and
backward agree on the ReLU mask element for element on inputs planted within a few fp32 ulps of a zero pre-activation.

Not covered: more than one unrolled trip of the BACKWARD streaming kernels (k_bn_bwd_reduce_stream has a floor of two trips per block, k_bn_bwd_apply_stream of one;
their workgroup target is fixed at 2048, so a longer walk needs tensors above 50 M elements); the RCCL / peer-store statistics paths; sg_bn_stats_from_tiles
(tests/test_quad_gpu.py)."""
import functools
import os
import re

import torch

from ew_checks import Buf, SENT, sentinel

EPS = 1e-4
U = 2.0 ** -24            # fp32 unit roundoff
BF16 = 2.0 ** -8          # bf16 (one rounding of a result), as logan_cbn_checks
FLOOR = 1e-6
MARGIN = 4.0
DTYPES = (torch.float32, torch.bfloat16)
DT_ID = {torch.float32: "fp32", torch.bfloat16: "bf16"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (entry point, kernel) -> the value of SG_BN_PATH_* in include/sgamd.h (header_paths() reads the header; test_bn_cpu compares)
PATHS = {"partial": {"generic": 0, "stream": 1}, "apply": {"scalar": 2, "vec": 3, "stream": 4}, "bwd_reduce": {"generic": 5, "stream": 6},
         "bwd_apply": {"scalar": 7, "vec": 8, "stream": 9}, "cbn_bwd2_apply": {"scalar": 10, "vec": 11},
         "apply_stream": {"v0": 12, "v1": 13, "v2": 14, "v3": 15}}      # which instantiation a streaming launch of sg_bn_apply was, counted besides apply / stream


def header_paths():
    """include/sgamd.h's enum -> {entry: {kernel: value}} and SG_BN_PATH_COUNT"""
    hdr = open(os.path.join(ROOT, "include", "sgamd.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"SG_BN_PATH_([A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    out = {}
    for name, v in vals.items():
        if name != "COUNT":
            entry, kern = name.rsplit("_", 1)
            out.setdefault(entry.lower(), {})[kern.lower()] = v
    return out, vals["COUNT"]


def V(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def _L():
    from studiogan_amd import _lib as L
    return L


def launch(entry, name, *args):
    """one library call -> by how much every counter of `entry` moved"""
    L = _L()
    lib = L.lib()
    n0 = {k: lib.sg_bn_path_launches(v) for k, v in PATHS[entry].items()} if entry else {}
    L.call(name, *args, L.stream())
    return {k: lib.sg_bn_path_launches(v) - n0[k] for k, v in PATHS[entry].items()} if entry else {}


def took(moved, path, what=""):
    assert moved == {k: int(k == path) for k in moved}, f"{what}: expected the {path} kernel, the counters moved by {moved}"


def want_path(spec, dtype):
    p = spec["path"]
    return p[DT_ID[dtype]] if isinstance(p, dict) else p


def gen(seed):
    return torch.Generator().manual_seed(seed)


def q(t, dtype):
    """one rounding to dtype, back in fp64"""
    return t.to(dtype).double()


def f32(t):
    return t.float().double()


def read(buf, dtype, shape):
    return buf.dev[buf.lo:buf.hi].cpu().clone().view(dtype).reshape(shape)


def raw(buf):
    return buf.dev[buf.lo:buf.hi].cpu().clone()


def guard(buf, name):
    g = buf.dev.cpu()
    assert bool((g[:buf.lo] == SENT).all()) and bool((g[buf.hi:] == SENT).all()), f"{name}: bytes outside the region were written"


def same_bytes(a, b, what):
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} bytes differ"


def dptr(t):
    return None if t is None else _L().ptr(t)


class Report:
    """every comparison of a case printed (error over range, error over bound), one failure at the end"""

    def __init__(self, tag):
        self.tag, self.bad, self.rows = tag, [], []

    def within(self, name, got, ref, bound):
        got, ref = got.double().reshape(-1), ref.double().reshape(-1)
        bound = bound.double().reshape(-1) if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
        assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
        err = (got - ref).abs()
        ok = bool(torch.isfinite(got).all()) and bool((err <= bound).all())
        rng = max(float(ref.abs().max()), 1e-300)
        over = float((err / bound.clamp_min(1e-300)).max()) if bool(torch.isfinite(got).all()) else float("inf")
        self.rows.append((name, float(err.max()) / rng, over))
        print(f"[{self.tag}] {name:14s} err {float(err.max()) / rng:.3e} of range, {over:.3e} of its bound {'ok' if ok else 'FAIL'}")
        if not ok:
            self.bad.append(name)

    def finish(self):
        assert not self.bad, f"{self.tag}: {self.bad} beyond the bound"
        return self.rows


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def measured(ref, bound, bf16_out):
    """the absolute bound of an output whose relative fp32 bound was measured on the reference side"""
    mx = float(ref.abs().max())
    return BF16 * ref.abs() + bound * mx if bf16_out else torch.full_like(ref, bound * mx)


# ---- affine layouts ---------------------------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("none", "gain", "bias", "chan", "sample", "packed")


def affine(layout, N, C, g):
    """-> fp32-valued gain / bias as [N, C] fp64 (what every element sees) and how the layout stores them"""
    per_n = layout in ("sample", "packed")
    rows = N if per_n else 1
    ga = (1.0 + 0.3 * torch.randn(rows, C, generator=g, dtype=torch.float64)).clamp(0.3, 2.0)
    ga[:, 1 % C] = -ga[:, 1 % C]                     # one channel with negative gains
    bi = 0.3 * torch.randn(rows, C, generator=g, dtype=torch.float64)
    ga, bi = f32(ga), f32(bi)
    if layout in ("none", "bias"):
        ga = torch.ones_like(ga)
    if layout in ("none", "gain"):
        bi = torch.zeros_like(bi)
    return dict(layout=layout, ga=ga.expand(N, C).clone(), bi=bi.expand(N, C).clone(), rows=rows)


def affine_dev(a, C, dev):
    """-> (tensors to keep alive, gain pointer, bias pointer, gb_stride_n)"""
    lay, ga, bi, rows = a["layout"], a["ga"][:a["rows"]], a["bi"][:a["rows"]], a["rows"]
    if lay == "packed":
        t = torch.cat([ga, bi], 1).float().contiguous().to(dev)
        return [t], dptr(t), dptr(t) + 4 * C, 2 * C
    g = ga.float().contiguous().to(dev) if lay in ("gain", "chan", "sample") else None
    b = bi.float().contiguous().to(dev) if lay in ("bias", "chan", "sample") else None
    return [g, b], dptr(g), dptr(b), C if lay == "sample" else 0


def elem_inputs(spec, dtype, backward=False):
    """x (rounded to dtype), arbitrary fp32 mean / invstd, the affine rows; backward: dy, res (rounded), arbitrary fp64 channel terms. With the fused ReLU no
    pre-activation lies within 1e-3 of zero in a backward case (asserted), so that the fp32 mask cannot differ from the fp64 one"""
    N, HW, C = spec["N"], spec["HW"], spec["C"]
    g = gen(spec.get("seed", 1) + 1000 * N + 10 * HW + C)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = q(r(N, HW, C) * (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) + 0.3 * r(C), dtype)
    mean, invstd = f32(0.2 * r(C)), f32(0.5 + torch.rand(C, generator=g, dtype=torch.float64))
    a = affine(spec.get("layout", "sample"), N, C, g)
    inp = dict(x=x, mean=mean, invstd=invstd, aff=a)
    if backward:
        count = float(N * HW)
        inp.update(dy=q(r(N, HW, C), dtype), res=q(r(N, HW, C), dtype), chan=r(C, 2) * count * 0.3, count=count)
        if spec.get("relu"):
            ga, bi = a["ga"][:, None, :], a["bi"][:, None, :]
            pre = lambda xx: (xx - mean) * invstd * ga + bi
            for _ in range(50):
                v = pre(x)
                bad = v.abs() < 2e-2
                if not bool(bad.any()):
                    break
                x = q(torch.where(bad, mean + (torch.where(v >= 0, 0.1, -0.1) - bi) / (ga * invstd), x), dtype)
            assert float(pre(x).abs().min()) >= 1e-3, "a ReLU input of the case sits within 1e-3 of zero"
            inp["x"] = x
    return inp


def stat_dev(inp, dev):
    return inp["mean"].float().to(dev), inp["invstd"].float().to(dev)


# ---- sg_bn_partial_stats ----------------------------------------------------------------------------------------------------------------------------------------------
def partial_case(spec, dev, dtype):
    rows, C = spec["rows"], spec["C"]
    ldx = spec.get("ldx", C) if not spec.get("pitch_v") else C + V(dtype)
    g = gen(7 + rows + C)
    # per-channel offsets of 6 to 8 standard deviations (sum x^2 is dominated by mean^2), deviations cut at 2.5: no element near zero, so that every row's share
    # of either sum stands clear of the bound
    off = (6.0 + 2.0 * torch.rand(C, generator=g, dtype=torch.float64)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    xv = q(off + torch.randn(rows, C, generator=g, dtype=torch.float64).clamp(-2.5, 2.5), dtype)
    full = torch.full((rows, ldx), 1e30, dtype=torch.float64)          # the pad columns of a pitched input
    full[:, :C] = xv
    x = Buf(dev, full.to(dtype), spec.get("shift", {}).get("x", 0))
    out = Buf(dev, torch.zeros(2 * C, dtype=torch.float64))
    path = want_path(spec, dtype)
    moved = launch("partial", "sg_bn_partial_stats", _L().dt(dtype), x.ptr(), ldx, rows, C, out.ptr())
    got = read(out, torch.float64, (C, 2))
    guard(out, "partial")
    took(moved, path, "sg_bn_partial_stats")
    ref = torch.stack([xv.sum(0), (xv * xv).sum(0)], 1)
    mag = torch.stack([xv.abs().sum(0), (xv * xv).sum(0)], 1)
    bound = (rows * 2.0 ** -52 if path == "generic" else 34.0 * U) * mag
    share = torch.stack([xv.abs().min(0).values, (xv * xv).min(0).values], 1)
    assert bool((share > 10.0 * bound).all()), "a row's share of a sum is within ten times the bound: a dropped row could pass"
    R = Report(f"partial_stats {DT_ID[dtype]} {spec_id(spec)}")
    R.within("sum x", got[:, 0], ref[:, 0], bound[:, 0])
    R.within("sum x^2", got[:, 1], ref[:, 1], bound[:, 1])
    return R.finish()


# ---- sg_bn_finalize / sg_bn_from_running ------------------------------------------------------------------------------------------------------------------------------
def finalize_case(spec, dev, dtype=None):
    C, count, running = 300, float(spec["count"]), spec["running"]
    g = gen(31 + int(count))
    m = 3.0 * torch.randn(C, generator=g, dtype=torch.float64)
    var = 0.1 + torch.rand(C, generator=g, dtype=torch.float64)
    if count == 1.0:
        var = torch.zeros(C, dtype=torch.float64)                      # one row: sum x^2 = x^2
    part = torch.stack([m * count, (var + m * m) * count], 1)
    part[7, 1] = (m[7] * m[7] - 1e-9) * count                          # a slightly negative variance: the clamp, invstd = 1 / sqrt(eps)
    eps, mom = float(torch.tensor(EPS, dtype=torch.float32)), float(torch.tensor(0.1, dtype=torch.float32))
    rm0, rv0 = f32(0.1 * torch.randn(C, generator=g)), f32(0.5 + torch.rand(C, generator=g))
    pd = part.contiguous().to(dev)
    mean, invstd = Buf(dev, sentinel((C,), torch.float32)), Buf(dev, sentinel((C,), torch.float32))
    rm, rv = Buf(dev, rm0.float()), Buf(dev, rv0.float())
    launch(None, "sg_bn_finalize", dptr(pd), count, C, EPS, 0.1, mean.ptr(), invstd.ptr(), rm.ptr() if running else None, rv.ptr() if running else None)
    mr = part[:, 0] / count
    vr = (part[:, 1] / count - mr * mr).clamp_min(0.0)
    assert float(part[7, 1] / count - mr[7] * mr[7]) < 0.0 and float(vr[7]) == 0.0
    ir = 1.0 / torch.sqrt(vr + eps)
    R = Report(f"finalize count={count:g} running={running}")
    R.within("mean", read(mean, torch.float32, (C,)), mr, 2.0 ** -23 * mr.abs())
    R.within("invstd", read(invstd, torch.float32, (C,)), ir, 2.0 ** -23 * ir)
    assert float(read(invstd, torch.float32, (C,))[7]) == float(torch.tensor(1.0 / eps ** 0.5, dtype=torch.float64).float())
    unb = vr * count / (count - 1.0) if count > 1.0 else vr
    if running:
        for name, buf, old, new in (("running_mean", rm, rm0, mr), ("running_var", rv, rv0, unb)):
            t1, t2 = (1.0 - mom) * old, mom * new
            R.within(name, read(buf, torch.float32, (C,)), t1 + t2, 3.0 * 2.0 ** -23 * torch.maximum(t1.abs(), t2.abs()))
    else:
        assert torch.equal(read(rm, torch.float32, (C,)), rm0.float()) and torch.equal(read(rv, torch.float32, (C,)), rv0.float())
    for n, b in (("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rv)):
        guard(b, n)
    return R.finish()


def from_running_case(spec, dev, dtype=None):
    C = 300
    g = gen(41)
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    rm0, rv0 = f32(0.1 * torch.randn(C, generator=g)), f32(0.5 + torch.rand(C, generator=g))
    rm, rv = rm0.float().to(dev), rv0.float().to(dev)
    mean, invstd = Buf(dev, sentinel((C,), torch.float32)), Buf(dev, sentinel((C,), torch.float32))
    launch(None, "sg_bn_from_running", dptr(rm), dptr(rv), C, EPS, mean.ptr(), invstd.ptr())
    ir = 1.0 / torch.sqrt(rv0 + eps)
    R = Report("from_running C=300")
    R.within("mean", read(mean, torch.float32, (C,)), rm0, 0.0)
    R.within("invstd", read(invstd, torch.float32, (C,)), ir, 2.0 ** -23 * ir)
    guard(mean, "mean"), guard(invstd, "invstd")
    return R.finish()


# ---- sg_bn_apply --------------------------------------------------------------------------------------------------------------------------------------------------------
class Variant:
    """sg_bn_apply_variant for the duration; back to what SG_BN_APPLY or the default says afterwards"""

    def __init__(self, variant, workgroups):
        self.v = (variant, workgroups)

    def __enter__(self):
        if self.v[0] is not None:
            _L().call("sg_bn_apply_variant", *self.v)

    def __exit__(self, *a):
        _L().call("sg_bn_apply_variant", -1, 0)


def apply_run(inp, spec, dev, dtype, shift, variant=(None, 0)):
    """-> (counter movement, y's values [N, HW, C] fp64, y's bytes)"""
    N, HW, C = spec["N"], spec["HW"], spec["C"]
    x = Buf(dev, inp["x"].to(dtype), shift.get("x", 0))
    y = Buf(dev, sentinel((N, HW, C), dtype), shift.get("y", 0))
    mean, invstd = stat_dev(inp, dev)
    keep, gp, bp, gsn = affine_dev(inp["aff"], C, dev)
    lib = _L().lib()
    inst = lambda: [lib.sg_bn_path_launches(v) for v in PATHS["apply_stream"].values()]
    with Variant(*variant):
        i0 = inst()
        moved = launch("apply", "sg_bn_apply", _L().dt(dtype), x.ptr(), y.ptr(), N, HW, C, dptr(mean), dptr(invstd), gp, bp, gsn, int(spec.get("relu", 0)))
        i1 = inst()
    ev = os.environ.get("SG_BN_APPLY", "")
    v = variant[0] if variant[0] is not None else (int(ev[0]) if ev[:1] in ("0", "1", "2", "3") else 0)
    assert [b - a for a, b in zip(i0, i1)] == [int(moved["stream"] == 1 and k == v) for k in range(4)], f"a streaming launch of variant {v} counted as {[b - a for a, b in zip(i0, i1)]}"
    got = read(y, dtype, (N, HW, C))
    guard(y, "y")
    return moved, got.double(), raw(y)


def apply_ref(inp, spec, dtype):
    a = inp["aff"]
    xh = (inp["x"] - inp["mean"]) * inp["invstd"]
    ga, bi = a["ga"][:, None, :], a["bi"][:, None, :]
    v = xh * ga + bi
    ref = torch.relu(v) if spec.get("relu") else v
    k = 2 + (a["layout"] not in ("none", "bias")) + (a["layout"] not in ("none", "gain"))       # subtract, multiply, [multiply by the gain], [add the bias]
    bound = k * U * (xh.abs() * ga.abs() + bi.abs())
    if dtype == torch.bfloat16:
        bound = bound + BF16 * ref.abs()
    return ref, bound


# variants of the streaming kernel as (variant, workgroup target): each with 8 workgroups (the unrolled body of every variant runs) and with 2 (one chunk per sample:
# the 8-deep body makes five trips at HW = 700), then once more with the default target
VARIANTS = [(v, w) for w in (8, 2) for v in (0, 1, 2, 3)] + [(3, 0)]


def apply_case(spec, dev, dtype):
    inp = elem_inputs(spec, dtype)
    ref, bound = apply_ref(inp, spec, dtype)
    path = want_path(spec, dtype)
    R = Report(f"apply {DT_ID[dtype]} {spec_id(spec)}")
    moved, got, by = apply_run(inp, spec, dev, dtype, spec.get("shift", {}))
    took(moved, path, "sg_bn_apply")
    R.within("y", got, ref, bound)
    if spec.get("fence"):                                   # the same case with HW on the other side of the gate: the streaming kernel
        s2 = dict(spec, HW=spec["fence"])
        i2 = elem_inputs(s2, dtype)
        m2, g2, _ = apply_run(i2, s2, dev, dtype, {})
        took(m2, "stream", "sg_bn_apply at the fence")
        R.within("y at the fence", g2, *apply_ref(i2, s2, dtype))
    for v in (VARIANTS if spec.get("variants") else []):
        mv, gv, bv = apply_run(inp, spec, dev, dtype, {}, v)
        took(mv, "stream", f"sg_bn_apply variant {v}")
        R.within(f"y variant {v[0]}/{v[1]}", gv, ref, bound)
        same_bytes(bv, by, f"variant {v} of the streaming kernel against the default launch")
    if spec.get("twin") and path != "scalar":             # same tensor 8 bytes further: the scalar kernel, same bytes
        m2, g2, b2 = apply_run(inp, spec, dev, dtype, {"x": 8})
        took(m2, "scalar", "sg_bn_apply on a shifted x")
        R.within("y scalar twin", g2, ref, bound)
        same_bytes(b2, by, f"the scalar kernel against the {path} kernel")
    return R.finish()


# ---- sg_bn_bwd_reduce ---------------------------------------------------------------------------------------------------------------------------------------------------
def masked(inp, spec, rd):
    """(xhat, dy after the ReLU mask, gain, bias) in the torch dtype rd"""
    a = inp["aff"]
    x, dy, mean, invstd = (inp[k].to(rd) for k in ("x", "dy", "mean", "invstd"))
    ga, bi = a["ga"].to(rd)[:, None, :], a["bi"].to(rd)[:, None, :]
    xh = (x - mean) * invstd
    g = torch.where(xh * ga + bi > 0, dy, torch.zeros_like(dy)) if spec.get("relu") else dy
    return xh, g, ga, bi


def reduce_restate(inp, spec, rd):
    xh, g, _, _ = masked(inp, spec, rd)
    return dict(sums=torch.stack([g.sum(1), (g * xh).sum(1)], 2))


def reduce_case(spec, dev, dtype):
    N, HW, C = spec["N"], spec["HW"], spec["C"]
    inp = elem_inputs(spec, dtype, backward=True)
    sh = spec.get("shift", {})
    x, dy = Buf(dev, inp["x"].to(dtype), sh.get("x", 0)), Buf(dev, inp["dy"].to(dtype), sh.get("dy", 0))
    sums = Buf(dev, torch.zeros(N, C, 2, dtype=torch.float32))
    mean, invstd = stat_dev(inp, dev)
    keep, gp, bp, gsn = affine_dev(inp["aff"], C, dev)
    moved = launch("bwd_reduce", "sg_bn_bwd_reduce", _L().dt(dtype), x.ptr(), dy.ptr(), N, HW, C, dptr(mean), dptr(invstd), gp, bp, gsn, int(spec.get("relu", 0)), sums.ptr())
    got = read(sums, torch.float32, (N, C, 2))
    guard(sums, "sums")
    took(moved, want_path(spec, dtype), "sg_bn_bwd_reduce")
    ref = reduce_restate(inp, spec, torch.float64)["sums"]
    b = stage_bounds("reduce", dtype == torch.bfloat16)["sums"][1]
    R = Report(f"bwd_reduce {DT_ID[dtype]} {spec_id(spec)}")
    for k, name in ((0, "sum dy'"), (1, "sum dy' xhat")):
        R.within(name, got[..., k], ref[..., k], measured(ref[..., k], b, False))
    return R.finish()


# ---- sg_bn_bwd_finalize -------------------------------------------------------------------------------------------------------------------------------------------------
def bfin_inputs(spec):
    N, C, lay = spec["N"], 72, spec["layout"]
    g = gen(51 + N)
    a = affine(lay, N, C, g)
    sums = f32(5.0 * torch.randn(N, C, 2, generator=g))
    rows = N if lay != "chan" else 1
    pre = f32(torch.randn(rows, 2 * C, generator=g))                  # [dgain | dbias] before the call: the kernel accumulates
    return dict(aff=a, sums=sums, pre=pre, rows=rows, C=C)


def bfin_restate(inp, spec, rd):
    C = inp["C"]
    s, ga, pre = inp["sums"].to(rd), inp["aff"]["ga"].to(rd), inp["pre"].to(rd)
    chan = torch.stack([(ga * s[..., 0]).sum(0), (ga * s[..., 1]).sum(0)], 1)
    s1, s2 = (s[..., 0].sum(0, keepdim=True), s[..., 1].sum(0, keepdim=True)) if spec["layout"] == "chan" else (s[..., 0], s[..., 1])
    dg = pre[:, :C] + s2 if spec["dgain"] else pre[:, :C]
    db = pre[:, C:] + s1 if spec["dbias"] else pre[:, C:]
    return dict(chan=chan, dgain=dg, dbias=db)


def bfin_case(spec, dev, dtype=None):
    inp = bfin_inputs(spec)
    N, C, lay, rows = spec["N"], inp["C"], spec["layout"], inp["rows"]
    sums = inp["sums"].float().contiguous().to(dev)
    keep, gp, _, gsn = affine_dev(inp["aff"], C, dev)
    chan = Buf(dev, torch.full((2 * C,), float("nan"), dtype=torch.float64))
    if lay == "packed":
        d = Buf(dev, inp["pre"].float())
        dgp, dbp, bufs = d.ptr(), d.ptr() + 4 * C, [d]
    else:
        d1, d2 = Buf(dev, inp["pre"][:, :C].float()), Buf(dev, inp["pre"][:, C:].float())
        dgp, dbp, bufs = d1.ptr(), d2.ptr(), [d1, d2]
    launch(None, "sg_bn_bwd_finalize", dptr(sums), N, C, gp, gsn, dgp if spec["dgain"] else None, dbp if spec["dbias"] else None, chan.ptr())
    if lay == "packed":
        o = read(bufs[0], torch.float32, (rows, 2 * C))
        got_g, got_b = o[:, :C], o[:, C:]
    else:
        got_g, got_b = read(bufs[0], torch.float32, (rows, C)), read(bufs[1], torch.float32, (rows, C))
    ref = bfin_restate(inp, spec, torch.float64)
    bd = stage_bounds("bwd_finalize", False)
    R = Report(f"bwd_finalize {spec_id(spec)}")
    R.within("chan", read(chan, torch.float64, (C, 2)), ref["chan"], measured(ref["chan"], bd["chan"][1], False))
    for name, got, on in (("dgain", got_g, spec["dgain"]), ("dbias", got_b, spec["dbias"])):
        if on:
            R.within(name, got, ref[name], measured(ref[name], bd[name][1], False))
        else:
            assert torch.equal(got.double(), ref[name]), f"{name} is null and its neighbour's rows were written"
    for b in bufs + [chan]:
        guard(b, "bwd_finalize output")
    return R.finish()


# ---- sg_bn_bwd_apply / sg_bn_bwd_apply_res -------------------------------------------------------------------------------------------------------------------------------
def bapply_restate(inp, spec, rd):
    xh, g, ga, _ = masked(inp, spec, rd)
    d = ga * g
    if spec.get("use_batch"):
        ch = inp["chan"].to(rd)
        d = d - (ch[:, 0] + xh * ch[:, 1]) * (1.0 / inp["count"])
    d = d * inp["invstd"].to(rd)
    if spec.get("res"):
        d = d + inp["res"].to(rd)
    return dict(dx=d)


def bapply_run(inp, spec, dev, dtype, shift):
    N, HW, C = spec["N"], spec["HW"], spec["C"]
    x, dy = Buf(dev, inp["x"].to(dtype), shift.get("x", 0)), Buf(dev, inp["dy"].to(dtype), shift.get("dy", 0))
    dx = Buf(dev, sentinel((N, HW, C), dtype), shift.get("dx", 0))
    res = Buf(dev, inp["res"].to(dtype)) if spec.get("res") else None
    mean, invstd = stat_dev(inp, dev)
    chan = inp["chan"].contiguous().to(dev)
    keep, gp, bp, gsn = affine_dev(inp["aff"], C, dev)
    args = [_L().dt(dtype), x.ptr(), dy.ptr(), dx.ptr(), N, HW, C, dptr(mean), dptr(invstd), gp, bp, gsn, int(spec.get("relu", 0)), dptr(chan), inp["count"],
            int(spec.get("use_batch", 0))]
    if res is None and not spec.get("null_res"):
        moved = launch("bwd_apply", "sg_bn_bwd_apply", *args)
    else:
        moved = launch("bwd_apply", "sg_bn_bwd_apply_res", *args, res.ptr() if res else None)
    got = read(dx, dtype, (N, HW, C))
    guard(dx, "dx")
    return moved, got.double(), raw(dx)


def bapply_case(spec, dev, dtype):
    inp = elem_inputs(spec, dtype, backward=True)
    path = want_path(spec, dtype)
    ref = bapply_restate(inp, spec, torch.float64)["dx"]
    bound = measured(ref, stage_bounds("bwd_apply", dtype == torch.bfloat16)["dx"][1], dtype == torch.bfloat16)
    R = Report(f"bwd_apply {DT_ID[dtype]} {spec_id(spec)}")
    moved, got, by = bapply_run(inp, spec, dev, dtype, spec.get("shift", {}))
    took(moved, path, "sg_bn_bwd_apply")
    R.within("dx", got, ref, bound)
    if spec.get("twin") and path != "scalar":
        for sh in ({"x": 8}, {"dx": 8}):                  # the scalar kernel, also when only dx is misaligned: same bytes
            m2, g2, b2 = bapply_run(inp, spec, dev, dtype, sh)
            took(m2, "scalar", f"sg_bn_bwd_apply shifted by {sh}")
            R.within(f"dx scalar twin {list(sh)[0]}", g2, ref, bound)
            same_bytes(b2, by, f"the scalar kernel ({list(sh)[0]} shifted) against the {path} kernel")
    return R.finish()


# ---- measured bounds of the backward stages -----------------------------------------------------------------------------------------------------------------------------
STAGES = {"reduce": (reduce_case, reduce_restate, lambda s, dt: elem_inputs(s, dt, backward=True), True),
          "bwd_finalize": (bfin_case, bfin_restate, lambda s, dt: bfin_inputs(s), False),
          "bwd_apply": (bapply_case, bapply_restate, lambda s, dt: elem_inputs(s, dt, backward=True), True)}


@functools.lru_cache(maxsize=None)
def stage_bounds(stage, bf16):
    """torch fp32 against torch fp64 on the inputs of every case of the stage -> {output: (measured, bound)}"""
    fn, restate, inputs, per_dtype = STAGES[stage]
    dtype = torch.bfloat16 if bf16 else torch.float32
    worst = {}
    for c in CASES:
        if c[0] is fn:
            inp = inputs(c[1], dtype)
            o64, o32 = restate(inp, c[1], torch.float64), restate(inp, c[1], torch.float32)
            for k in o64:
                worst[k] = max(worst.get(k, 0.0), rel(o32[k], o64[k]))
    return {k: (v, max(MARGIN * v, FLOOR)) for k, v in worst.items()}


# ---- the ReLU mask: forward and backward, element for element ----------------------------------------------------------------------------------------------------------
def mask_inputs(spec, dtype):
    """random data with >= 256 planted elements whose pre-activation lies within a few fp32 ulps of zero: x = round(mean - bias / (gain invstd)) + k ulp, k in [-8, 8].
    Checked here, before any device call: under both fp32 evaluations of ((x - mean) invstd) gain + bias (multiply then add; one fused multiply-add, which is the
    fp64 evaluation of the last step rounded once, exact for fp32 operands) at least a quarter of the planted elements are positive and at least a quarter are not,
    and the two evaluations disagree on at least one."""
    N, HW, C = spec["N"], spec["HW"], spec["C"]
    inp = elem_inputs(dict(spec, layout="sample", relu=0), dtype, backward=True)
    g = gen(77 + HW + C)
    x, mean, invstd = inp["x"].clone(), inp["mean"], inp["invstd"]
    ga, bi = inp["aff"]["ga"][:, None, :].expand(N, HW, C), inp["aff"]["bi"][:, None, :].expand(N, HW, C)
    n_plant = max(256, (N * HW * C) // 4)
    zero = (mean - bi / (ga * invstd)).reshape(-1)
    ok = torch.nonzero(zero.abs() > 1e-2).reshape(-1)                   # (k ulps of a value that close to zero would be nothing)
    at = ok[torch.randperm(ok.numel(), generator=g)[:n_plant]]
    assert at.numel() == n_plant
    k = torch.randint(-8, 9, (n_plant,), generator=g)
    x0 = zero[at].to(dtype)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    bits = x0.view(it).clone()
    bits = torch.where(x0 >= 0, bits + k.to(it), bits - k.to(it))       # k ulps up or down (no planted value is within 8 ulps of zero: asserted)
    assert float(x0.double().abs().min()) > 1e-3
    x.view(-1)[at] = bits.view(dtype).double()
    dy = inp["dy"]
    dy = q(torch.where(dy.abs() < 2.0 ** -10, torch.full_like(dy, 0.5), dy), dtype)
    assert float(dy.abs().min()) >= 2.0 ** -10 and float(inp["aff"]["ga"].abs().min()) >= 0.3
    inp.update(x=x, dy=dy, u=dy.flip(0))
    xs, m32, i32, g32, b32 = (t.float() for t in (x, mean, invstd, ga, bi))
    t = ((xs - m32) * i32)
    unfused = (t * g32 + b32).reshape(-1)[at] > 0
    fused = (t.double() * g32.double() + b32.double()).reshape(-1)[at] > 0
    for name, m in (("multiply then add", unfused), ("fused multiply-add", fused)):
        f = float(m.float().mean())
        assert 0.25 <= f <= 0.75, f"{name}: {f:.2f} of the planted elements are positive"
    if dtype == torch.float32:          # (a bf16 x cannot sit within fp32 ulps of the zero of its pre-activation: there the plant probes the mask at bf16 spacing)
        assert bool((fused != unfused).any()), "the two evaluations agree on every planted element: the plant cannot see a contraction difference"
    inp["at"] = at
    return inp


def mask_case(spec, dev, dtype):
    """running statistics, no residual: dx / g_dy is exactly 0 where y is 0 and non-zero where y > 0, on every path the shape reaches"""
    N, HW, C = spec["N"], spec["HW"], spec["C"]
    inp = mask_inputs(spec, dtype)
    main = "stream" if HW >= 16 else "vec"
    s = dict(spec, relu=1, use_batch=0, layout="sample")
    ys = {}
    for name, sh in ((main, {}), ("scalar", {"x": 8})):
        moved, y, _ = apply_run(inp, s, dev, dtype, sh)
        took(moved, name, "sg_bn_apply")
        ys[name] = y
    on = ys[main] > 0
    assert torch.equal(on, ys["scalar"] > 0), "the forward kernels disagree on the mask"
    planted = on.reshape(-1)[inp["at"]]
    assert bool(planted.any()) and not bool(planted.all()), "the planted elements all fell on one side"
    outs = {}
    for name, sh in ((main, {}), ("scalar", {"dx": 8})):
        moved, dx, _ = bapply_run(inp, s, dev, dtype, sh)
        took(moved, name, "sg_bn_bwd_apply")
        outs["bwd_apply " + name] = dx
    # the second-order passes' g_dy, use_batch = 0, A = B = 0: mask * gain invstd u
    mean, invstd = stat_dev(inp, dev)
    keep, gp, bp, gsn = affine_dev(inp["aff"], C, dev)
    chan7 = torch.zeros(7 * C, dtype=torch.float64).to(dev)
    for name, sh in (("vec", 0), ("scalar", 8)):
        x, dy, u = Buf(dev, inp["x"].to(dtype), sh), Buf(dev, inp["dy"].to(dtype)), Buf(dev, inp["u"].to(dtype))
        gd = Buf(dev, sentinel((N, HW, C), dtype))
        moved = launch("cbn_bwd2_apply", "sg_cbn_bwd2_apply", _L().dt(dtype), x.ptr(), dy.ptr(), u.ptr(), gd.ptr(), None, N, HW, C, dptr(mean), dptr(invstd), gp, bp,
                       None, None, gsn, 1, dptr(chan7), inp["count"], 0)
        took(moved, name, "sg_cbn_bwd2_apply")
        outs["cbn_bwd2_apply " + name] = read(gd, dtype, (N, HW, C)).double()
        guard(gd, "g_dy")
    # the per-channel pass has per-channel rows: sample 0's rows for every sample, the forward again with them
    a0 = dict(inp["aff"], layout="chan", rows=1, ga=inp["aff"]["ga"][:1].expand(N, C).clone(), bi=inp["aff"]["bi"][:1].expand(N, C).clone())
    inp0 = dict(inp, aff=a0)
    _, y0, _ = apply_run(inp0, dict(s, layout="chan"), dev, dtype, {})
    keep0, gp0, bp0, _ = affine_dev(a0, C, dev)
    x, dy, u = Buf(dev, inp["x"].to(dtype)), Buf(dev, inp["dy"].to(dtype)), Buf(dev, inp["u"].to(dtype))
    gd = Buf(dev, sentinel((N, HW, C), dtype))
    chan5 = torch.zeros(5 * C, dtype=torch.float64).to(dev)
    launch(None, "sg_bn_bwd2_apply", _L().dt(dtype), x.ptr(), dy.ptr(), u.ptr(), gd.ptr(), None, N, HW, C, dptr(mean), dptr(invstd), gp0, bp0, 1, dptr(chan5), inp["count"], 0)
    g0 = read(gd, dtype, (N, HW, C)).double()
    guard(gd, "g_dy")
    assert torch.equal(g0 != 0, y0 > 0), f"sg_bn_bwd2_apply: g_dy's mask differs from the forward's at {int(((g0 != 0) != (y0 > 0)).sum())} elements"
    for name, o in outs.items():
        assert torch.equal(o != 0, on), f"{name}: the mask differs from the forward's at {int(((o != 0) != on).sum())} elements"
    print(f"[mask {DT_ID[dtype]} {spec_id(spec)}] {int(planted.sum())} of {planted.numel()} planted elements pass the ReLU; {len(outs) + 1} backward outputs agree")


# ---- second-order stage 1: one kernel for per-channel vectors (row pitch 0) and per-sample rows ------------------------------------------------------------------------
def bwd2_pitch_case(spec, dev, dtype):
    """sg_bn_bwd2_reduce on gain[C] / bias[C] and sg_cbn_bwd2_reduce on rows that repeat those values for every sample, at pitch C and at the packed pitch 2 C, write
    the SAME BYTES into sums[N][C][5]. At these sizes one block adds into each address (HW <= 16: one row group), so the result does not depend on atomic order"""
    N, HW, C = spec["N"], spec["HW"], spec["C"]
    assert HW <= 16
    inp = elem_inputs(dict(spec, layout="chan", relu=1), dtype, backward=True)
    ga, bi = inp["aff"]["ga"], inp["aff"]["bi"]
    assert torch.equal(ga, ga[:1].expand(N, C)) and torch.equal(bi, bi[:1].expand(N, C))
    u = q(torch.randn(N, HW, C, generator=gen(91 + C), dtype=torch.float64), dtype)
    x, dy, ud = (Buf(dev, t.to(dtype)) for t in (inp["x"], inp["dy"], u))
    mean, invstd = stat_dev(inp, dev)
    vec = [ga[0].float().contiguous().to(dev), bi[0].float().contiguous().to(dev)]
    rows = [ga.float().contiguous().to(dev), bi.float().contiguous().to(dev)]
    packed = torch.cat([ga, bi], 1).float().contiguous().to(dev)

    def run(name, gp, bp, *pitch):
        sums = Buf(dev, torch.zeros(N, C, 5, dtype=torch.float32))
        launch(None, name, _L().dt(dtype), x.ptr(), dy.ptr(), ud.ptr(), N, HW, C, dptr(mean), dptr(invstd), gp, bp, *pitch, 1, sums.ptr())
        guard(sums, name)
        return raw(sums), read(sums, torch.float32, (N, C, 5))

    by, got = run("sg_bn_bwd2_reduce", dptr(vec[0]), dptr(vec[1]))
    xh, g, _, _ = masked(inp, dict(relu=1), torch.float64)
    assert bool((g == 0).any()) and bool((g != 0).any()), "the ReLU masks nothing or everything: the rows would not matter"
    assert bool((got[..., 0] != 0).all()) and rel(got[..., 3], (g * xh).sum(1)) < 1e-2, "sums were not written"      # (a sanity line; the check is the bytes)
    same_bytes(run("sg_cbn_bwd2_reduce", dptr(rows[0]), dptr(rows[1]), C)[0], by, "sg_cbn_bwd2_reduce on repeated rows of pitch C against sg_bn_bwd2_reduce")
    same_bytes(run("sg_cbn_bwd2_reduce", dptr(packed), dptr(packed) + 4 * C, 2 * C)[0], by, "sg_cbn_bwd2_reduce on repeated packed rows of pitch 2 C against sg_bn_bwd2_reduce")
    print(f"[bwd2_pitch {DT_ID[dtype]} {spec_id(spec)}] {by.numel()} bytes of sums equal at row pitch 0, C and 2 C; {int((g == 0).sum())} of {g.numel()} elements masked")


# ---- end to end against the fp64 oracle ---------------------------------------------------------------------------------------------------------------------------------
ROWS_SHAPES = [(19, 2, 2, 72), (37, 3, 2, 8), (2, 48, 47, 8)]      # N beyond the first trip of both finalize kernels (16 / 4 sample groups); 4512 rows: the streaming statistics kernel
CHAN_SHAPES = [(2, 40, 40, 8), (19, 3, 3, 6)]
CHAN_GRID = ((1, 1), (0, 1), (1, 0))
E2E_OUT = ("y", "dx", "dgam", "dbet", "g_dy", "g_x", "g_gam")
BF16_OUT = ("y", "dx", "g_dy", "g_x")


def e2e_inputs(kind, shape, relu, ub, bf16):
    import logan_cbn_checks as LC
    seed = 7000 + 97 * (ROWS_SHAPES + CHAN_SHAPES).index(shape) + 2 * relu + ub
    return LC.bn_inputs(shape, relu, ub, seed, bf16=bf16, **(dict(equal_rows=True, zero_ab=True) if kind == "chan" else {}))


def e2e_oracle(inp, relu, ub, rd):
    """logan_cbn_checks.bn_oracle plus the forward's output"""
    import logan_cbn_checks as LC
    o = LC.bn_oracle(inp, relu, ub, rd)
    c = {k: v.to(rd) for k, v in inp.items()}
    x = c["x"]
    mean, var = (x.mean((0, 1, 2)), ((x - x.mean((0, 1, 2))) ** 2).mean((0, 1, 2))) if ub else (c["rm"], c["rv"])
    y = (x - mean) / torch.sqrt(var + EPS) * c["gam"][:, None, None, :] + c["bet"][:, None, None, :]
    o["y"] = torch.relu(y) if relu else y
    return o


def e2e_cases(kind):
    if kind == "rows":
        return [(s, relu, ub) for s in ROWS_SHAPES for relu in (0, 1) for ub in (0, 1)]
    return [(s, relu, ub) for s in CHAN_SHAPES for relu, ub in CHAN_GRID]


@functools.lru_cache(maxsize=None)
def e2e_bounds(kind, bf16):
    worst = dict.fromkeys(E2E_OUT, 0.0)
    for shape, relu, ub in e2e_cases(kind):
        inp = e2e_inputs(kind, shape, relu, ub, bf16)
        o64, o32 = e2e_oracle(inp, relu, ub, torch.float64), e2e_oracle(inp, relu, ub, torch.float32)
        for k in worst:
            a, b = (o32[k].sum(0), o64[k].sum(0)) if (kind == "chan" and k == "g_gam") else (o32[k], o64[k])
            if float(b.abs().max()) > 0.0:
                worst[k] = max(worst[k], rel(a, b))
    return {k: (v, max(MARGIN * v, FLOOR)) for k, v in worst.items()}


def _compare(R, got, ref, bounds, bf16, keys):
    for k in keys:
        r = ref[k].double()
        if float(r.abs().max()) == 0.0:
            R.within(k + " (zero)", got[k].detach().cpu(), r, 0.0)
        else:
            R.within(k, got[k].detach().cpu(), r, measured(r, bounds[k][1], bf16 and k in BF16_OUT))


def forward_y(inp, relu, ub, dev, bf16, per_channel=False):
    from studiogan_amd import functional as F
    dt = torch.bfloat16 if bf16 else torch.float32
    cfg = F.BNCfg(bool(ub), False, EPS, 0.1, bool(relu), None)
    gam, bet = (inp["gam"][0], inp["bet"][0]) if per_channel else (inp["gam"], inp["bet"])
    with torch.no_grad():
        return F.BNFn.apply(inp["x"].to(dt).to(dev), gam.float().to(dev), bet.float().to(dev), inp["rm"].float().to(dev), inp["rv"].float().to(dev), cfg)


def e2e_rows_case(spec, dev, dtype):
    """functional.BNFn with per-sample rows: forward, backward and double backward (logan_cbn_checks.bn_product, unchanged) against the fp64 oracle"""
    import logan_cbn_checks as LC
    shape, relu, ub, packed = spec["shape"], spec["relu"], spec["ub"], spec["packed"]
    bf16 = dtype == torch.bfloat16
    inp = e2e_inputs("rows", shape, relu, ub, bf16)
    o = e2e_oracle(inp, relu, ub, torch.float64)
    lib = _L().lib()
    n0 = [lib.sg_bn_path_launches(PATHS["partial"][k]) for k in ("generic", "stream")]
    p = LC.bn_product(inp, relu, ub, packed, dev, bf16)
    n1 = [lib.sg_bn_path_launches(PATHS["partial"][k]) for k in ("generic", "stream")]
    N, H, W, C = shape
    stream = N * H * W >= 4096 and C % V(dtype) == 0
    assert [b - a for a, b in zip(n0, n1)] == ([0, 0] if not ub else [0, 1] if stream else [1, 0]), "the statistics took another kernel than the shape says"
    p["y"] = forward_y(inp, relu, ub, dev, bf16)
    R = Report(f"rows {DT_ID[dtype]} {spec_id(spec)}")
    _compare(R, p, o, e2e_bounds("rows", bf16), bf16, E2E_OUT)
    return R.finish()


def e2e_chan_case(spec, dev, dtype):
    """the per-channel second-order pass (BNFn with [C] gain / bias -> BNBwdFn) against the oracle with equal rows and A = B = 0, g_gam summed over the rows.
    drop = "dy" / "x": that tensor does not require grad (the null g_dy / g_x branch of sg_bn_bwd2_apply)"""
    from studiogan_amd import functional as F
    shape, relu, ub, drop = spec["shape"], spec["relu"], spec["ub"], spec.get("drop")
    bf16 = dtype == torch.bfloat16
    dt = dtype
    inp = e2e_inputs("chan", shape, relu, ub, bf16)
    o = e2e_oracle(inp, relu, ub, torch.float64)
    o["g_gam"] = o["g_gam"].sum(0)
    N, H, W, C = shape
    x = inp["x"].to(dt).to(dev).requires_grad_(drop != "x")
    dy = inp["dy"].to(dt).to(dev).requires_grad_(drop != "dy")
    u = inp["u"].to(dt).to(dev)
    gam, bet = inp["gam"][0].float().to(dev).requires_grad_(True), inp["bet"][0].float().to(dev)
    rm, rv = inp["rm"].float().to(dev), inp["rv"].float().to(dev)
    cfg = F.BNCfg(bool(ub), False, EPS, 0.1, bool(relu), None)
    L = _L()
    if drop == "x":
        # x needs no gradient: BNFn's backward would not be asked for dx, so the operator is called on its own with the statistics of the library
        mean, invstd = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
        if ub:
            part = torch.zeros(2 * C, dtype=torch.float64, device=dev)
            L.call("sg_bn_partial_stats", L.dt(dt), L.ptr(x), C, N * H * W, C, L.ptr(part), L.stream())
            L.call("sg_bn_finalize", L.ptr(part), float(N * H * W), C, EPS, 0.1, L.ptr(mean), L.ptr(invstd), None, None, L.stream())
        else:
            L.call("sg_bn_from_running", L.ptr(rm), L.ptr(rv), C, EPS, L.ptr(mean), L.ptr(invstd), L.stream())
        dx = F.BNBwdFn.apply(dy, x, gam, bet, mean, invstd, cfg, float(N * H * W))
    else:
        y = F.BNFn.apply(x, gam, bet, rm, rv, cfg)
        (dx,) = torch.autograd.grad(y, (x,), dy, create_graph=True)
    want = [t for t in (dy, x, gam) if t.requires_grad]
    gr = dict(zip([id(t) for t in want], torch.autograd.grad((u.float() * dx.float()).sum(), want, allow_unused=True)))
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    p = dict(dx=dx.detach(), g_gam=z(gr[id(gam)], gam), y=forward_y(inp, relu, ub, dev, bf16, per_channel=True))
    keys = ["y", "dx", "g_gam"]
    if drop != "dy":
        p["g_dy"] = z(gr[id(dy)], dy)
        keys.append("g_dy")
    if drop != "x":
        p["g_x"] = z(gr[id(x)], x)
        keys.append("g_x")
    R = Report(f"chan {DT_ID[dtype]} {spec_id(spec)}")
    _compare(R, p, o, e2e_bounds("chan", bf16), bf16, keys)
    return R.finish()


# ---- the case table: (check, spec, runs in both dtypes, GPU only) ------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    add = lambda fn, spec, both=True, gpu_only=False: out.append((fn, spec, both, gpu_only))
    # statistics
    add(partial_case, dict(rows=150, C=72, path="generic"))                      # three row groups, second channel tile with an 8-wide tail
    add(partial_case, dict(rows=70, C=6, path="generic"))
    add(partial_case, dict(rows=4418, C=64, ldx=65, path="generic"))             # the pitch breaks the vector predicate above the row threshold
    add(partial_case, dict(rows=4418, C=64, shift={"x": 8}, path="generic"))            # x 8 bytes off a 16-byte boundary
    add(partial_case, dict(rows=4095, C=64, path="generic"))                     # one row below the threshold
    add(partial_case, dict(rows=4096, C=64, path="stream"))
    add(partial_case, dict(rows=4097, C=64, path="stream"))                      # a last block of ONE row: the row a lane starts at is the last of its chunk
    add(partial_case, dict(rows=4418, C=64, path="stream"))
    add(partial_case, dict(rows=4418, C=40, path={"bf16": "stream", "fp32": "stream"}))      # bf16: CV = 5, a 255-thread block
    add(partial_case, dict(rows=4418, C=24, path="stream"))                      # fp32: CV = 6, a 252-thread block
    add(partial_case, dict(rows=4418, C=8, path="stream"))                       # one block, the early break
    add(partial_case, dict(rows=4418, C=64, pitch_v=1, path="stream"))           # pitched, ldx = C + V
    add(partial_case, dict(rows=4096, C=1024, path={"bf16": "stream", "fp32": "generic"}))      # the CV = 128 fence (bf16)
    add(partial_case, dict(rows=4096, C=1032, path="generic"))
    for count, running in ((4418, True), (4418, False), (1, True)):
        add(finalize_case, dict(count=count, running=running), both=False)
    add(from_running_case, dict(), both=False)
    # sg_bn_apply: every path's first shape in every affine layout, with and without the ReLU
    first = {"stream": dict(N=4, HW=36, C=24), "vec": dict(N=3, HW=15, C=72), "scalar": dict(N=3, HW=15, C=6)}
    for path, shp in first.items():
        for lay in LAYOUTS:
            for relu in (0, 1):
                add(apply_case, dict(shp, layout=lay, relu=relu, path=path, twin=(lay == "sample")))
    add(apply_case, dict(N=2, HW=700, C=64, relu=1, path="stream", twin=1))      # unrolled body, several chunks, ragged last chunk
    add(apply_case, dict(N=2, HW=700, C=128, relu=1, path="stream", variants=1, twin=1))      # bf16: the 8-deep body of variants 1 and 3
    add(apply_case, dict(N=2, HW=700, C=64, relu=0, path="stream", variants=1, twin=1))       # fp32: the same
    add(apply_case, dict(N=3, HW=9, C=16, relu=1, path="vec", fence=16, twin=1))
    add(apply_case, dict(N=1, HW=9, C=2056, relu=1, path={"bf16": "vec", "fp32": "vec"}, twin=1))       # bf16: CV = 257
    add(apply_case, dict(N=1, HW=16, C=2056, relu=1, path={"bf16": "vec", "fp32": "vec"}, twin=1))      # CV > 256 alone keeps it off the streaming kernel
    add(apply_case, dict(N=1, HW=16, C=1028, relu=1, path={"bf16": "scalar", "fp32": "vec"}, twin=1))   # fp32: CV = 257
    add(apply_case, dict(N=1, HW=16, C=2048, relu=1, path={"bf16": "stream", "fp32": "vec"}))           # bf16: CV = 256, the last streaming width
    add(apply_case, dict(N=3, HW=9, C=20, relu=1, path={"bf16": "scalar", "fp32": "vec"}))
    add(apply_case, dict(N=2, HW=20, C=20, relu=1, path={"bf16": "scalar", "fp32": "stream"}))
    for sh in ({"x": 8}, {"y": 8}, {"x": -1}, {"y": -1}):                        # -1: one element
        add(apply_case, dict(N=4, HW=36, C=24, relu=1, path="scalar", shift=sh))
    # sg_bn_bwd_reduce: the same path-selecting shapes
    for relu in (0, 1):
        add(reduce_case, dict(N=4, HW=36, C=24, relu=relu, path="stream"))      # a block that has only a tail
        add(reduce_case, dict(N=3, HW=15, C=72, relu=relu, path="generic"))
        add(reduce_case, dict(N=3, HW=15, C=6, relu=relu, path="generic"))
    add(reduce_case, dict(N=2, HW=700, C=64, relu=1, path="stream"))             # the floor of two unrolled trips per block (ppb = 8 lanes), ragged last chunk
    add(reduce_case, dict(N=2, HW=700, C=128, relu=1, layout="packed", path="stream"))
    add(reduce_case, dict(N=3, HW=16, C=16, relu=1, layout="chan", path="stream"))
    add(reduce_case, dict(N=3, HW=9, C=16, relu=1, layout="chan", path="generic"))
    add(reduce_case, dict(N=1, HW=16, C=2056, relu=1, path={"bf16": "generic", "fp32": "generic"}))
    add(reduce_case, dict(N=2, HW=20, C=20, relu=1, path={"bf16": "generic", "fp32": "stream"}))
    add(reduce_case, dict(N=2, HW=150, C=72, relu=1, shift={"x": 8}, layout="none", path="generic"))      # generic kernel, several row groups, a second channel tile
    add(reduce_case, dict(N=4, HW=36, C=24, relu=1, shift={"dy": 8}, path="generic"))
    # sg_bn_bwd_finalize
    for N in (1, 4, 19, 37):
        for lay in ("chan", "sample", "packed"):
            add(bfin_case, dict(N=N, layout=lay, dgain=1, dbias=1), both=False)
    for lay in ("chan", "sample", "packed"):
        for dg, db in ((1, 0), (0, 1), (0, 0)):
            add(bfin_case, dict(N=19, layout=lay, dgain=dg, dbias=db), both=False)
    # sg_bn_bwd_apply / _res
    for path, shp in first.items():
        for ub in (0, 1):
            for relu in (0, 1):
                for res in (0, 1):
                    add(bapply_case, dict(shp, use_batch=ub, relu=relu, res=res, path=path, twin=(ub == relu)))
    add(bapply_case, dict(N=2, HW=700, C=64, use_batch=1, relu=1, res=1, layout="packed", path="stream", twin=1))
    add(bapply_case, dict(N=2, HW=700, C=128, use_batch=1, relu=1, res=0, null_res=1, layout="chan", path="stream", twin=1))
    add(bapply_case, dict(N=3, HW=9, C=16, use_batch=1, relu=1, res=1, layout="none", path="vec", twin=1))
    add(bapply_case, dict(N=3, HW=16, C=16, use_batch=1, relu=1, res=1, layout="gain", path="stream", twin=1))
    add(bapply_case, dict(N=1, HW=16, C=2056, use_batch=1, relu=1, res=1, path={"bf16": "vec", "fp32": "vec"}, twin=1))
    add(bapply_case, dict(N=1, HW=16, C=1028, use_batch=1, relu=1, res=1, path={"bf16": "scalar", "fp32": "vec"}, twin=1))
    add(bapply_case, dict(N=2, HW=20, C=20, use_batch=1, relu=1, res=1, path={"bf16": "scalar", "fp32": "stream"}))
    for sh in ({"x": 8}, {"dy": 8}, {"dx": 8}, {"dx": -1}):
        add(bapply_case, dict(N=4, HW=36, C=24, use_batch=1, relu=1, res=1, path="scalar", shift=sh))
    # second-order stage 1: the per-channel entry point is the per-sample kernel at row pitch 0
    add(bwd2_pitch_case, dict(N=3, HW=15, C=72))                                 # a second channel tile with an 8-wide tail
    add(bwd2_pitch_case, dict(N=3, HW=15, C=6))
    # the ReLU mask on every path
    add(mask_case, dict(N=4, HW=36, C=24))
    add(mask_case, dict(N=3, HW=15, C=72))
    # end to end
    for shape, relu, ub in e2e_cases("rows"):
        add(e2e_rows_case, dict(shape=shape, relu=relu, ub=ub, packed=(relu == ub)))
    for shape, relu, ub in e2e_cases("chan"):
        add(e2e_chan_case, dict(shape=shape, relu=relu, ub=ub))
    for drop in ("dy", "x"):
        add(e2e_chan_case, dict(shape=CHAN_SHAPES[0], relu=1, ub=1, drop=drop))
        add(e2e_chan_case, dict(shape=CHAN_SHAPES[1], relu=1, ub=1, drop=drop))
    return out


def spec_id(spec):
    def one(k, v):
        if k == "path":
            return "->" + (v if isinstance(v, str) else "/".join(f"{a}:{b}" for a, b in v.items()))
        if k == "shift":
            return " ".join(f"{a}{'+8B' if b == 8 else '+1el'}" for a, b in v.items())
        if k == "shape":
            return "x".join(str(s) for s in v)
        return f"{k}={v}"
    return " ".join(one(k, v) for k, v in spec.items() if k not in ("seed", "twin"))


CASES = _cases()
ENTRY_OF = {partial_case: "partial", apply_case: "apply", reduce_case: "bwd_reduce", bapply_case: "bwd_apply"}


def params(gpu):
    """(case, dtype) pairs of one place: the interpreter leaves out the cases marked GPU only"""
    out = []
    for c in CASES:
        if c[3] and not gpu:
            continue
        for dt in (DTYPES if c[2] else (torch.float32,)):
            out.append((c, dt))
    return out


def param_id(p):
    (fn, spec, both, _), dt = p
    return f"{fn.__name__[:-5]} {spec_id(spec)}" + (f" {DT_ID[dt]}" if both else "")


def paths_in_table(gpu=True):
    """{entry: set of kernels some case of the table expects}; the mask cases name theirs in mask_case"""
    seen = {e: set() for e in PATHS}
    for (fn, spec, both, gpu_only), dt in params(gpu):
        if fn in ENTRY_OF:
            seen[ENTRY_OF[fn]].add(want_path(spec, dt))
        if fn is apply_case and want_path(spec, dt) == "stream":
            seen["apply_stream"].add("v0")
        if spec.get("variants"):
            seen["apply_stream"] |= {f"v{v}" for v, _ in VARIANTS}
        if fn is mask_case:
            main = "stream" if spec["HW"] >= 16 else "vec"
            seen["apply"] |= {main, "scalar"}
            seen["bwd_apply"] |= {main, "scalar"}
            seen["cbn_bwd2_apply"] |= {"vec", "scalar"}
    return seen


def run_case(case, dev, dtype):
    fn, spec = case[0], dict(case[1])
    if "shift" in spec:                                   # -1: one element of the dtype
        spec["shift"] = {k: (v if v > 0 else (2 if dtype == torch.bfloat16 else 4)) for k, v in spec["shift"].items()}
    return fn(spec, dev, dtype)


# ---- profiles/bn_bounds.txt -------------------------------------------------------------------------------------------------------------------------------------------
def write_bounds(path, gpu_log=None):
    """the measured reference-side errors and the bounds they give; gpu_log: the printed output of one GPU run of tests/test_bn_gpu.py, whose per-output errors are
    recorded next to them (the largest per check and output)"""
    import platform
    lines = ["Bounds of tests/bn_checks.py that are MEASURED on the reference side: torch in fp32 on the CPU against torch in fp64 on the same inputs, per output, max-abs",
             "error over the tensor's max-abs, the largest over the cases of the check. bound = max(4 x measured, 1e-6); bf16 tensors (y, dx, g_dy, g_x): 2^-8 |ref| per",
             "element plus that bound times max|ref|. The statistics, finalize and apply bounds are derived, not measured (module docstring).",
             f"torch {torch.__version__}, {platform.machine()}; python tests/bn_checks.py [log of a GPU run] writes this file.", ""]
    tabs = [(f"{st} ({'bf16' if bf else 'fp32'} inputs)", stage_bounds(st, bf)) for st in STAGES for bf in ((False, True) if STAGES[st][3] else (False,))]
    tabs += [(f"end to end, {'per-sample rows' if kind == 'rows' else 'per-channel pass'} ({'bf16-rounded x / dy / u' if bf else 'fp32 inputs'})", e2e_bounds(kind, bf))
             for kind in ("rows", "chan") for bf in (False, True)]
    for name, b in tabs:
        lines.append(name)
        for k, (m, bd) in b.items():
            lines.append(f"    {k:10s} measured {m:.3e}   bound {bd:.3e}")
        lines.append("")
    if gpu_log:
        worst = {}
        for m in re.finditer(r"\[(\S+) (fp32|bf16)?[^\]]*\] (.+?)\s+err (\S+) of range, (\S+) of its bound", open(gpu_log).read()):
            key = (m.group(1), m.group(2) or "fp32", re.sub(r" variant.*| scalar twin.*| at the fence", "", m.group(3)).strip())
            e, o = float(m.group(4)), float(m.group(5))
            w = worst.get(key, (0.0, 0.0))
            worst[key] = (max(w[0], e), max(w[1], o))
        lines += ["One run on an MI355X (tests/test_bn_gpu.py): the largest error per check, dtype and output, as max-abs error over the reference's max-abs, and as a",
                  "fraction of the bound of the element where that fraction is largest.", ""]
        for (chk, dt, out), (e, o) in sorted(worst.items()):
            lines.append(f"    {chk:14s} {dt}  {out:16s} error {e:.3e} of range   {o:.3e} of its bound")
        lines.append("")
    open(path, "w").write("\n".join(lines))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    write_bounds(os.path.join(ROOT, "profiles", "bn_bounds.txt"), sys.argv[1] if len(sys.argv) > 1 else None)
