"""Checks of the second-order pass through a CONDITIONAL batch norm (latent optimisation -- LOGAN -- on class-conditional generators), written once for both places
they run: the GPU (tests/test_logan_cbn_gpu.py) and the kernel sources on the CPU interpreter (tests/test_logan_cbn_cpu.py under hipemu.fullemu.Installed).

Bounds. The oracle is torch autograd's double backward in fp64 on the CPU. The fp32 bound of the operator-level checks is MEASURED on the reference side, never on the
code under test: the same double backward evaluated by torch in fp32 on the CPU against the fp64 oracle, per output, as max-abs error over the tensor's max-abs, the
largest over the cases of a check; the product is allowed 4x that (the atomics' summation order against torch's) with a floor of 1e-6. The values of one run and the
bounds they give are recorded in profiles/logan_cbn_bounds.txt; the checks compute them again on the CPU each time (cached per process), so they hold for the
torch build at hand. bf16 tensors: 2^-8 of the tensor's max-abs (one bf16 rounding of the result plus the fp32 bound)."""
import functools
import os

import numpy as np
import torch

from util import Collector

EPS = 1e-4
BN_SHAPES = [(3, 4, 4, 8), (2, 5, 3, 72), (2, 40, 40, 8)]      # C = 72: the 64-channel block tail; HW = 1600: 100 row chunks per sample in the reduce (blockIdx.y > 0)
BN_EXTRA_SHAPES = [(2, 3, 3, 6), (2, 2, 2, 1028)]              # C = 6: no 16-byte channel vectors (scalar apply kernel); C = 1028: a second tile of 256 channel vectors
FLOOR = 1e-6
MARGIN = 4.0
BF16 = 2.0 ** -8


def _bf(t):
    return t.to(torch.bfloat16).double()


def bn_inputs(shape, relu, use_batch, seed, bf16=False, equal_rows=False, zero_ab=False, zero_u=False):
    """fp64 inputs of one case. With the fused ReLU no |gam_n xhat + bet_n| is below 1e-3 (asserted), so that no mask can flip between summation orders: elements
    that land inside the band are moved out of it (to +-0.05), x re-rounded to bf16 where the case runs in bf16, until none is left."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = r(N, H, W, C) * (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) + 0.3 * r(C)
    gam = (1.0 + 0.3 * r(N, C)).clamp(0.3, 2.0)
    gam[:, 1] = -gam[:, 1]                       # one channel with negative gains
    bet = 0.3 * r(N, C)
    if equal_rows:
        gam, bet = gam[:1].expand(N, C).clone(), bet[:1].expand(N, C).clone()
    dy, u = r(N, H, W, C), r(N, H, W, C)
    A, B = r(N, C), r(N, C)
    rm, rv = 0.1 * r(C), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    if zero_ab:
        A, B = torch.zeros_like(A), torch.zeros_like(B)
    if zero_u:
        u = torch.zeros_like(u)
    if bf16:
        x, dy, u = _bf(x), _bf(dy), _bf(u)

    def pre(xx):
        if use_batch:
            mean = xx.mean((0, 1, 2))
            var = ((xx - mean) ** 2).mean((0, 1, 2))
        else:
            mean, var = rm, rv
        rs = 1.0 / torch.sqrt(var + EPS)
        return (xx - mean) * rs * gam[:, None, None, :] + bet[:, None, None, :], rs
    if relu:
        for _ in range(50):
            v, rs = pre(x)
            bad = v.abs() < 2e-3
            if not bool(bad.any()):
                break
            tgt = torch.where(v >= 0, 0.05, -0.05)
            x = torch.where(bad, x + (tgt - v) / (gam[:, None, None, :] * rs), x)
            if bf16:
                x = _bf(x)
        v, _ = pre(x)
        assert float(v.abs().min()) >= 1e-3, "a ReLU input of the case sits within 1e-3 of zero"
    return dict(x=x, dy=dy, u=u, gam=gam, bet=bet, A=A, B=B, rm=rm, rv=rv)


def bn_oracle(inp, relu, use_batch, dtype):
    """torch autograd in `dtype` on the CPU: y = relu?(xhat gam_n + bet_n), (dx, dgam, dbet) with a graph, then the gradient of sum u dx + sum A dgam + sum B dbet
    w.r.t. (dy, x, gam). -> dict of first-order and second-order results"""
    c = {k: v.to(dtype) for k, v in inp.items()}
    x, dy, gam, bet = (c[k].clone().requires_grad_(True) for k in ("x", "dy", "gam", "bet"))
    if use_batch:
        mean = x.mean((0, 1, 2))
        var = ((x - mean) ** 2).mean((0, 1, 2))
    else:
        mean, var = c["rm"], c["rv"]
    xhat = (x - mean) / torch.sqrt(var + EPS)
    y = xhat * gam[:, None, None, :] + bet[:, None, None, :]
    if relu:
        y = torch.relu(y)
    dx, dgam, dbet = torch.autograd.grad(y, (x, gam, bet), dy, create_graph=True)
    Lsum = (c["u"] * dx).sum() + (c["A"] * dgam).sum() + (c["B"] * dbet).sum()
    g_dy, g_x, g_gam = torch.autograd.grad(Lsum, (dy, x, gam), allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    return dict(dx=dx.detach(), dgam=dgam.detach(), dbet=dbet.detach(), g_dy=z(g_dy, dy), g_x=z(g_x, x), g_gam=z(g_gam, gam))


def bn_product(inp, relu, use_batch, packed, dev, bf16=False):
    """functional.BNFn with per-sample rows -> autograd.grad(create_graph=True) -> backward"""
    from studiogan_amd import functional as F
    dt = torch.bfloat16 if bf16 else torch.float32
    x = inp["x"].to(dt).to(dev).requires_grad_(True)
    dy = inp["dy"].to(dt).to(dev).requires_grad_(True)
    u = inp["u"].to(dt).to(dev)
    rm, rv = inp["rm"].float().to(dev), inp["rv"].float().to(dev)
    C = x.shape[3]
    cfg = F.BNCfg(bool(use_batch), False, EPS, 0.1, bool(relu), None, packed=packed)
    A, B = inp["A"].float().to(dev), inp["B"].float().to(dev)
    if packed:
        rows = torch.cat([inp["gam"], inp["bet"]], 1).float().to(dev).requires_grad_(True)
        y = F.BNFn.apply(x, rows, None, rm, rv, cfg)
        dx, drows = torch.autograd.grad(y, (x, rows), dy, create_graph=True)
        dgam, dbet = drows[:, :C], drows[:, C:]
    else:
        gam, bet = inp["gam"].float().to(dev).requires_grad_(True), inp["bet"].float().to(dev).requires_grad_(True)
        y = F.BNFn.apply(x, gam, bet, rm, rv, cfg)
        dx, dgam, dbet = torch.autograd.grad(y, (x, gam, bet), dy, create_graph=True)
    Lsum = (u.float() * dx.float()).sum() + (A * dgam).sum() + (B * dbet).sum()
    if packed:
        g_dy, g_x, g_rows = torch.autograd.grad(Lsum, (dy, x, rows), allow_unused=True)
        assert g_rows is None or float(g_rows[:, C:].abs().max()) == 0.0, "the bias rows received a gradient"
        g_gam = None if g_rows is None else g_rows[:, :C]
    else:
        g_dy, g_x, g_gam, g_bet = torch.autograd.grad(Lsum, (dy, x, gam, bet), allow_unused=True)
        assert g_bet is None or float(g_bet.abs().max()) == 0.0, "the bias rows received a gradient"
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    assert g_dy is None or g_dy.dtype == dt
    return dict(dx=dx.detach(), dgam=dgam.detach(), dbet=dbet.detach(), g_dy=z(g_dy, dy), g_x=z(g_x, x), g_gam=z(g_gam, inp["gam"].float().to(dev)))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


SECOND = ("g_dy", "g_x", "g_gam")
FIRST = ("dx", "dgam", "dbet")


def bn_grid(shape):
    """(relu, use_batch, flags) of every case a shape runs: the full relu x use_batch grid, plus A = B = 0 and u = 0"""
    cases = [(relu, ub, {}) for relu in (0, 1) for ub in (0, 1)]
    cases += [(1, 1, {"zero_ab": True}), (1, 1, {"zero_u": True}), (0, 0, {"zero_u": True})]
    return cases


@functools.lru_cache(maxsize=None)
def bn_bounds(bf16=False):
    """the fp32 bound per output (module docstring): torch fp32 against torch fp64 over every case of every shape -> {output: (measured, bound)}"""
    worst = dict.fromkeys(FIRST + SECOND, 0.0)
    for si, shape in enumerate(BN_SHAPES + BN_EXTRA_SHAPES):
        for ci, (relu, ub, fl) in enumerate(bn_grid(shape)):
            inp = bn_inputs(shape, relu, ub, 100 * si + ci, bf16=bf16, **fl)
            o64, o32 = bn_oracle(inp, relu, ub, torch.float64), bn_oracle(inp, relu, ub, torch.float32)
            for k in worst:
                if float(o64[k].abs().max()) > 0.0:
                    worst[k] = max(worst[k], _rel(o32[k], o64[k]))
    return {k: (v, max(MARGIN * v, FLOOR)) for k, v in worst.items()}


def bn_case(shape, dev, bf16=False, layouts=(True, False)):
    """Test 1: every case of `shape` in both layouts against the fp64 oracle"""
    si = (BN_SHAPES + BN_EXTRA_SHAPES).index(shape)
    bounds = bn_bounds(bf16)
    C = Collector()
    for ci, (relu, ub, fl) in enumerate(bn_grid(shape)):
        inp = bn_inputs(shape, relu, ub, 100 * si + ci, bf16=bf16, **fl)
        o = bn_oracle(inp, relu, ub, torch.float64)
        for packed in layouts:
            p = bn_product(inp, relu, ub, packed, dev, bf16)
            tag = f"{shape} relu={relu} batch={ub} {'packed' if packed else 'separate'} {fl or ''}"
            for k in FIRST + SECOND:
                tol = BF16 if (bf16 and k in ("dx", "g_dy", "g_x")) else bounds[k][1]
                if float(o[k].abs().max()) == 0.0:
                    C.check(f"{tag} {k} (zero)", p[k], o[k], 0.0, abs_tol=0.0)
                else:
                    C.check(f"{tag} {k}", p[k], o[k], tol)
    C.finish()


def bn_equal_rows_case(dev):
    """all rows equal, A = B = 0: the per-sample pass against the existing per-channel one (functional.BNBwdFn) -- the same formulas in fp32 with another evaluation
    order, held to the fp32 bound of the outputs (both sit that close to the fp64 oracle); the per-channel gain gradient is the sum of the rows' gradients"""
    from studiogan_amd import functional as F
    shape = BN_SHAPES[1]
    bounds = bn_bounds(False)
    C = Collector()
    for relu, ub in ((1, 1), (0, 1), (1, 0)):
        inp = bn_inputs(shape, relu, ub, 900 + 2 * relu + ub, equal_rows=True, zero_ab=True)
        p = bn_product(inp, relu, ub, True, dev)
        x = inp["x"].float().to(dev).requires_grad_(True)
        dy = inp["dy"].float().to(dev).requires_grad_(True)
        gam, bet = inp["gam"][0].float().to(dev).requires_grad_(True), inp["bet"][0].float().to(dev)
        cfg = F.BNCfg(bool(ub), False, EPS, 0.1, bool(relu), None)
        y = F.BNFn.apply(x, gam, bet, inp["rm"].float().to(dev), inp["rv"].float().to(dev), cfg)
        (dx,) = torch.autograd.grad(y, (x,), dy, create_graph=True)
        g_dy, g_x, g_gam = torch.autograd.grad((inp["u"].float().to(dev) * dx).sum(), (dy, x, gam), allow_unused=True)
        tag = f"equal rows relu={relu} batch={ub}"
        C.check(tag + " dx", p["dx"], dx, bounds["dx"][1])
        C.check(tag + " g_dy", p["g_dy"], g_dy, bounds["g_dy"][1])
        if ub:
            C.check(tag + " g_x", p["g_x"], g_x, bounds["g_x"][1])
        else:
            assert float(p["g_x"].abs().max()) == 0.0 and (g_x is None or float(g_x.abs().max()) == 0.0)
        C.check(tag + " g_gam", p["g_gam"].sum(0), g_gam, bounds["g_gam"][1])
    C.finish()


def write_bounds(path):
    """profiles/logan_cbn_bounds.txt: the measured reference-side errors and the bounds they give"""
    import platform
    lines = ["Bounds of tests/logan_cbn_checks.py, measured on the REFERENCE side: torch autograd's double backward in fp32 on the CPU against the same in fp64,",
             "per output, max-abs error over the tensor's max-abs, the largest over the cases of the check. bound = max(4 x measured, 1e-6).",
             f"torch {torch.__version__}, {platform.machine()}; python tests/logan_cbn_checks.py writes this file.", ""]
    for name, b in (("test 1 (BNFn with per-sample rows), fp32 inputs", bn_bounds(False)), ("test 1, bf16-rounded x / dy / u (the bf16 outputs dx, g_dy, g_x are held to 2^-8 instead)", bn_bounds(True)),
                    ("test 2 (CbnAffineFn / CbnAffineGroupFn, spectral norm on)", affine_bounds())):
        lines.append(name)
        for k, (m, bd) in b.items():
            lines.append(f"    {k:10s} measured {m:.3e}   bound {bd:.3e}")
        lines.append("")
    open(path, "w").write("\n".join(lines))


# ---- whole updates against the fp64 oracle (oracle/restate.py networks + the five lines of latent_optimise restated, as aug_checks.logan_oracle_case) ----------
LOGAN_LOSS = {"lo_rate": 0.8, "lo_steps4train": 2, "lo_steps4eval": 2, "lo_alpha": 0.9, "lo_beta": 0.1, "lo_lambda": 0.1}      # configs/CIFAR10/LOGAN.yaml's block
# latents = LOGAN_SCALE * randn(seed): chosen on the CPU so that the tie guard below passes for both fixtures and both updates (no ReLU input of either network
# within fp32 rounding of zero along the whole double backward), then fixed. The guard runs again inside every test, before the product.
LOGAN_SEEDS = {"biggan32": 11, "bigdeep32": 11}
LOGAN_SCALE = 0.9
TIE = 1e-5


def logan_inputs(name):
    from util import load_golden, sub
    fix, meta = load_golden(name)
    y = meta["yaml"]
    B, zd, nc = meta["batch"], y["MODEL"]["z_dim"], y["DATA"]["num_classes"]
    g = torch.Generator().manual_seed(LOGAN_SEEDS[name])
    z = {s: LOGAN_SCALE * torch.randn(B, zd, generator=g) for s in ("d", "g")}
    fl = {s: torch.randint(0, nc, (B,), generator=g) for s in ("d", "g")}
    draw = {s: torch.rand(B, 1, generator=g) for s in ("d", "g")}
    ins = sub(fix, "in/")
    return y, meta, sub(fix, "G_init/"), sub(fix, "D_init/"), ins["real0"], ins["rl0"], z, fl, draw


def logan_oracle(y, gsd, dsd, pg, pd, real, rl, z, fl, draw, side, dtype, LS=LOGAN_LOSS, eval_mode=False):
    """one update (side "d" / "g") of the LOGAN step on the oracle's networks in `dtype`; eval_mode: only the latent step, both networks in eval mode
    -> dict(zs, cost, loss, grads)"""
    from oracle import restate as O, make_golden as MG
    gen, dis = O.model_fns(MG.oracle_cfg(y))
    cast = lambda v: v.clone().to(dtype) if v.is_floating_point() else v.clone()
    GP, GB = {k: cast(v) for k, v in gsd.items() if k in pg}, {k: cast(v) for k, v in gsd.items() if k not in pg}
    DP, DB = {k: cast(v) for k, v in dsd.items() if k in pd}, {k: cast(v) for k, v in dsd.items() if k not in pd}
    leaves = DP if side == "d" else GP
    if not eval_mode:
        for v in leaves.values():
            v.requires_grad_(True)
    mode = "eval" if eval_mode else ("untrack" if side == "d" else "track")
    sn = not eval_mode
    zc = z.to(dtype).requires_grad_(True)
    adv, _ = dis(gen(zc, fl, GP, GB, mode, sn), fl, DP, DB, mode, sn)
    zg = torch.autograd.grad(adv.sum(), zc, create_graph=True)[0]
    delta = LS["lo_alpha"] * zg / (LS["lo_beta"] + (zg.norm(2, dim=1) ** 2).unsqueeze(1))
    zs = torch.clamp(zc + (draw > 1 - LS["lo_rate"]).to(dtype) * delta, -1.0, 1.0)
    cost = (delta.norm(2, dim=1) ** 2).mean()
    out = dict(zs=zs.detach(), cost=cost.detach(), zg=zg.detach(), z=zc.detach())
    if eval_mode:
        return out
    fake = gen(zs, fl, GP, GB, mode)
    fd, _ = dis(fake, fl, DP, DB) if side == "g" else (None, None)
    if side == "d":
        rd, _ = dis(real.to(dtype), rl, DP, DB)
        fd, _ = dis(fake, fl, DP, DB)
        loss = O.d_loss("hinge", rd, fd) + LS["lo_lambda"] * cost
    else:
        loss = O.g_loss("hinge", fd) + LS["lo_lambda"] * cost
    gr = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    out.update(loss=loss.detach(), grads={k: (g if g is not None else torch.zeros_like(v)).detach() for (k, v), g in zip(leaves.items(), gr)})
    return out


def tie_guard(o64, o32):
    """the oracle in fp64 against the same in fp32 torch: parameter gradients further apart than 1e-5 of the largest mean that the latents sit on a ReLU tie"""
    gmax = max(float(g.abs().max()) for g in o64["grads"].values())
    worst = max(float((o32["grads"][k].double() - g).abs().max()) for k, g in o64["grads"].items()) / gmax
    return worst


def build_pair(y, gsd, dsd, dev, mixed=False):
    from test_model_gpu import build_from_yaml
    G, D = build_from_yaml(y, mixed, dev)
    G.load_state_dict({k: v.to(dev) for k, v in gsd.items()}, strict=True)
    D.load_state_dict({k: v.to(dev) for k, v in dsd.items()}, strict=True)
    return G, D


def make_worker(G, D, y, meta, LS=LOGAN_LOSS, apply_lo=True):
    from util import hyper
    from studiogan_amd.worker import Worker
    opt = hyper(y)
    kw = dict(apply_lo=True, lo_rate=LS["lo_rate"], lo_steps4train=LS["lo_steps4train"], lo_alpha=LS["lo_alpha"], lo_beta=LS["lo_beta"], lo_lambda=LS["lo_lambda"]) if apply_lo else {}
    return Worker(G, D, opt["z_dim"], y["DATA"]["num_classes"], meta["batch"], "hinge", opt["g_lr"], opt["d_lr"], opt["beta1"], opt["beta2"], d_updates_per_step=1, **kw)


def logan_update_case(name, side, dev):
    """Test 3: Worker(apply_lo=True).train_discriminator / train_generator on the networks of tests/golden/<name>.npz (cBN + attention + SN in G, PD + SN + attention
    in D) against the fp64 oracle: moved latents, transport cost, loss and every parameter gradient (for the generator update: incl. the conditional batch norms' gain /
    bias weights and the shared embedding). Bounds: aug_checks.logan_oracle_case's (2e-5 on the scalars, 1e-4 on the gradients with floor 1e-2 of the largest). A
    failure with the one-flipped-unit signature is to be diagnosed as in profiles/r06_logan_tie.txt (other inputs), not met with a looser bound."""
    from aug_checks import Replayed
    from studiogan_amd import losses as SL
    y, meta, gsd, dsd, real, rl, z, fl, draw = logan_inputs(name)
    G, D = build_pair(y, gsd, dsd, dev)
    pg, pd = {k for k, _ in G.named_parameters()}, {k for k, _ in D.named_parameters()}
    o = logan_oracle(y, gsd, dsd, pg, pd, real, rl, z[side], fl[side], draw[side], side, torch.float64)
    o32 = logan_oracle(y, gsd, dsd, pg, pd, real, rl, z[side], fl[side], draw[side], side, torch.float32)
    tie = tie_guard(o, o32)
    print(f"[{name} {side}] tie guard: fp32 torch against fp64, gradients: {tie:.3e} of the largest; |dz| max {float((o['zs'] - o['z']).abs().max()):.3e}, cost {float(o['cost']):.3e}")
    assert tie <= TIE, f"the test's latents sit on a ReLU tie ({tie:.2e}): choose another seed"
    inside = o["zs"].abs() < 1.0          # (elements the clamp leaves alone: only they show the step itself)
    assert float(((o["zs"] - o["z"]) * inside).abs().max()) > 1e-3 and float(inside.double().mean()) > 0.3, "the latents did not move: the check would not see the second-order pass"
    w = make_worker(G, D, y, meta)
    got = {}
    lo = SL.latent_optimise

    def spy(**kw):
        zs, c = lo(**kw)
        got["zs"] = zs.detach().clone()
        return zs, c
    SL.latent_optimise = spy
    try:
        with Replayed([draw[side]]):
            if side == "d":
                loss = w.train_discriminator(0, [(real.to(dev), rl.to(dev))], [(z[side].to(dev), fl[side].to(dev))])
            else:
                loss = w.train_generator(0, [(z[side].to(dev), fl[side].to(dev))])
    finally:
        SL.latent_optimise = lo
    C = Collector()
    C.check(f"{side} moved latents (z' - z)", got["zs"].cpu().double() - z[side].double(), o["zs"] - o["z"], 2e-5)
    C.check(f"{side} transport cost", w.trsp_cost, o["cost"], 2e-5)
    C.check(f"{side} loss", loss, o["loss"], 2e-5)
    gmax = max(float(g.abs().max()) for g in o["grads"].values())
    net = D if side == "d" else G
    for k, prm in net.named_parameters():
        C.check(f"{side}_grad/" + k, prm.grad if prm.grad is not None else torch.zeros_like(prm), o["grads"][k], 1e-4, floor=1e-2 * gmax)
    C.finish()


# ---- test 2: the conditional batch norms' affine products [1 + gain(y) | bias(y)] as differentiable operators ------------------------------------------------------
AFF_B, AFF_K = 3, 20
AFF_OUT = ("first dy", "g_dgb", "g_w")


def _affine_root(C, n, dev, swap=()):
    """n conditional batch norms (spectral norm on) under one root = one weight bank; swap: indices whose bias linear is registered BEFORE the gain linear, so that
    the two weight images are not back to back in the bank (CbnAffineFn's two-GEMM form)"""
    from studiogan_amd import ops

    class Root(torch.nn.Module):
        def __init__(self):
            super().__init__()
            MOD = ops.Modules(apply_g_sn=True, g_cond_mtd="cBN", backbone="big_resnet")
            self.cbn = torch.nn.ModuleList([ops.ConditionalBatchNorm2d(AFF_K, C, MOD) for _ in range(n)])
            for i in swap:
                mods = self.cbn[i]._modules
                mods["gain"] = mods.pop("gain")
            ops.init_weights(self.modules, "ortho")
            ops.adopt(self, torch.float32)
    torch.manual_seed(7 + C)
    return Root().to(dev)


def _affine_oracle(sd, ys, yidx, n, T, U, dtype):
    """F.linear on W / sigma (one power iteration, as the module's forward in training mode): rows_i = [1 + y W_g^T | y W_b^T]; first pass d(sum_i T_i rows_i)/dy with a
    graph; second pass: gradient of sum_g U_g dy_g w.r.t. T (the cotangents of the rows), and both weights of every layer"""
    from oracle import restate as O
    P = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items() if k.endswith("weight_orig")}
    B = {k: v.clone().to(dtype) for k, v in sd.items() if k.endswith(("weight_u", "weight_v"))}
    yv = [t.clone().to(dtype).requires_grad_(True) for t in ys]
    Tv = [t.clone().to(dtype).requires_grad_(True) for t in T]
    tot = 0.0
    for i in range(n):
        y = yv[yidx[i]]
        rows = torch.cat([1.0 + O.linear(y, P, B, f"cbn.{i}.gain"), O.linear(y, P, B, f"cbn.{i}.bias")], 1)
        tot = tot + (Tv[i] * rows).sum()
    dys = torch.autograd.grad(tot, yv, create_graph=True)
    L2 = sum((U[g].to(dtype) * dys[g]).sum() for g in range(len(yv)))
    names = [f"cbn.{i}.{h}.weight_orig" for i in range(n) for h in ("gain", "bias")]
    gr = torch.autograd.grad(L2, Tv + [P[k] for k in names])
    return dict(dys=[d.detach() for d in dys], g_T=list(gr[:n]), g_w=dict(zip(names, gr[n:])))


def _affine_inputs(C, n, G):
    g = torch.Generator().manual_seed(50 + C + n)
    ys = [torch.randn(AFF_B, AFF_K, generator=g) for _ in range(G)]
    T = [torch.randn(AFF_B, 2 * C, generator=g) for _ in range(n)]
    U = [torch.randn(AFF_B, AFF_K, generator=g) for _ in range(G)]
    return ys, T, U


AFF_CASES = [("single adjacent", 1, (), (0,), False), ("single non-adjacent", 1, (0,), (0,), False), ("group of 3, 2 vectors", 3, (), (0, 1, 0), True),
             ("group of 3, one non-adjacent", 3, (1,), (0, 1, 0), True)]


def _affine_run(C, n, swap, yidx, grouped, dev, dtype_oracle=None):
    """-> (product results or None, fp64 oracle, fp32 oracle)"""
    from studiogan_amd import functional as F
    from studiogan_amd.bank import get_bank
    root = _affine_root(C, n, dev, swap)
    sd = {k: v.detach().cpu().clone() for k, v in root.state_dict().items()}
    G = max(yidx) + 1
    ys, T, U = _affine_inputs(C, n, G)
    o64, o32 = _affine_oracle(sd, ys, yidx, n, T, U, torch.float64), _affine_oracle(sd, ys, yidx, n, T, U, torch.float32)
    if dev is None:
        return None, o64, o32
    root.train()
    bank = get_bank(root, torch.float32)
    slot = bank.begin_forward(True)
    yv = [t.to(dev).requires_grad_(True) for t in ys]
    Tv = [t.to(dev).requires_grad_(True) for t in T]
    mods = list(root.cbn)
    if grouped:
        F.cbn_prefetch(slot, [(m, yv[yidx[i]]) for i, m in enumerate(mods)])
        assert slot.cbn_rows is not None and len(slot.cbn_rows) == n, "the grouped launch did not take the layers"
        rows = [slot.cbn_rows[id(m)] for m in mods]
    else:
        rows = [F.CbnAffineFn.apply(yv[yidx[i]], m.gain.master_weight, m.bias.master_weight, m.gain._sg_rt, m.bias._sg_rt, slot, m._ones2) for i, m in enumerate(mods)]
    pg, pb = bank.w_f32(slot, mods[0].gain._sg_rt), bank.w_f32(slot, mods[0].bias._sg_rt)
    for i, m in enumerate(mods):
        adj = bank.w_f32(slot, m.bias._sg_rt) == bank.w_f32(slot, m.gain._sg_rt) + 4 * C * AFF_K
        assert adj == (i not in swap), f"layer {i}: weight images adjacent = {adj}"
    tot = sum((Tv[i] * rows[i]).sum() for i in range(n))
    dys = torch.autograd.grad(tot, yv, create_graph=True)
    L2 = sum((U[g].to(dev) * dys[g]).sum() for g in range(G))
    for p in root.parameters():
        p.grad = None
    L2.backward()
    got = dict(dys=[d.detach() for d in dys], g_T=[t.grad for t in Tv], g_w={k: p.grad for k, p in root.named_parameters()})
    return got, o64, o32


@functools.lru_cache(maxsize=None)
def affine_bounds():
    worst = dict.fromkeys(AFF_OUT, 0.0)
    for C in (8, 24):
        for _, n, swap, yidx, grouped in AFF_CASES:
            _, o64, o32 = _affine_run(C, n, swap, yidx, grouped, None)
            worst["first dy"] = max([worst["first dy"]] + [_rel(a, b) for a, b in zip(o32["dys"], o64["dys"])])
            worst["g_dgb"] = max([worst["g_dgb"]] + [_rel(a, b) for a, b in zip(o32["g_T"], o64["g_T"])])
            worst["g_w"] = max([worst["g_w"]] + [_rel(o32["g_w"][k], o64["g_w"][k]) for k in o64["g_w"]])
    return {k: (v, max(MARGIN * v, FLOOR)) for k, v in worst.items()}


def affine_case(C, dev):
    """CbnAffineFn (adjacent and non-adjacent weight images) and CbnAffineGroupFn (3 layers, 2 distinct conditioning vectors), B = 3, K = 20, spectral norm on: the
    double backward w.r.t. the rows' cotangents and both weights of every layer (through the normalisation's backward) against fp64 torch"""
    bounds = affine_bounds()
    Cc = Collector()
    for tag, n, swap, yidx, grouped in AFF_CASES:
        got, o64, _ = _affine_run(C, n, swap, yidx, grouped, dev)
        for g in range(max(yidx) + 1):
            Cc.check(f"C={C} {tag}: first pass dy[{g}]", got["dys"][g], o64["dys"][g], bounds["first dy"][1])
        for i in range(n):
            Cc.check(f"C={C} {tag}: g_dgb[{i}]", got["g_T"][i], o64["g_T"][i], bounds["g_dgb"][1])
        for k, g in o64["g_w"].items():
            assert got["g_w"][k] is not None, k
            Cc.check(f"C={C} {tag}: g_w {k}", got["g_w"][k], g, bounds["g_w"][1])
    Cc.finish()


# ---- test 4: the latent step at evaluation time ----------------------------------------------------------------------------------------------------------------
class _FixedFloatTensor:
    """torch.FloatTensor(B, 1).uniform_() of latent_optimise hands out the recorded drop-mask draw (nothing else of torch's samplers is touched)"""

    def __init__(self, draw):
        self.draw = draw

    def __enter__(self):
        self.saved, draw = torch.FloatTensor, self.draw

        class FT:
            def __init__(self, *size):
                assert tuple(size) == tuple(draw.shape), size

            def uniform_(self, a=0.0, b=1.0):
                return draw.clone()
        torch.FloatTensor = FT
        return self

    def __exit__(self, *a):
        torch.FloatTensor = self.saved


def logan_eval_case(dev, name="biggan32"):
    """metrics.generate_images_and_stack_features(latent_opt=...) with generator and discriminator in eval mode (running statistics: use_batch = 0 through every
    conditional batch norm, no power iteration), lo_steps4eval = 2: the latents the generator finally receives against the oracle's step from the latents the
    function drew. The running statistics are those of two training-mode forwards of the oracle."""
    from studiogan_amd import metrics as M
    from oracle import restate as O, make_golden as MG
    y, meta, gsd, dsd, real, rl, z, fl, draw = logan_inputs(name)
    gsd, dsd = {k: v.clone() for k, v in gsd.items()}, {k: v.clone() for k, v in dsd.items()}
    G, D = build_pair(y, gsd, dsd, dev)
    pg, pd = {k for k, _ in G.named_parameters()}, {k for k, _ in D.named_parameters()}
    gen, dis = O.model_fns(MG.oracle_cfg(y))
    GB, DB = {k: v for k, v in gsd.items() if k not in pg}, {k: v for k, v in dsd.items() if k not in pd}
    with torch.no_grad():
        # a state worth evaluating: forty training-mode forwards of both oracle networks move the running statistics (momentum 0.1: the initial (0, 1) has decayed to
        # 1.5 %) and the spectral-norm vectors (eval mode does no power iteration: on the fixture's random u / v the weights are divided by a sigma far too small,
        # d D(G(z)) / dz is ~1e11 at this width and the step ~1e-12). gsd / dsd are what both sides load.
        for i in range(40):
            s = "dg"[i % 2]
            img = gen(z[s], fl[s], {k: v for k, v in gsd.items() if k in pg}, GB, "track")
            dis(img, fl[s], {k: v for k, v in dsd.items() if k in pd}, DB)
    G.load_state_dict({k: v.to(dev) for k, v in gsd.items()}, strict=True)
    D.load_state_dict({k: v.to(dev) for k, v in dsd.items()}, strict=True)
    G.eval(), D.eval()
    calls = []

    class Cap(torch.nn.Module):
        def __init__(self, g):
            super().__init__()
            self.g = g

        def forward(self, zs, ys, eval=False):
            calls.append((zs.detach().cpu().clone(), ys.detach().cpu().clone(), eval))
            return self.g(zs, ys, eval=eval)

    class Stub:
        def get_outputs(self, x, quantize=True):
            assert bool(torch.isfinite(x).all())
            return torch.zeros(x.shape[0], 8, device=x.device), torch.zeros(x.shape[0], 8, device=x.device)
    B, LS = meta["batch"], LOGAN_LOSS
    torch.manual_seed(21)
    saved = M.softmax_rows
    M.softmax_rows = lambda t: t
    try:
        with _FixedFloatTensor(draw["d"]):
            M.generate_images_and_stack_features(Cap(G), Stub(), B, B, y["MODEL"]["z_dim"], y["DATA"]["num_classes"], device=dev,
                                                 latent_opt=dict(discriminator=D, lo_rate=LS["lo_rate"], lo_steps=LS["lo_steps4eval"], lo_alpha=LS["lo_alpha"], lo_beta=LS["lo_beta"]))
    finally:
        M.softmax_rows = saved
    assert len(calls) == 2 and all(c[2] for c in calls), "one generator forward inside the latent step, one for the images, both with eval=True"
    z0, ys = calls[0][0], calls[0][1]
    o = logan_oracle(y, gsd, dsd, pg, pd, None, None, z0, ys, draw["d"], "d", torch.float64, eval_mode=True)
    o32 = logan_oracle(y, gsd, dsd, pg, pd, None, None, z0, ys, draw["d"], "d", torch.float32, eval_mode=True)
    tie = float((o32["zg"].double() - o["zg"]).abs().max() / o["zg"].abs().max())
    inside = o["zs"].abs() < 1.0          # (elements the clamp leaves alone: only they show the step itself)
    step = float(((o["zs"] - o["z"]) * inside).abs().max())
    print(f"[{name} eval] tie guard: fp32 torch against fp64, d D(G(z)) / dz: {tie:.3e}; |dz| max inside the clamp {step:.3e}, {float(inside.double().mean()):.2f} of the elements inside")
    assert tie <= TIE, f"the drawn latents sit on a ReLU tie ({tie:.2e}): choose another seed"
    assert step > 1e-3 and float(inside.double().mean()) > 0.3, "the latents did not move: the check would not see the second-order pass"
    C = Collector()
    C.check("eval: moved latents (z' - z)", calls[1][0].double() - z0.double(), o["zs"] - o["z"], 2e-5)
    C.finish()


# ---- test 5: mixed precision ---------------------------------------------------------------------------------------------------------------------------------------
def logan_mixed_case(dev, name="biggan32"):
    """mixed_precision=True: one discriminator and one generator update complete, the losses are finite, and the transport cost of either update is within 5e-2
    (relative) of the fp32 run's -- the project's bf16 step-level scalar bound (aug_checks gradient_penalty_case)."""
    from aug_checks import Replayed
    y, meta, gsd, dsd, real, rl, z, fl, draw = logan_inputs(name)
    res = {}
    for mixed in (False, True):
        G, D = build_pair(y, gsd, dsd, dev, mixed)
        w = make_worker(G, D, y, meta)
        with Replayed([draw["d"]]):
            d_loss = w.train_discriminator(0, [(real.to(dev), rl.to(dev))], [(z["d"].to(dev), fl["d"].to(dev))])
        d_cost = w.trsp_cost.detach().float().cpu()
        with Replayed([draw["g"]]):
            g_loss = w.train_generator(0, [(z["g"].to(dev), fl["g"].to(dev))])
        g_cost = w.trsp_cost.detach().float().cpu()
        res[mixed] = (float(d_loss), float(g_loss), float(d_cost), float(g_cost))
        for k, p in list(G.named_parameters()) + list(D.named_parameters()):
            assert bool(torch.isfinite(p.detach().float()).all()), k
    print("fp32 (d_loss, g_loss, d cost, g cost):", res[False], " bf16:", res[True])
    assert all(np.isfinite(v) for v in res[True]), res[True]
    for i, what in ((2, "discriminator"), (3, "generator")):
        rel = abs(res[True][i] - res[False][i]) / abs(res[False][i])
        assert rel <= 5e-2, f"transport cost of the {what} update: bf16 {res[True][i]:.6e} against fp32 {res[False][i]:.6e} ({rel:.2e} relative)"


# ---- test 6: the first-order path launches what it launched before ----------------------------------------------------------------------------------------------
# library calls (studiogan_amd._lib.call, by entry point) of one plain biggan32 discriminator + generator update in fp32 WITHOUT latent optimisation, counted on the
# commit in front of the conditional second-order pass
FIRST_ORDER_CALLS = {'sg_adam_ema': 2, 'sg_add_relu': 6, 'sg_avgpool2_bwd': 1, 'sg_avgpool2_fwd': 3, 'sg_bn_apply': 14, 'sg_bn_bwd_apply_res': 7, 'sg_bn_bwd_finalize': 7,
                     'sg_bn_bwd_reduce': 7, 'sg_bn_finalize': 14, 'sg_bn_partial_stats': 14, 'sg_colsum': 31, 'sg_conv2d_fwd': 125, 'sg_conv2d_wgrad': 42,
                     'sg_conv2d_wgrad_plan': 42, 'sg_dot': 3, 'sg_embedding_bwd': 3, 'sg_embedding_fwd': 5, 'sg_gemm': 41, 'sg_linear_group': 2, 'sg_loss_d': 1, 'sg_loss_g': 1,
                     'sg_maxpool2_bwd': 8, 'sg_maxpool2_fwd': 10, 'sg_nchw_grad_to_nhwc': 1, 'sg_nchw_to_nhwc': 5, 'sg_nhwc_to_nchw': 4, 'sg_pd_head_bwd': 3,
                     'sg_pd_head_fwd': 3, 'sg_relu_mask': 6, 'sg_relu_sum_hw_bwd': 3, 'sg_relu_sum_hw_fwd': 3, 'sg_sn_backward': 3, 'sg_sn_forward': 5, 'sg_softmax_rows': 5,
                     'sg_softmax_rows_bwd': 4}      # 434 in all


def first_order_calls(dev, name="biggan32"):
    import collections
    from studiogan_amd import _lib as L
    y, meta, gsd, dsd, real, rl, z, fl, draw = logan_inputs(name)
    G, D = build_pair(y, gsd, dsd, dev)
    w = make_worker(G, D, y, meta, apply_lo=False)
    counts, orig = collections.Counter(), L.call

    def counting(nm, *a):
        counts[nm] += 1
        return orig(nm, *a)
    L.call = counting
    try:
        w.train_discriminator(0, [(real.to(dev), rl.to(dev))], [(z["d"].to(dev), fl["d"].to(dev))])
        w.train_generator(0, [(z["g"].to(dev), fl["g"].to(dev))])
    finally:
        L.call = orig
    return dict(counts)


def first_order_case(dev):
    got = first_order_calls(dev)
    print("library calls:", sum(got.values()), dict(sorted(got.items())))
    assert not any(k.startswith("sg_cbn_bwd2") for k in got)
    assert got == FIRST_ORDER_CALLS, {k: (got.get(k, 0), FIRST_ORDER_CALLS.get(k, 0)) for k in set(got) | set(FIRST_ORDER_CALLS) if got.get(k, 0) != FIRST_ORDER_CALLS.get(k, 0)}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_bounds(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "logan_cbn_bounds.txt"))
