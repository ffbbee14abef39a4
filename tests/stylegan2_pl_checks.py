"""The checks of path-length regularisation through the StyleGAN2 generator that tests/test_stylegan2_pl_cpu.py runs through the kernel-source interpreter
and tests/test_stylegan2_pl_gpu.py on the device: one statement of each, `dev` says where the tensors live. Expectations are fp64 autograd of the restatements
(tests/modconv_ref.py, tests/stylegan2_ref.py); the networks' come from tests/golden/stylegan2_pl.npz. TEST INFRASTRUCTURE ONLY.

Bounds: the operators' existing ones, 2e-5 of the expected tensor's range in fp32 and 1e-2 in bf16 against fp64 on bf16-rounded inputs; the networks at
max(2e-5, 4 x ref32_err) in fp32 and 3 x the fixture's bf16_floor with bf16 blocks."""
import contextlib
import inspect

import torch

import modconv_ref as R
import stylegan2_ref as S
from util import check

CL = torch.channels_last
# the seven operator geometries of tests/modconv_ref.py, and one whose 72 output channels take the engine's 96-row tile in fp32 (bf16 has no such tangent
# instantiation and runs it as a ragged 128-row tile). i, j: 6 input channels, no multiple of the 16-byte vector in either dtype, so the operand policy's
# wrap-around table read runs (more than once per chunk in bf16, 6 < 8): i at up = 1 with 36 output channels (the 128 x 128 tile, ragged) on an odd map, j
# at up = 2 through the transposed gather and the stride-2 data gradient, per-sample noise. (Appended: the seeds are 6100 + index.)
OP_CASES = dict(R.OP_CASES, h=(2, 16, 72, 6, 3, 1, True, "sample", True), i=(2, 6, 36, 5, 3, 1, True, "shared", True), j=(2, 6, 8, 4, 3, 2, True, "sample", False))
MODCONV_CASES = list(OP_CASES)
TAIL_EPI = {      # the fused tail's epilogues: (act, gain, clamp)
    "lrelu": ("lrelu", S.SQRT2, None),
    "lrelu_clamp": ("lrelu", S.SQRT2, 2.5),
    "linear": ("linear", 1.0, None),
    "linear_clamp": ("linear", 1.0, 2.5),
}


def dtype_name(dtype):
    return "fp32" if dtype == torch.float32 else "bf16"


def tol_of(dtype):
    return 2e-5 if dtype == torch.float32 else 1e-2


def grid(seed, *shape, scale=1.0):
    """a seeded tensor on the 2^-6 grid below 3 (bf16 holds every value)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale * 64).round().clamp(-192, 192) / 64


def _rb(t, dtype):
    """fp64 values of t as the kernel is given them"""
    return t.double() if dtype == torch.float32 else t.to(torch.bfloat16).double()


def _dot(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a * b).sum()), float((a * b).abs().sum())


def assert_pairing(name, lhs_terms, rhs_terms, tol):
    """sum <a, b> over lhs_terms == sum <a, b> over rhs_terms, to tol of the sum of the absolute products (each product carries its operands' rounding)"""
    lhs, rhs, scale = 0.0, 0.0, 0.0
    for a, b in lhs_terms:
        v, s = _dot(a, b)
        lhs, scale = lhs + v, scale + s
    for a, b in rhs_terms:
        v, s = _dot(a, b)
        rhs, scale = rhs + v, scale + s
    print(f"{name:48s} lhs={lhs:.9e} rhs={rhs:.9e} tol={tol:.1e} of {scale:.3e}")
    assert abs(lhs - rhs) <= tol * scale, (name, lhs, rhs, scale)


# ---- modulated_conv2d ---------------------------------------------------------------------------------------------------------------------------------------

def modconv_second_order_ref(x, w, s, nz, gy, vx, vs, up, demod, flip, gain=None):
    """fp64: (dx, ds, (d_gy, d_x, d_s, d_w)) with Psi = <vx, dx> + <vs, ds> differentiated for gy, x, s and the weight"""
    x, w, s, gy = (t.detach().clone().requires_grad_(True) for t in (x, w, s, gy))
    y = R.modconv_ref(x, w, s, nz, up=up, demodulate=demod, flip_weight=flip, f=R.low_pass().double())
    if gain is not None:
        y = y * gain
    dx, ds = torch.autograd.grad(y, [x, s], gy, create_graph=True)
    second = torch.autograd.grad((dx * vx).sum() + (ds * vs).sum(), [gy, x, s, w])
    return dx.detach(), ds.detach(), second


def check_modconv_second_order(lib, dev, tag, dtype, report=None, gain=None, route="fused"):
    """all four second-order gradients of one operator case against fp64 autograd, the pairing identity, the launch count; gain: the post_gain case (through
    _ModConvFn, as StyleGAN3's input layer calls it; no noise). route: "fused" (one sg_modconv2d_jvp launch), "composition" (operand combine,
    sg_modconv2d_fwd, multiply-add with y) or None, the operator's own measured rule (modulated_conv2d.tangent_fused)"""
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops import modulated_conv2d as MC
    N, C, Cout, H, k, up, demod, noise, flip = OP_CASES[tag]
    if gain is not None:
        noise = None
    x, w, s, nz, gy = R.exact_inputs(6100 + MODCONV_CASES.index(tag), N, C, Cout, H, k, up, noise)
    assert bool((s == 0).any()), "the styles of every case hold exact zeros"
    vx, vs = grid(6200 + MODCONV_CASES.index(tag), *x.shape), grid(6300 + MODCONV_CASES.index(tag), *s.shape)
    tol = tol_of(dtype)
    xr, wr, gyr, vxr = (_rb(t, dtype) for t in (x, w, gy, vx))
    edx, eds, want = modconv_second_order_ref(xr, wr, s, nz, gyr, vxr, vs, up, demod, flip, gain)
    xd = x.to(dev, dtype).contiguous(memory_format=CL).requires_grad_(True)
    wd, sd = w.to(dev, torch.float32).requires_grad_(True), s.to(dev, torch.float32).requires_grad_(True)
    nd = None if nz is None else nz.to(dev, torch.float32)
    gyd = gy.to(dev, dtype).requires_grad_(True)
    if gain is None:
        y = MC.modulated_conv2d(xd, wd, sd, noise=nd, up=up, padding=k // 2, resample_filter=R.low_pass().to(dev), demodulate=demod, flip_weight=flip)
    else:
        assert up == 1
        y = MC._ModConvFn.apply(xd, wd, sd, None, 1, demod, flip, torch.tensor([gain], dtype=torch.float32, device=dev))
    wgrads = []
    raw, saved_route = MC.conv2d_wgrad_raw, MC.TANGENT_ROUTE[0]
    MC.conv2d_wgrad_raw = lambda *a, **kw: (wgrads.append(1), raw(*a, **kw))[1]
    MC.TANGENT_ROUTE[0] = route
    fused = MC.tangent_fused(dtype, up)
    assert route is None or fused == (route == "fused")
    try:
        j0, m0 = lib.sg_modconv_jvp_launches(), lib.sg_modconv_launches()
        with style_ops.second_order(generator=True):
            dx, ds = torch.autograd.grad(y, [xd, sd], gyd, create_graph=True)
        assert dx.requires_grad and ds.requires_grad
        assert wgrads == [], "the first pass under inputs=[x, s] launches no weight gradient"
        assert lib.sg_modconv_jvp_launches() == j0 and lib.sg_modconv_launches() - m0 == 1, "the first pass: the data-gradient launch alone"
        vxd, vsd = vx.to(dev, dtype), vs.to(dev, torch.float32)
        m1 = lib.sg_modconv_launches()
        got = torch.autograd.grad((dx.float() * vxd.float()).sum() + (ds * vsd).sum(), [gyd, xd, sd, wd])     # (outside the context: the graph stays valid)
        assert lib.sg_modconv_jvp_launches() - j0 == (1 if fused else 0), "one sg_modconv2d_jvp launch per second-order pass on the fused route, none on the other"
        # the forward kernel's launches of the pass: G' through the data-gradient route (with demodulation), and the composition's own
        assert lib.sg_modconv_launches() - m1 == (1 if demod else 0) + (0 if fused else 1)
        assert len(wgrads) == (2 if demod else 1), "the weight's second-order gradient: two weight-gradient launches (one without demodulation)"
    finally:
        MC.conv2d_wgrad_raw, MC.TANGENT_ROUTE[0] = raw, saved_route
    name = f"modconv2 {tag}{' gain' if gain is not None else ''} {dtype_name(dtype)} {route or 'rule'}{'' if route else ' = fused' if fused else ' = composition'}"
    check(f"{name} dx", dx, edx, tol, report)
    check(f"{name} ds", ds, eds, tol, report)
    for what, a, e in zip(("d_gy", "d_x", "d_s", "d_w"), got, want):
        assert a.dtype == (dtype if what in ("d_gy", "d_x") else torch.float32) and tuple(a.shape) == tuple(e.shape), what
        check(f"{name} {what}", a, e, tol, report)
    assert_pairing(f"{name} <vx,dx>+<vs,ds> = <d_gy,gy>", [(vxd, dx), (vsd, ds)], [(got[0], gyd)], tol)


def check_tangent_rule(lib, dev, report=None):
    """the default route is the measured one (profiles/stylegan2_pl_bench.txt): the one launch in fp32 at up = 1, the composition at up = 2 and in bf16"""
    from studiogan_amd.style_ops import modulated_conv2d as MC
    assert MC.TANGENT_ROUTE[0] is None
    table = {(dt, up): MC.tangent_fused(dt, up) for dt in (torch.float32, torch.bfloat16) for up in (1, 2)}
    assert table == {(torch.float32, 1): True, (torch.float32, 2): False, (torch.bfloat16, 1): False, (torch.bfloat16, 2): False}
    for tag, dtype in (("b", torch.float32), ("e", torch.float32), ("b", torch.bfloat16)):
        check_modconv_second_order(lib, dev, tag, dtype, report, route=None)


def check_modconv_refuses_weight_cotangent(dev):
    """a cotangent on dW (or dnoise) is no path of the regulariser: the grad-function refuses it by name"""
    import pytest
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d
    x, w, s, nz, gy = R.exact_inputs(6400, 2, 8, 8, 5, 3, 1, "sample")
    xd, wd, sd = (t.to(dev, torch.float32).requires_grad_(True) for t in (x, w, s))
    nd = nz.to(dev, torch.float32).requires_grad_(True)
    y = modulated_conv2d(xd, wd, sd, noise=nd, padding=1)
    with style_ops.second_order(generator=True):
        dw, dn = torch.autograd.grad(y, [wd, nd], gy.to(dev, torch.float32), create_graph=True)
    for g in (dw, dn):
        with pytest.raises(NotImplementedError, match="cotangent"):
            torch.autograd.grad(g.square().sum(), [xd], retain_graph=True)


# ---- fir_bias_act -------------------------------------------------------------------------------------------------------------------------------------------

def tail_case(shape, noise, dtype):
    """(core, noise, bias, gy, vx, vn, vb): the [2H+1]^2 core of a fused-tail case of tests/stylegan2_ref.py on the 2^-6 grid, cotangents likewise"""
    x, w, s, nz, bias, gy = S.tail_inputs(shape, noise)
    N, C = s.shape
    d = (s.square() @ w.square().sum(dim=(2, 3)).t() + 1e-8).rsqrt()
    core = S.up2_core(x * s.reshape(N, C, 1, 1), w) * d.reshape(N, -1, 1, 1)
    core = ((core * 64).round() / 64).clamp(-8, 8)
    seed = 6500 + 10 * list(S.TAIL_SHAPES).index(shape) + S.TAIL_NOISE.index(noise)
    vx, vb = grid(seed, *core.shape), grid(seed + 1, *bias.shape)
    vn = None if nz is None else grid(seed + 2, *nz.shape)
    return core, nz, bias, gy, vx, vn, vb


def tail_second_order_ref(core, nz, bias, gy, vx, vn, vb, act, gain, clamp_, dtype):
    """fp64 autograd of clamp(gain act(FIR(core) + noise + bias)) with the sides decided as the operator decides them, from the STORED output (rounded to
    dtype): positive side where y > 0, the clamp passing where |y| < clamp. -> (dx, d_dy)"""
    core, gy, bias = (t.detach().clone().requires_grad_(True) for t in (core, gy, bias))
    nzl = None if nz is None else nz.detach().clone().requires_grad_(True)
    f = R.low_pass().double()

    def forward(mask=None, inside=None):
        pre = S.fir_up2(core, f) + (0 if nzl is None else nzl) + bias.reshape(1, -1, 1, 1)
        a = (S.lrelu(pre, mask) if act == "lrelu" else pre) * gain
        if clamp_ is None:
            return a
        return a.clamp(-clamp_, clamp_) if inside is None else torch.where(inside, a, a.detach().clamp(-clamp_, clamp_))
    stored = forward().detach().to(dtype).double()
    y = forward(stored > 0, None if clamp_ is None else stored.abs() < clamp_)
    leaves = [core, bias] + ([nzl] if nzl is not None else [])
    first = torch.autograd.grad(y, leaves, gy, create_graph=True)
    psi = (first[0] * vx).sum() + (first[1] * vb).sum() + ((first[2] * vn).sum() if nzl is not None else 0)
    (d_dy,) = torch.autograd.grad(psi, gy)
    return first[0].detach(), d_dy


def check_tail_second_order(lib, dev, shape, noise, epi, dtype, report=None):
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops.fir_bias_act import fir_bias_act, fir_nhwc_raw
    act, gain, clamp_ = TAIL_EPI[epi]
    core, nz, bias, gy, vx, vn, vb = tail_case(shape, noise, dtype)
    tol = tol_of(dtype)
    edx, edd = tail_second_order_ref(_rb(core, dtype), nz, bias, _rb(gy, dtype), _rb(vx, dtype), vn, vb, act, gain, clamp_, dtype)
    f = R.low_pass().to(dev)
    cd = core.to(dev, dtype).contiguous(memory_format=CL).requires_grad_(True)
    gyd = gy.to(dev, dtype).requires_grad_(True)
    bd = bias.to(dev, torch.float32).requires_grad_(True)
    nd = None if nz is None else nz.to(dev, torch.float32).requires_grad_(True)
    leaves = [cd, bd] + ([nd] if nd is not None else [])
    n0 = lib.sg_fir_bias_act_launches()
    y = fir_bias_act(cd, f, [1, 1, 1, 1], noise=nd, bias=bd, act=act, gain=gain, clamp=clamp_, filter_gain=4.0)
    with style_ops.second_order(generator=True):
        first = torch.autograd.grad(y, leaves, gyd, create_graph=True)
    assert all(g.requires_grad for g in first) and lib.sg_fir_bias_act_launches() - n0 == 2
    vxd, vbd = vx.to(dev, dtype), vb.to(dev, torch.float32)
    terms = [(vxd, first[0]), (vbd, first[1])] + ([(vn.to(dev, torch.float32), first[2])] if nd is not None else [])
    psi = sum((a.float() * b.float()).sum() for a, b in terms)
    got = torch.autograd.grad(psi, [gyd] + leaves, allow_unused=True, retain_graph=epi == "linear")
    assert lib.sg_fir_bias_act_launches() - n0 == 3, "the second-order pass of the tail is one launch"
    assert all(g is None or float(g.abs().max()) == 0 for g in got[1:]), "the activation is piecewise linear: nothing flows to x, the bias or the noise"
    d_dy = got[0]
    assert d_dy.dtype == dtype and tuple(d_dy.shape) == tuple(gy.shape)
    name = f"tail2 {shape} noise={noise} {epi} {dtype_name(dtype)}"
    check(f"{name} dx", first[0], edx, tol, report)
    check(f"{name} d_dy", d_dy, edd, tol, report)
    assert_pairing(f"{name} <v,d(gy)> = <d_dy,gy>", terms, [(d_dy, gyd)], tol)
    if epi == "linear":         # no gate: the launch with the core's cotangent alone IS the plain launch, bit for bit
        (plain,) = torch.autograd.grad((first[0].float() * vxd.float()).sum(), [gyd])
        want = fir_nhwc_raw(vxd.permute(0, 2, 3, 1).contiguous(), f, (1, 1, 1, 1), filter_gain=4.0).permute(0, 3, 1, 2)
        assert torch.equal(plain, want), name


# ---- the context --------------------------------------------------------------------------------------------------------------------------------------------

def check_context_flags():
    """second_order(generator=True) lifts the two generator names on a counter of its own, restores on exit and on exceptions; a plain second_order() does not"""
    import pytest
    from studiogan_amd import style_ops
    from studiogan_amd.functional import _base as B
    gen, dis = ("modulated_conv2d", "fir_bias_act"), ("act_fir", "conv2d_resample", "minibatch_std")
    assert B._SECOND_ORDER[0] == 0 and B._SECOND_ORDER_GEN[0] == 0
    with style_ops.second_order(generator=True):
        assert B._SECOND_ORDER_GEN[0] == 1
        assert all(B._first_order_only(n) is True for n in gen + dis)
        with style_ops.second_order():          # a plain one inside: the generator's depth is untouched
            assert B._SECOND_ORDER_GEN[0] == 1 and all(B._first_order_only(n) is True for n in gen)
        with style_ops.second_order(generator=True):        # re-entrant
            assert B._SECOND_ORDER_GEN[0] == 2
        assert B._SECOND_ORDER_GEN[0] == 1
        for name in ("modulated_conv2d (third order)", "fir_bias_act (third order)", "ConvTransposeFn", "filtered_lrelu"):
            with pytest.raises(NotImplementedError, match="create_graph"):
                B._first_order_only(name)
        with torch.no_grad():
            assert B._first_order_only("modulated_conv2d") is False
    assert B._SECOND_ORDER[0] == 0 and B._SECOND_ORDER_GEN[0] == 0
    with pytest.raises(ZeroDivisionError):
        with style_ops.second_order(generator=True):
            1 / 0
    assert B._SECOND_ORDER[0] == 0 and B._SECOND_ORDER_GEN[0] == 0
    with style_ops.second_order():
        assert B._SECOND_ORDER[0] == 1 and B._SECOND_ORDER_GEN[0] == 0
        for name in gen:
            with pytest.raises(NotImplementedError, match="create_graph"):
                B._first_order_only(name)
    for name in gen:
        with pytest.raises(NotImplementedError, match="create_graph"):
            B._first_order_only(name)


def check_refusals(dev):
    """through the operators: a bare create_graph=True and a plain second_order() refuse, second_order(generator=True) records, third order refuses"""
    import pytest
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops.fir_bias_act import fir_bias_act
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d
    new = lambda seed, *s: grid(seed, *s).to(dev, torch.float32).requires_grad_(True)      # noqa: E731
    w, s = new(6601, 4, 4, 3, 3), new(6602, 2, 4)
    ops = {"modulated_conv2d": lambda t: modulated_conv2d(t, w, s, padding=1),
           "fir_bias_act": lambda t: fir_bias_act(t, R.low_pass().to(dev), [1, 1, 1, 1], bias=torch.ones(4, device=dev), act="lrelu")}
    for name, op in ops.items():
        x = new(6603, 2, 4, 5, 5)
        with pytest.raises(NotImplementedError, match=name):
            torch.autograd.grad(op(x).square().sum(), x, create_graph=True)
        with style_ops.second_order():
            with pytest.raises(NotImplementedError, match=name):
                torch.autograd.grad(op(x).square().sum(), x, create_graph=True)
        with style_ops.second_order(generator=True):
            (g,) = torch.autograd.grad(op(x).square().sum(), x, create_graph=True)
            assert g.requires_grad, name
            with pytest.raises(NotImplementedError, match="third order"):
                torch.autograd.grad(g.square().sum(), x, create_graph=True)
        (g,) = torch.autograd.grad(op(x).square().sum(), x)         # first order is untouched
        assert not g.requires_grad


# ---- the networks -------------------------------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def bias_act_on_the_interpreter():
    """style_ops.bias_act checks for a GPU tensor by itself, not through the gate tests/hipemu/fullemu.py opens (tests/test_stylegan3_cpu.py relies on that
    refusal), so a whole generator does not run on the interpreter as it stands. For the CPU runs of the network checks its launcher is rebound to ITS OWN
    SOURCE without that one statement; everything else of the operator, the sg_bias_act kernel included, is the product's."""
    from studiogan_amd.style_ops import bias_act as BA
    saved = BA._launch
    src = inspect.getsource(saved)
    gate = "if not x.is_cuda:"
    assert src.count(gate) == 1
    exec(compile(src.replace(gate, "if False:"), BA.__file__, "exec"), BA.__dict__)
    try:
        yield
    finally:
        BA._launch = saved


def load_fixtures():
    import make_golden_stylegan2_pl as M
    t = lambda z: {k: (torch.from_numpy(v) if v.dtype.kind in "fi" else v) for k, v in z.items()}      # noqa: E731
    return t(S.load_golden()), t(M.load_golden())


def state(gen, tag):
    return {k: gen[f"{tag}/sd/{k}"].float() for k in (str(k) for k in gen[f"{tag}/keys"])}


def generator(gen, tag, dev, **extra):
    from studiogan_amd.backbones import stylegan2 as SG
    G = SG.Generator(**S.kwargs_of(S.CASES[tag], **extra))
    G.load_state_dict(state(gen, tag), strict=True)
    return G.to(dev)


def bound(pl, tag, what):
    return max(2e-5, 4 * float(pl[f"{tag}/ref32_err/{what}"]))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def labels_of(pl, tag, dev):
    c = pl[f"{tag}/c"]
    return c.argmax(dim=1).to(dev) if c.shape[1] > 0 else torch.zeros(c.shape[0], dtype=torch.int64, device=dev)


def pl_step(lib, G, pl, tag, dev):
    """(loss, pl_lengths, regulariser) through losses.PathLengthRegularizer on the fixture's latents and noise; the loss's backward has run. One
    sg_modconv2d_jvp launch per modulated convolution, all of them in the loss's backward."""
    from studiogan_amd import losses
    from studiogan_amd.functional import _base as B
    from studiogan_amd.style_ops import modulated_conv2d as MC
    import make_golden_stylegan2_pl as M
    z, noise = pl[f"{tag}/z"].to(dev), pl[f"{tag}/pl_noise"].to(dev)
    c = torch.nn.functional.one_hot(labels_of(pl, tag, dev), S.CASES[tag]["c_dim"]) if S.CASES[tag]["c_dim"] else None
    reg = losses.PathLengthRegularizer(dev, pl_decay=M.PL_DECAY, pl_weight=M.PL_WEIGHT, pl_no_weight_grad=True)
    ws = G.mapping(z, c)
    m0 = lib.sg_modconv_launches()
    img = G.synthesis(ws, noise_mode="const")
    convs = lib.sg_modconv_launches() - m0
    assert convs >= len(G.synthesis.style_layers())
    (g,) = torch.autograd.grad((img * noise).sum(), ws, retain_graph=True)       # (the plain first-order gradient: what the lengths are the norms of)
    lengths = g.square().sum(2).mean(1).sqrt()
    j0 = lib.sg_modconv_jvp_launches()
    loss = reg.cal_pl_reg(fake_images=img, ws=ws, pl_noise=noise)
    assert loss.requires_grad and loss.dim() == 0 and B._SECOND_ORDER[0] == 0 and B._SECOND_ORDER_GEN[0] == 0
    assert lib.sg_modconv_jvp_launches() == j0
    routes, rule = [], MC.tangent_fused
    MC.tangent_fused = lambda dtype, up: (routes.append(rule(dtype, up)), routes[-1])[1]
    try:
        loss.backward()
    finally:
        MC.tangent_fused = rule
    assert len(routes) == convs, "one second-order pass per modulated convolution (a resnet block's skip is one, with unit styles)"
    assert lib.sg_modconv_jvp_launches() - j0 == sum(routes), "one tangent launch per convolution the rule gives it to"
    assert any(routes) and not all(routes), "the fp32 up = 1 layers take the one launch, the up = 2 layers the composition"
    return loss.detach(), lengths, reg


def check_network_fp32(lib, dev, fix, tag, report=None):
    gen, pl = fix
    G = generator(gen, tag, dev)
    loss, lengths, reg = pl_step(lib, G, pl, tag, dev)
    what = lambda k: f"pl {tag} {k} (ref32_err {float(pl[f'{tag}/ref32_err/{k}']):.1e})"      # noqa: E731
    check(what("pl_lengths"), lengths, pl[f"{tag}/pl_lengths"], bound(pl, tag, "pl_lengths"), report)
    check(what("loss"), loss, pl[f"{tag}/loss"], bound(pl, tag, "loss"), report)
    check(what("pl_mean"), reg.pl_mean, pl[f"{tag}/pl_mean"], bound(pl, tag, "pl_mean"), report)
    params = dict(G.named_parameters())
    assert list(params) == [k[len(tag) + 4:] for k in pl if k.startswith(f"{tag}/dp/")]
    zeros = 0
    for k, p in params.items():
        e = pl[f"{tag}/dp/{k}"]
        if float(e.abs().max()) == 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0, k
            zeros += 1
            continue
        check(what(f"dp/{k}"), p.grad, e, bound(pl, tag, f"dp/{k}"), report)
    assert zeros >= 1 and all(params[k].grad is not None for k in params if k.startswith("mapping.")), "the mapping network is part of the loss's graph"


def check_network_bf16(lib, dev, fix, tag, report=None):
    """blocks b8 and b16 in bf16 (conv_clamp 256) against fp64 with the clamp: each quantity at 3 x its share of bf16_floor (none larger than the fixture's
    bf16_floor), the parameter gradients in relative L2 per tensor. No element is excused: the floor comes from an emulation that already differs from fp64 on
    some leaky-ReLU sides (tests/make_golden_stylegan2_pl.py), so it carries what a moved side costs. A parameter of ONE element (the noise strengths) is held
    to 3 x bf16_floor itself: the relative error of a single number is one draw, and the emulation's own draw says nothing about its scale (the five noise
    strengths' shares run from 2.0e-3 to 1.6e-1 for the same kind of sum); their peers' largest share is bf16_floor.
    Through the interpreter the two smallest of them sit at 1.5e-2 and 1.7e-2, the level of every multi-element tensor's share."""
    gen, pl = fix
    G = generator(gen, tag, dev, **S.LOWP)
    acts = {}
    hook = G.synthesis.b16.register_forward_hook(lambda m, i, o: acts.__setitem__(16, o[0]))
    loss, lengths, reg = pl_step(lib, G, pl, tag, dev)
    hook.remove()
    assert acts[16].dtype == torch.bfloat16
    floor = lambda k: float(pl[f"{tag}/bf16_floor_of/{k}"])      # noqa: E731
    assert all(floor(k[len(tag) + 15:]) <= float(pl[f"{tag}/bf16_floor"]) for k in pl if k.startswith(f"{tag}/bf16_floor_of/"))
    name = f"pl {tag} bf16 blocks"
    check(f"{name} pl_lengths (floor {floor('pl_lengths'):.1e})", lengths, pl[f"{tag}/lowp/pl_lengths"], 3 * floor("pl_lengths"), report)
    check(f"{name} loss (floor {floor('loss'):.1e})", loss, pl[f"{tag}/lowp/loss"], 3 * floor("loss"), report)
    check(f"{name} pl_mean (floor {floor('pl_mean'):.1e})", reg.pl_mean, pl[f"{tag}/lowp/pl_mean"], 3 * floor("pl_mean"), report)
    bad = []
    for k, p in G.named_parameters():
        e = pl[f"{tag}/lowp/dp/{k}"]
        if float(e.abs().max()) == 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0, k
            continue
        assert bool(torch.isfinite(p.grad).all()), k
        share = floor(f"dp/{k}") if e.numel() > 1 else float(pl[f"{tag}/bf16_floor"])
        d, t = rel_l2(p.grad, e), 3 * share
        line = f"{name} dp/{k} (floor {share:.1e})"
        print(f"{line:48s} l2err={d:.3e} tol={t:.1e} {'ok' if d <= t else 'FAIL'}")
        if report is not None:
            report.append((line + " [rel L2]", d, t))
        bad.append(line) if d > t else None
    assert not bad, bad


def check_g_reg_step(lib, dev, fix, report=None, tag="orig", g_reg_interval=4):
    """losses.stylegan_g_reg_step leaves g_reg_interval x the loss's gradients in .grad (the bound scales with the expectation), returns the detached scaled
    loss, accumulates with acml_steps, and gives the output bias the loss does not reach a ZERO gradient (the `+ fake_images[:, 0, 0, 0].mean() * 0` term),
    not none"""
    from studiogan_amd import losses
    import make_golden_stylegan2_pl as M
    gen, pl = fix
    G = generator(gen, tag, dev)
    z, noise, labels = pl[f"{tag}/z"].to(dev), pl[f"{tag}/pl_noise"].to(dev), labels_of(pl, tag, dev)
    reg = losses.PathLengthRegularizer(dev, pl_decay=M.PL_DECAY, pl_weight=M.PL_WEIGHT, pl_no_weight_grad=True)
    value = losses.stylegan_g_reg_step(G, z, labels, reg, g_reg_interval, pl_noise=noise, noise_mode="const")
    assert not value.requires_grad and value.grad_fn is None
    check(f"g_reg_step {tag} loss", value, pl[f"{tag}/loss"] * g_reg_interval, bound(pl, tag, "loss"), report)
    check(f"g_reg_step {tag} pl_mean", reg.pl_mean, pl[f"{tag}/pl_mean"], bound(pl, tag, "pl_mean"), report)
    reg.pl_mean.zero_()         # (the same step once more, half as much on top)
    losses.stylegan_g_reg_step(G, z, labels, reg, g_reg_interval, acml_steps=2, pl_noise=noise, noise_mode="const")
    for k, p in G.named_parameters():
        e = pl[f"{tag}/dp/{k}"] * (g_reg_interval * 1.5)
        assert p.grad is not None, k
        if float(e.abs().max()) == 0:
            assert float(p.grad.abs().max()) == 0, k
            continue
        check(f"g_reg_step {tag} dp/{k}", p.grad, e, bound(pl, tag, f"dp/{k}"), report)


def check_style_mixing(dev, fix, tag="skip"):
    """losses.stylegan_generate_images against a torch restatement of its three mixing lines under the same generator seed (the cutoff and the coin are drawn on
    the tensors' device, then the second latents); p = 0 leaves ws untouched; truncation_psi = -1 is no truncation"""
    from studiogan_amd import losses
    gen, pl = fix
    G = generator(gen, tag, dev)
    z, labels, ncls = pl[f"{tag}/z"].to(dev), labels_of(pl, tag, dev), S.CASES[tag]["c_dim"]
    synthesis = lambda ws, **kw: G.synthesis(ws, noise_mode="const", **kw)      # noqa: E731
    with torch.no_grad():
        c = torch.nn.functional.one_hot(labels, ncls)
        plain = G.mapping(z, c)
        ws0, img0 = losses.stylegan_generate_images(z, labels, ncls, 0.0, False, G.mapping, synthesis, -1, None)
        assert torch.equal(ws0, plain) and torch.equal(img0, synthesis(plain))
        wt, _ = losses.stylegan_generate_images(z, labels, ncls, 0.0, False, G.mapping, synthesis, 0.7, 2)
        assert torch.equal(wt, G.mapping(z, c, truncation_psi=0.7, truncation_cutoff=2)) and not torch.equal(wt, plain)
        cut = set()
        for seed in range(6):
            torch.manual_seed(900 + seed)
            ws, img = losses.stylegan_generate_images(z, labels, ncls, 0.9, False, G.mapping, synthesis, -1, None)
            torch.manual_seed(900 + seed)
            cutoff = torch.empty([], dtype=torch.int64, device=dev).random_(1, plain.shape[1])
            cutoff = torch.where(torch.rand([], device=dev) < 0.9, cutoff, torch.full_like(cutoff, plain.shape[1]))
            second = G.mapping(torch.randn_like(z), c)
            k = int(cutoff)
            assert torch.equal(ws, torch.cat([plain[:, :k], second[:, k:]], dim=1)) and torch.equal(img, synthesis(ws)), seed
            cut.add(k)
        assert len(cut) > 1 and min(cut) >= 1
