"""The checks of R1 through the StyleGAN2 discriminator that tests/test_stylegan2_r1_cpu.py runs through the kernel-source interpreter and
tests/test_stylegan2_r1_gpu.py on the device: one statement of each, `dev` says where the tensors live. Expectations are fp64 autograd of the restatement
(tests/stylegan2_dis_ref.py) or of torch's own operators; the networks' come from tests/golden/stylegan2_r1.npz. TEST INFRASTRUCTURE ONLY."""
import torch
import torch.nn.functional as F

import modconv_ref as R
import stylegan2_dis_ref as D
from util import check

CL = torch.channels_last
MBSTD_R1_CASES = ("g2f1", "g3", "all", "split")
CONV_GEOMS = [(1, 1), (3, 1), (3, 2)]       # (kernel, stride)
CONV_CHANNELS = (3, 12, 25)


def dtype_name(dtype):
    return "fp32" if dtype == torch.float32 else "bf16"


def tol_of(dtype):
    return 2e-5 if dtype == torch.float32 else 1e-2


def err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def grid(seed, *shape):
    """a seeded tensor on the 2^-6 grid below 3 (bf16 holds every value)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * 64).round().clamp(-192, 192) / 64


def load_fixtures():
    import make_golden_stylegan2_r1 as M
    t = lambda z: {k: (torch.from_numpy(v) if v.dtype.kind in "fi" else v) for k, v in z.items()}      # noqa: E731
    return t(D.load_golden()), t(M.load_golden())


def state(dis, tag):
    return {k: dis[f"{tag}/sd/{k}"].float() for k in (str(k) for k in dis[f"{tag}/keys"])}


def param_keys(dis, tag):
    return [k[len(tag) + 4:] for k in dis if k.startswith(f"{tag}/dp/")]


# ---- the head of a down layer -----------------------------------------------------------------------------------------------------------------------------

def head_second_order_ref(x, bias, gy, v, pad, down, epi):
    """fp64: (dx, d_dy) with dx = d<act_fir(x), gy>/dx and d_dy = d<dx, v>/dgy"""
    e = D.HEAD_EPI[epi]
    x = x.clone().requires_grad_(True)
    gy = gy.clone().requires_grad_(True)
    y = D.act_fir(x, R.low_pass().double(), D.HEAD_PADS[pad], down, bias if e["bias"] else None, e["act"], e["gain"], e["clamp_"])
    (dx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    (d_dy,) = torch.autograd.grad(dx, gy, v)
    return dx.detach(), d_dy


def check_head_second_order(lib, dev, shape, down, dtype, report=None):
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops.act_fir import act_fir
    from studiogan_amd.style_ops.upfirdn2d import upfirdn2d
    f, tol = R.low_pass().to(dev), tol_of(dtype)
    for pad in D.HEAD_PADS:
        for epi, e in D.HEAD_EPI.items():
            x, bias, gy = D.head_inputs(shape, pad, down)
            D.head_ref(x, bias, gy, pad, down, epi)         # (asserts the margins: no pre-activation at 0, none near the clamp, the clamp bites)
            v = grid(5200 + down, *x.shape)
            edx, edd = head_second_order_ref(x, bias, gy, v, pad, down, epi)
            xd = x.to(dev, dtype).contiguous(memory_format=CL).requires_grad_(True)
            gyd = gy.to(dev, dtype).contiguous(memory_format=CL).requires_grad_(True)
            bd = bias.to(dev, torch.float32).requires_grad_(True) if e["bias"] else None
            n0 = lib.sg_act_fir_launches()
            y = act_fir(xd, f, list(D.HEAD_PADS[pad]), down=down, bias=bd, act=e["act"], gain=e["gain"], clamp=e["clamp_"])
            with style_ops.second_order():
                (dx,) = torch.autograd.grad(y, xd, gyd, create_graph=True)
            assert dx.requires_grad and lib.sg_act_fir_launches() - n0 == 2
            got = torch.autograd.grad(dx, [gyd, xd] + ([bd] if bd is not None else []), v.to(dev, dtype), allow_unused=True)
            assert lib.sg_act_fir_launches() - n0 == 3, "the second-order pass of the head is one launch"
            d_dy = got[0]
            assert all(g is None or float(g.abs().max()) == 0 for g in got[1:]), "the activation is piecewise linear: no second-order term for x or the bias"
            assert d_dy.dtype == dtype and tuple(d_dy.shape) == tuple(gy.shape)
            tag = f"head2 {shape} down={down} {pad} {epi} {dtype_name(dtype)}"
            check(f"{tag} dx", dx, edx, tol, report)
            check(f"{tag} d_dy", d_dy, edd, tol, report)
            if epi == "plain":      # no gate: the launch IS upfirdn2d of the cotangent on the NCHW copy, bit for bit
                yu = upfirdn2d(v.to(dev, dtype), f, down=down, padding=list(D.HEAD_PADS[pad]))
                assert torch.equal(yu, d_dy.contiguous()), tag


def check_gate_border(dev, down, report=None):
    """The mirror of the forward's border rule. The forward pads the ACTIVATED map with zeros; the gate pass pads v * da/dx with zeros, and must not evaluate a
    gate outside the image at all: there is no x there, and 0 * gate(whatever the address holds) is NaN for a non-finite read. With the bias whose activation
    would move the forward's border by O(1), on the shape whose every output touches the padding: the result is the fp64 one, finite, and the adjoint of the
    first-order pass (<v, dx(gy)> = <d_dy(v), gy>), which a border handled differently in the two launches would break."""
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops.act_fir import act_fir
    x, _, gy = D.head_inputs("edge", "p2", down)
    bias = torch.full((x.shape[1],), 1.5 + 2.0 ** -7, dtype=torch.float64)
    v = grid(5300 + down, *x.shape)
    x64, gy64 = x.clone().requires_grad_(True), gy.clone().requires_grad_(True)
    y64 = D.act_fir(x64, R.low_pass().double(), (2, 2, 2, 2), down, bias, "lrelu", D.SQRT2, None)
    (dx64,) = torch.autograd.grad(y64, x64, gy64, create_graph=True)
    (want,) = torch.autograd.grad(dx64, gy64, v)
    xd = x.to(dev, torch.float32).contiguous(memory_format=CL).requires_grad_(True)
    gyd = gy.to(dev, torch.float32).requires_grad_(True)
    y = act_fir(xd, R.low_pass().to(dev), [2, 2, 2, 2], down=down, bias=bias.to(dev, torch.float32), act="lrelu")
    with style_ops.second_order():
        (dx,) = torch.autograd.grad(y, xd, gyd, create_graph=True)
    (d_dy,) = torch.autograd.grad(dx, gyd, v.to(dev, torch.float32))
    assert bool(torch.isfinite(d_dy).all())
    check(f"head2 border down={down}", d_dy, want, 2e-5, report)
    lhs, rhs = float((v * dx.detach().double().cpu()).sum()), float((d_dy.double().cpu() * gy).sum())
    assert abs(lhs - rhs) <= 2e-5 * max(abs(lhs), float(v.abs().max() * dx.detach().abs().max())), (lhs, rhs)


# ---- minibatch standard deviation -------------------------------------------------------------------------------------------------------------------------

def mbstd_second_order_ref(x, gy, v, group, nch):
    x, gy = x.clone().requires_grad_(True), gy.clone().requires_grad_(True)
    (dx,) = torch.autograd.grad(D.minibatch_std(x, group, nch), x, gy, create_graph=True)
    d_dout, d_x = torch.autograd.grad(dx, [gy, x], v)
    return dx.detach(), d_dout, d_x


def check_mbstd_second_order(lib, dev, case, report=None):
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops.minibatch_std import minibatch_std
    N, C, H, W, group, nch = D.MBSTD_CASES[case]
    assert (lib.sg_mbstd_splits(N, H, W, C, N if group is None else min(group, N), nch) > 1) == (case == "split"), "the chunked path is the `split` case's"
    for constant in ((False, True) if case == "g2f1" else (False,)):
        x, gy = D.mbstd_inputs(case, constant)
        v = grid(5400 + N, *x.shape)
        edx, edd, ex = mbstd_second_order_ref(x, gy, v, group, nch)
        xd = x.to(dev, torch.float32).contiguous(memory_format=CL).requires_grad_(True)
        gyd = gy.to(dev, torch.float32).requires_grad_(True)
        n0 = lib.sg_mbstd_launches()
        out = minibatch_std(xd, group, nch)
        with style_ops.second_order():
            (dx,) = torch.autograd.grad(out, xd, gyd, create_graph=True)
        d_dout, d_x = torch.autograd.grad(dx, [gyd, xd], v.to(dev, torch.float32), retain_graph=case == "split")
        assert lib.sg_mbstd_launches() - n0 == 3, "forward, backward and the second-order pass are one launch each"
        tag = f"mbstd2 {case}{' constant groups' if constant else ''}"
        assert bool(torch.isfinite(d_dout).all()) and bool(torch.isfinite(d_x).all()), tag
        assert torch.equal(d_dout[:, :C].cpu(), v.float()), "the pass-through channels' cotangent is v itself"
        check(f"{tag} dx", dx, edx, 2e-5, report)
        check(f"{tag} d_dout", d_dout, edd, 2e-5, report)
        check(f"{tag} d_x", d_x, ex, 2e-5, report)
        if case == "split":     # deterministic: the hand-over adds the chunks' sums in chunk order, whoever arrived when
            again = torch.autograd.grad(dx, [gyd, xd], v.to(dev, torch.float32))
            assert torch.equal(again[0], d_dout) and torch.equal(again[1], d_x)


# ---- the plain convolutions -------------------------------------------------------------------------------------------------------------------------------

def check_conv_second_order(dev, geom, C, dtype, report=None):
    """conv2d_plain's double backward against F.conv2d's in fp64 (operands on grids both dtypes hold); -> the convolution entries that ran"""
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops import conv2d_resample as CR
    k, s = geom
    Cout, tol = 6, tol_of(dtype)
    g = torch.Generator().manual_seed(700 + 10 * C + k + s)
    q = lambda *sh, d=64: (torch.randn(*sh, generator=g, dtype=torch.float64) * d).round().clamp(-3 * d, 3 * d) / d      # noqa: E731
    x, w = q(2, C, 7, 5, d=16), q(Cout, C, k, k, d=16) / 4
    x64, w64 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y64 = F.conv2d(x64, w64, stride=s, padding=k // 2 if s == 1 else 0)
    gy, v, vw = q(*y64.shape, d=16), q(*x.shape, d=16), q(*w.shape, d=16)
    gy64 = gy.clone().requires_grad_(True)
    dx64, dw64 = torch.autograd.grad(y64, [x64, w64], gy64, create_graph=True)
    want = torch.autograd.grad((dx64 * v).sum() + (dw64 * vw).sum(), [gy64, w64, x64])
    xd = x.to(dev, dtype).contiguous(memory_format=CL).requires_grad_(True)
    wd = w.to(dev, torch.float32).requires_grad_(True)
    gyd = gy.to(dev, dtype).requires_grad_(True)
    with CR.record() as log:
        y = CR.conv2d_plain(xd, wd, s)
        with style_ops.second_order():
            dx, dw = torch.autograd.grad(y, [xd, wd], gyd, create_graph=True)
        assert [r[0] for r in log] == ["fwd", "dgrad", "wgrad"]
        got = torch.autograd.grad((dx.float() * v.to(dev, torch.float32)).sum() + (dw * vw.to(dev, torch.float32)).sum(), [gyd, wd, xd])
        assert sorted(r[0] for r in log[3:]) == ["dgrad2", "dgrad2", "dgrad2", "wgrad2"], log
    tag = f"conv2 k={k} s={s} C={C} {dtype_name(dtype)}"
    check(f"{tag} dx", dx, dx64.detach(), tol, report)
    check(f"{tag} dw", dw, dw64.detach(), tol, report)
    for what, a, b in zip(("d_gy", "d_w", "d_x"), got, want):
        check(f"{tag} {what}", a, b, tol, report)
    return {r[1] for r in log if r[0] == "fwd"}


def check_no_weight_gradient_in_the_first_pass(lib, dev, monkeypatch):
    """conv -> head -> stride-2 conv -> minibatch std: autograd.grad(inputs=[images]) inside the context launches the two data gradients and no weight
    gradient (the reference's no_weight_gradients); the penalty's backward launches them"""
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops import conv2d_resample as CR
    from studiogan_amd.style_ops.act_fir import act_fir
    from studiogan_amd.style_ops.minibatch_std import minibatch_std
    calls = []
    raw = CR.conv2d_wgrad_raw
    monkeypatch.setattr(CR, "conv2d_wgrad_raw", lambda *a, **k: (calls.append(1), raw(*a, **k))[1])
    x = grid(81, 4, 12, 8, 8).to(dev, torch.float32).contiguous(memory_format=CL).requires_grad_(True)
    w0 = torch.nn.Parameter((grid(82, 12, 12, 3, 3) / 8).to(dev, torch.float32))
    w1 = torch.nn.Parameter((grid(83, 8, 12, 3, 3) / 8).to(dev, torch.float32))
    b0 = torch.nn.Parameter((grid(84, 12) + 2.0 ** -7).to(dev, torch.float32))
    with CR.record() as log:
        t = act_fir(CR.conv2d_plain(x, w0 * 0.5, 1), R.low_pass().to(dev), [2, 2, 2, 2], bias=b0, act="lrelu")
        out = minibatch_std(CR.conv2d_plain(t, w1 * 0.5, 2), 2, 1)
        adv = (out * grid(85, *out.shape).to(dev, torch.float32)).sum()
        n0 = len(log)
        with style_ops.second_order():
            (g,) = torch.autograd.grad(adv, [x], create_graph=True)
        assert calls == [] and [r[0] for r in log[n0:]] == ["dgrad", "dgrad"], (calls, log[n0:])
        penalty = g.square().sum([1, 2, 3]).mean() / 2
        n1 = len(log)
        penalty.backward()
        roles = [r[0] for r in log[n1:]]
    assert roles.count("wgrad2") == 2 and "dgrad2" in roles, roles
    assert len(calls) >= 2 and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in (w0, w1, b0))
    assert float(w0.grad.abs().max()) > 0 and float(w1.grad.abs().max()) > 0


def check_refusals(dev):
    """outside the context the three operators keep refusing create_graph; inside it modulated_conv2d does, and so does third order"""
    import pytest
    from studiogan_amd import style_ops
    from studiogan_amd.style_ops.act_fir import act_fir
    from studiogan_amd.style_ops.conv2d_resample import conv2d_plain
    from studiogan_amd.style_ops.minibatch_std import minibatch_std
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d
    new = lambda seed, *s: grid(seed, *s).to(dev, torch.float32).requires_grad_(True)      # noqa: E731
    w = new(91, 4, 4, 3, 3)
    ops = {"act_fir": lambda t: act_fir(t, R.low_pass().to(dev), [1, 1, 1, 1], bias=torch.ones(4, device=dev), act="lrelu"),
           "minibatch_std": lambda t: minibatch_std(t, 2), "conv2d_resample": lambda t: conv2d_plain(t, w, 1)}
    for name, op in ops.items():
        x = new(92, 2, 4, 4, 4)
        with pytest.raises(NotImplementedError, match="create_graph"):
            torch.autograd.grad(op(x).square().sum(), x, create_graph=True)
        with style_ops.second_order():
            (g,) = torch.autograd.grad(op(x).square().sum(), x, create_graph=True)
            assert g.requires_grad, name
            with pytest.raises(NotImplementedError, match="create_graph"):         # third order
                torch.autograd.grad(g.square().sum(), x, create_graph=True)
        (g,) = torch.autograd.grad(op(x).square().sum(), x)         # first order is untouched
        assert not g.requires_grad
    x, s = new(93, 1, 4, 4, 4), new(94, 1, 4)
    with style_ops.second_order():
        with pytest.raises(NotImplementedError, match="modulated_conv2d"):
            torch.autograd.grad(modulated_conv2d(x, w, s, padding=1, flip_weight=False).square().sum(), [s], create_graph=True)


# ---- the networks -----------------------------------------------------------------------------------------------------------------------------------------

def discriminator(dis, tag, dev, **extra):
    from studiogan_amd.backbones import stylegan2_dis as SD
    Dn = SD.Discriminator(**D.kwargs_of(D.CASES[tag], **extra))
    Dn.load_state_dict(state(dis, tag), strict=True)
    return Dn.to(dev)


def bound(r1, tag, what):
    return max(2e-5, 4 * float(r1[f"{tag}/ref32_err/{what}"]))


def r1_step(Dn, img, label):
    """(penalty, r1_grads) through losses.stylegan_cal_r1_reg; the penalty's backward has run"""
    from studiogan_amd import losses
    adv = Dn(img, label)["adv_output"]
    (g,) = torch.autograd.grad(adv.sum(), img, retain_graph=True)       # (the plain first-order image gradient: what the penalty squares)
    penalty = losses.stylegan_cal_r1_reg(adv_output=adv, images=img)
    assert penalty.requires_grad and penalty.dim() == 0
    penalty.backward()
    return penalty.detach(), g


def check_network_fp32(lib, dev, fix, tag, fused, report):
    dis, r1 = fix
    Dn = discriminator(dis, tag, dev, fused_down=fused)
    img = r1[f"{tag}/img"].detach().to(dev).requires_grad_(True)
    penalty, g = r1_step(Dn, img, r1[f"{tag}/label"].to(dev))
    name = f"r1 {tag} {'fused' if fused else 'layerwise'}"
    what = lambda k: f"{name} {k} (ref32_err {float(r1[f'{tag}/ref32_err/{k}']):.1e})"      # noqa: E731
    check(what("penalty"), penalty, r1[f"{tag}/penalty"], bound(r1, tag, "penalty"), report)
    check(what("r1_grads"), g, r1[f"{tag}/r1_grads"], bound(r1, tag, "r1_grads"), report)
    params = dict(Dn.named_parameters())
    assert list(params) == param_keys(dis, tag)
    for k, p in params.items():
        e = r1[f"{tag}/dp/{k}"]
        if float(e.abs().max()) == 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0, k
            continue
        check(what(f"dp/{k}"), p.grad, e, bound(r1, tag, f"dp/{k}"), report)
    if tag == "skip":       # Freeze-D: the frozen layers are buffers and have no gradient
        assert not any(k.startswith(("b16.fromrgb", "b16.conv0")) for k in params)


def check_network_bf16(lib, dev, fix, tag, fused, report):
    """block b16 in bf16 (conv_clamp 256) against fp64 with the clamp: each quantity at 3 x its share of bf16_floor (none larger than the fixture's bf16_floor),
    the parameter gradients in relative L2 per tensor. No element is excused: tests/make_golden_stylegan2_r1.py shows that the bf16 emulation, which the floor
    comes from, already differs from fp64 on up to 0.2 % of a layer's leaky ReLU sides, so the floor carries what a moved side costs."""
    dis, r1 = fix
    Dn = discriminator(dis, tag, dev, fused_down=fused, **D.LOWP)
    acts = {}
    hook = Dn.b16.register_forward_hook(lambda m, i, o: acts.__setitem__(16, o[0]))
    img = r1[f"{tag}/img"].detach().to(dev).requires_grad_(True)
    penalty, g = r1_step(Dn, img, r1[f"{tag}/label"].to(dev))
    hook.remove()
    assert acts[16].dtype == torch.bfloat16 and acts[16].is_contiguous(memory_format=CL)
    floor = lambda k: float(r1[f"{tag}/bf16_floor_of/{k}"])      # noqa: E731
    assert all(floor(k[len(tag) + 15:]) <= float(r1[f"{tag}/bf16_floor"]) for k in r1 if k.startswith(f"{tag}/bf16_floor_of/"))
    name = f"r1 {tag} {'fused' if fused else 'layerwise'} bf16 blocks"
    check(f"{name} penalty (floor {floor('penalty'):.1e})", penalty, r1[f"{tag}/lowp/penalty"], 3 * floor("penalty"), report)
    check(f"{name} r1_grads (floor {floor('r1_grads'):.1e})", g, r1[f"{tag}/lowp/r1_grads"], 3 * floor("r1_grads"), report)
    for k, p in Dn.named_parameters():
        e = r1[f"{tag}/lowp/dp/{k}"]
        if float(e.abs().max()) == 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0, k
            continue
        assert bool(torch.isfinite(p.grad).all()), k
        d, t = rel_l2(p.grad, e), 3 * floor(f"dp/{k}")
        line = f"{name} dp/{k} (floor {floor(f'dp/{k}'):.1e})"
        print(f"{line:48s} l2err={d:.3e} tol={t:.1e} {'ok' if d <= t else 'FAIL'}")
        if report is not None:
            report.append((line + " [rel L2]", d, t))
        assert d <= t, line


def check_launch_counters(lib, dev, fix):
    """one R1 step of `resnet` with fused heads. Four launches of the head kernel's family serve a fused head or a skip FIR (2 blocks x 2 = 4 of them): the
    forward, the first-order backward inside the context, the gate launch of the penalty's backward -- and the first-order backward ONCE MORE in the penalty's
    backward, outside the context: the minibatch standard deviation has a second derivative, so the penalty also depends on the activations in front of it,
    and that gradient walks the forward graph's own backward (fp64 autograd of the restatement has the same term; without it the weight gradients of every
    layer in front of the statistic miss the fixture). The statistic itself: forward, backward, second-order pass."""
    from studiogan_amd import losses
    dis, r1 = fix
    Dn = discriminator(dis, "resnet", dev, fused_down=True)
    img = r1["resnet/img"].detach().to(dev).requires_grad_(True)
    n0, m0 = lib.sg_act_fir_launches(), lib.sg_mbstd_launches()
    adv = Dn(img, r1["resnet/label"].to(dev))["adv_output"]
    assert lib.sg_act_fir_launches() - n0 == 4 and lib.sg_mbstd_launches() - m0 == 1
    penalty = losses.stylegan_cal_r1_reg(adv_output=adv, images=img)
    assert lib.sg_act_fir_launches() - n0 == 8 and lib.sg_mbstd_launches() - m0 == 2
    penalty.backward()
    assert lib.sg_act_fir_launches() - n0 == 16, "per head: forward, backward, gate, and the forward graph's backward for the statistic's second derivative"
    assert lib.sg_mbstd_launches() - m0 == 3


def check_d_reg_step(lib, dev, fix, report, tag="skip", r1_lambda=10.0, d_reg_interval=16):
    """losses.stylegan_d_reg_step leaves d_reg_interval * r1_lambda x the penalty's gradients in .grad (the bound scales with the expectation), returns the
    detached scaled penalty, and gives every head the penalty does not read a ZERO gradient (the reference's enable_allreduce terms), not none"""
    from studiogan_amd import losses
    dis, r1 = fix
    Dn = discriminator(dis, tag, dev)
    scale = r1_lambda * d_reg_interval
    img = r1[f"{tag}/img"].detach().to(dev)
    value = losses.stylegan_d_reg_step(Dn, img, r1[f"{tag}/label"].to(dev), r1_lambda, d_reg_interval)
    assert not value.requires_grad and value.grad_fn is None and not img.requires_grad
    check(f"d_reg_step {tag} penalty", value, r1[f"{tag}/penalty"] * scale, bound(r1, tag, "penalty"), report)
    half = losses.stylegan_d_reg_step(Dn, img, r1[f"{tag}/label"].to(dev), r1_lambda, d_reg_interval, acml_steps=2)      # accumulates half as much on top
    check(f"d_reg_step {tag} penalty, acml_steps=2", half, r1[f"{tag}/penalty"] * scale / 2, bound(r1, tag, "penalty"), report)
    for k, p in Dn.named_parameters():
        e = r1[f"{tag}/dp/{k}"] * (scale * 1.5)
        assert p.grad is not None, k
        if float(e.abs().max()) == 0:
            assert float(p.grad.abs().max()) == 0, k
            continue
        check(f"d_reg_step {tag} dp/{k}", p.grad, e, bound(r1, tag, f"dp/{k}"), report)
    assert any(k.startswith("linear2") for k, _ in Dn.named_parameters())
