"""GPU parity of the StyleGAN2 discriminator (backbones/stylegan2_dis.py) and of what it adds: the head of a down layer (csrc/style_fir.hip sg_act_fir_nhwc
through style_ops.act_fir), the minibatch standard deviation (csrc/mbstd.hip) and the plain convolutions of style_ops.conv2d_resample.

Bounds. fp32 operators: 2e-5 of the expected tensor's range. bf16 operators: inputs rounded to bf16, the fp64 restatement on the rounded values, 1e-2 of range
(tests/test_stylegan2_gpu.py::_tol). fp32 networks: max(2e-5, 4 * ref32_err) of range per quantity, ref32_err = the reference's own fp32 distance from the fp64
expectation (tests/make_golden_stylegan2_dis.py). bf16 networks: outputs only, 3 * bf16_floor, the floor = the restatement with bf16 storage on the CPU.
The head kernel's inputs sit on grids both dtypes hold exactly (stylegan2_dis_ref.head_inputs), so no activation side or clamp decision may differ from fp64.
Every measured error goes to profiles/stylegan2_dis_pytest_gpu.txt when the module is done."""
import os

import pytest
import torch

import modconv_ref as R
import stylegan2_dis_ref as D
from util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = []
DTYPES = [torch.float32, torch.bfloat16]
CL = torch.channels_last


def _tol(dtype):
    return 2e-5 if dtype == torch.float32 else 1e-2


def _name(dtype):
    return "fp32" if dtype == torch.float32 else "bf16"


@pytest.fixture(scope="module")
def fix():
    yield {k: (torch.from_numpy(v) if v.dtype.kind in "fi" else v) for k, v in D.load_golden().items()}
    try:
        with open(os.path.join(ROOT, "profiles", "stylegan2_dis_pytest_gpu.txt"), "w") as f:
            f.write("tests/test_stylegan2_dis_gpu.py on %s: max |got - expected| / max |expected| of every check (networks: bound = max(2e-5, 4 ref32_err), "
                    "bf16: 3 bf16_floor)\n" % torch.cuda.get_device_name(0))
            for name, e, tol in REPORT:
                f.write(f"{name:84s} err={e:.3e} tol={tol:.2e}\n")
    except OSError:
        pass


# ---- the head of a down layer -----------------------------------------------------------------------------------------------------------------------------

def _head_device(x, bias, gy, pad, down, e, dtype, fused):
    from studiogan_amd.style_ops.act_fir import act_fir
    from studiogan_amd.style_ops.bias_act import bias_act
    from studiogan_amd.style_ops.upfirdn2d import upfirdn2d
    f = R.low_pass().to(DEV)
    xd = x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
    bd = bias.to(DEV, torch.float32).requires_grad_(True) if e["bias"] else None
    if fused:
        y = act_fir(xd, f, list(pad), down=down, bias=bd, act=e["act"], gain=e["gain"], clamp=e["clamp_"])
        assert y.is_contiguous(memory_format=CL)
    else:
        a = bias_act(xd, None if bd is None else bd.to(dtype), act=e["act"], gain=e["gain"], clamp=e["clamp_"])
        y = upfirdn2d(a, f, down=down, padding=list(pad))
    assert y.dtype == dtype
    gr = torch.autograd.grad(y, [xd] + ([bd] if bd is not None else []), gy.to(DEV, dtype))
    return y.detach(), gr[0], (gr[1] if bd is not None else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("down", [1, 2])
@pytest.mark.parametrize("shape", list(D.HEAD_SHAPES))
def test_head_matches_chain_and_restatement(sg, shape, down, dtype):
    lib, tol = sg.lib(), _tol(dtype)
    for pad in D.HEAD_PADS:
        for epi, e in D.HEAD_EPI.items():
            x, bias, gy = D.head_inputs(shape, pad, down)       # (bf16 holds every value: nothing to round)
            ey, edx, edb = D.head_ref(x, bias, gy, pad, down, epi)      # (asserts the margins: no pre-activation at 0, none near the clamp, the clamp bites)
            tag = f"head {shape} down={down} {pad} {epi} {_name(dtype)}"
            n0 = lib.sg_act_fir_launches()
            got = _head_device(x, bias, gy, D.HEAD_PADS[pad], down, e, dtype, True)
            assert lib.sg_act_fir_launches() - n0 == 2, "forward and data gradient are one launch each"
            chain = _head_device(x, bias, gy, D.HEAD_PADS[pad], down, e, dtype, False)
            assert lib.sg_act_fir_launches() - n0 == 2, "the chain does not run the fused kernel"
            for which, (y, dx, db) in (("fused", got), ("chain", chain)):
                check(f"{tag} {which} y", y, ey, tol, REPORT)
                check(f"{tag} {which} dx", dx, edx, tol, REPORT)
                if edb is not None:
                    check(f"{tag} {which} dbias", db, edb, tol, REPORT)
            if dtype == torch.float32:      # two fp32 evaluations: the same bound between them
                for what, a, b in zip(("y", "dx", "dbias"), got, chain):
                    if a is not None:
                        check(f"{tag} fused vs chain {what}", a, b.double(), tol, REPORT)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_head_activation_sides_are_fp64s(sg, dtype):
    """cap 0: through a one-tap filter the operator returns the activated map itself, and its gradient the gate; neither may differ from fp64 in a single
    side of the leaky ReLU or a single clamp decision"""
    from studiogan_amd.style_ops.act_fir import act_fir
    x, bias, _ = D.head_inputs("seams", "p2", 1)
    e = D.HEAD_EPI["clamp"]
    xd = x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
    a = act_fir(xd, None, [0, 0, 0, 0], bias=bias.to(DEV, torch.float32), act="lrelu", gain=e["gain"], clamp=e["clamp_"])
    (gate,) = torch.autograd.grad(a, xd, torch.ones_like(a))
    pre = x + bias.reshape(1, -1, 1, 1)
    ea = D.bias_act(x, bias, "lrelu", e["gain"], e["clamp_"])
    a, gate = a.cpu().double(), gate.cpu().double()
    assert torch.equal(a > 0, pre > 0) and torch.equal(a.abs() == e["clamp_"], ea.abs() == e["clamp_"]) and bool((ea.abs() == e["clamp_"]).any())
    want = torch.where(ea.abs() == e["clamp_"], 0.0, torch.where(pre > 0, 1.0, 0.2) * e["gain"])
    assert torch.equal(gate == 0, want == 0) and torch.equal(gate > 1, want > 1)
    check(f"head sides {_name(dtype)} activated map", a, ea, _tol(dtype), REPORT)
    check(f"head sides {_name(dtype)} gate", gate, want, _tol(dtype), REPORT)


def test_head_border_is_zero_not_act_of_bias(sg):
    from studiogan_amd.style_ops.act_fir import act_fir
    for down in (1, 2):
        x, _, _ = D.head_inputs("edge", "p2", down)
        bias = torch.full((x.shape[1],), 1.5 + 2.0 ** -7, dtype=torch.float64)      # act(bias) = 2.1: in the padding it would move the border by O(1)
        want = D.act_fir(x, R.low_pass().double(), (2, 2, 2, 2), down, bias, "lrelu", D.SQRT2, None)
        leak = D.fir(D.bias_act(torch.nn.functional.pad(x, [2, 2, 2, 2]), bias, "lrelu", D.SQRT2), R.low_pass().double(), (0, 0, 0, 0), down)
        assert float((leak - want).abs().max()) > 0.1 * float(want.abs().max())
        y = act_fir(x.to(DEV, torch.float32).contiguous(memory_format=CL), R.low_pass().to(DEV), [2, 2, 2, 2], down=down, bias=bias.to(DEV, torch.float32), act="lrelu")
        check(f"head border down={down}", y, want, 2e-5, REPORT)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("down", [1, 2])
@pytest.mark.parametrize("C", [12, 13, 40])
def test_plain_mode_is_upfirdn2d_bit_for_bit(sg, C, down, dtype):
    """no gate: the kernel keeps sg_upfirdn2d's tap order, forward and adjoint, so both equal upfirdn2d on the NCHW copy BIT FOR BIT (12: whole fp32 vectors and
    the scalar path in bf16; 13: scalar; 40: vectors), strip boundary included"""
    from studiogan_amd.style_ops.act_fir import act_fir
    from studiogan_amd.style_ops.upfirdn2d import upfirdn2d
    g = torch.Generator().manual_seed(17 + C)
    f43 = torch.randn(4, 3, generator=g).to(DEV)
    for (H, W), f, pad, flip, gain in (((9, 11), R.low_pass().to(DEV), (2, 2, 2, 2), False, 1.0), ((9, 11), R.low_pass().to(DEV), (1, 1, 1, 1), True, 0.5),
                                      ((9, 11), f43, (2, 0, 1, 3), False, 1.0), ((8, 6), f43, (0, 1, -1, 3), True, 2.0), ((70, 5), R.low_pass().to(DEV), (2, 2, 2, 2), False, 1.0)):
        x = torch.randn(2, C, H, W, generator=g).to(DEV, dtype)
        xa, xb = x.contiguous(memory_format=CL).requires_grad_(True), x.clone().requires_grad_(True)
        a = act_fir(xa, f, list(pad), down=down, flip_filter=flip, filter_gain=gain)
        b = upfirdn2d(xb, f, down=down, padding=list(pad), flip_filter=flip, gain=gain)
        assert a.shape == b.shape and torch.equal(a.contiguous(), b), (C, pad, flip, float((a.float() - b.float()).abs().max()))
        gy = torch.randn(b.shape, generator=g).to(DEV, dtype)
        (da,), (db,) = torch.autograd.grad(a, xa, gy), torch.autograd.grad(b, xb, gy)
        assert torch.equal(da.contiguous(), db), (C, pad, flip, float((da.float() - db.float()).abs().max()))


def test_head_refuses_what_it_does_not_serve(sg):
    from studiogan_amd import _lib as L
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    f = torch.ones(5, 5, device=DEV)
    y = torch.empty(1, 4, 4, 8, device=DEV)
    args = lambda fh, down, act: (L.F32, x.data_ptr(), f.data_ptr(), y.data_ptr(), None, 1, 4, 4, 8, fh, fh, down, fh // 2, fh - 1 - fh // 2, fh // 2,      # noqa: E731
                                  fh - 1 - fh // 2, 0, 1.0, act, 0.2, 1.0, -1.0, L.stream())
    with pytest.raises(RuntimeError, match="1..4 taps"):
        L.call("sg_act_fir_nhwc", *args(5, 1, 1))
    with pytest.raises(RuntimeError, match="linear .1. or lrelu"):
        L.call("sg_act_fir_nhwc", *args(3, 1, 4))
    with pytest.raises(RuntimeError, match="down must be 1 or 2"):
        L.call("sg_act_fir_nhwc", *args(3, 3, 1))
    L.call("sg_act_fir_nhwc", *args(3, 1, 3))
    with pytest.raises(RuntimeError, match="N % G"):
        L.call("sg_mbstd_fwd", x.data_ptr(), 8, y.data_ptr(), None, None, 3, 2, 2, 8, 2, 1, L.stream())
    with pytest.raises(RuntimeError, match="C % F"):
        L.call("sg_mbstd_fwd", x.data_ptr(), 8, y.data_ptr(), None, None, 2, 2, 2, 8, 2, 3, L.stream())


# ---- minibatch standard deviation -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(D.MBSTD_CASES))
def test_minibatch_std(sg, case):
    from studiogan_amd.style_ops.minibatch_std import minibatch_std
    N, C, H, W, group, nch = D.MBSTD_CASES[case]
    lib = sg.lib()
    assert (lib.sg_mbstd_splits(N, H, W, C, N if group is None else min(group, N), nch) > 1) == (case == "split"), "the chunked path is the `split` case's"
    for constant in ((False, True) if case in ("g4f2", "g2f1") else (False,)):
        x, gy = D.mbstd_inputs(case, constant)      # (asserts every group's variance >= 2^-6 unless constant)
        o64, dx64 = D.mbstd_ref(x, gy, group, nch)
        xd = x.to(DEV, torch.float32).contiguous(memory_format=CL).requires_grad_(True)
        n0 = lib.sg_mbstd_launches()
        out = minibatch_std(xd, group, nch)
        (dx,) = torch.autograd.grad(out, xd, gy.to(DEV, torch.float32))
        assert lib.sg_mbstd_launches() - n0 == 2, "one launch forward, one backward"
        assert tuple(out.shape) == (N, C + nch, H, W) and out.is_contiguous(memory_format=CL) and torch.equal(out[:, :C], xd.detach())
        tag = f"mbstd {case}{' constant groups' if constant else ''}"
        if constant:        # zero variance: s = sqrt(1e-8), no gradient through the statistic, nothing divides by zero
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all())
            assert float((out.detach()[:, C:] - 1e-4).abs().max()) <= 1e-10 and torch.equal(dx, gy.to(DEV, torch.float32)[:, :C])
        check(f"{tag} out", out, o64, 2e-5, REPORT)
        check(f"{tag} dx", dx, dx64, 2e-5, REPORT)
        # the torch composition of the same lines, on the device
        xt = x.to(DEV, torch.float32).requires_grad_(True)
        ot = D.minibatch_std(xt, group, nch)
        (dxt,) = torch.autograd.grad(ot, xt, gy.to(DEV, torch.float32))
        check(f"{tag} out vs torch", out, ot.detach().double(), 2e-5, REPORT)
        if not constant:
            check(f"{tag} dx vs torch", dx, dxt.double(), 2e-5, REPORT)


# ---- the plain convolutions -------------------------------------------------------------------------------------------------------------------------------

def _layer_ref(sd, x, k, down, gy, lp):
    """fp64 DConv2dLayer (linear activation, the weight image in the operand dtype) and its gradients"""
    f = R.low_pass().double()
    x = x.clone().requires_grad_(True)
    sd = {k_: v.clone().requires_grad_(True) for k_, v in sd.items()}
    if down == 1:
        y = D.conv(x, sd, "l", lp=lp)
    elif k == 3:
        y = D.conv(D.fir(x, f, (2, 2, 2, 2)), sd, "l", stride=2, lp=lp)
    else:
        y = D.conv(D.fir(x, f, (1, 1, 1, 1), 2), sd, "l", lp=lp)
    y = y + sd["l.bias"].reshape(1, -1, 1, 1)
    return y.detach(), torch.autograd.grad(y, [x, sd["l.weight"], sd["l.bias"]], gy)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", [(1, 1), (3, 1), (3, 2), (1, 2)], ids=lambda g: f"k{g[0]}down{g[1]}")
def test_conv2d_resample_layers(sg, geom, dtype):
    from studiogan_amd.backbones.stylegan2_dis import DConv2dLayer
    from studiogan_amd.style_ops import conv2d_resample as CR
    k, down = geom
    vec = 4 if dtype == torch.float32 else 8
    seen = set()
    tol, lp = _tol(dtype), (None if dtype == torch.float32 else torch.bfloat16)
    for C in (3, 12, 16, 25):       # (16: the input channels fill 16-byte vectors in bf16 too, so both entries run in both dtypes)
        for Cout in (12, 24):
            g = torch.Generator().manual_seed(100 * C + Cout + k)
            q = lambda *s: (torch.randn(*s, generator=g, dtype=torch.float64) * 64).round().clamp(-192, 192) / 64      # noqa: E731
            x, gy = q(2, C, 8, 8), q(2, Cout, 8 // down, 8 // down)
            sd = {"l.weight": q(Cout, C, k, k), "l.bias": q(Cout)}
            ey, eg = _layer_ref(sd, x, k, down, gy, lp)
            for fused in ((True, False) if down == 2 else (True,)):
                layer = DConv2dLayer(C, Cout, k, down=down).to(DEV)
                layer.load_state_dict({"weight": sd["l.weight"].float(), "bias": sd["l.bias"].float(), "resample_filter": R.low_pass()}, strict=True)
                xd = x.to(DEV, dtype).contiguous(memory_format=CL).requires_grad_(True)
                with CR.record() as log:
                    y = layer(xd, fused=fused)
                    assert y.dtype == dtype and tuple(y.shape) == tuple(ey.shape)
                    gr = torch.autograd.grad(y, [xd, layer.weight, layer.bias], gy.to(DEV, dtype))
                # which entry ran: the planned dispatch when the launch's input channels fill 16-byte vectors, the NULL-table modulated entry otherwise
                assert [(r[0], r[1]) for r in log] == [("fwd", CR.ENTRIES[0 if C % vec == 0 else 1]), ("dgrad", CR.ENTRIES[0 if Cout % vec == 0 else 1])], log
                seen.update(r[1] for r in log)
                tag = f"conv k={k} down={down} C={C} Cout={Cout} {'fused' if fused else 'chain'} {_name(dtype)}"
                check(f"{tag} y", y, ey, tol, REPORT)
                for what, a, b in zip(("dx", "dw", "db"), gr, eg):
                    check(f"{tag} {what}", a, b, tol, REPORT)
    assert seen == set(CR.ENTRIES)


# ---- the networks -----------------------------------------------------------------------------------------------------------------------------------------

def _sd(fix, tag):
    out = {}
    for k in (str(k) for k in fix[f"{tag}/keys"]):
        out[k] = fix[f"{tag}/sd/{k}" if f"{tag}/sd/{k}" in fix else f"orig/sd/{k}"].float()
    return out


def _discriminator(fix, tag, **extra):
    from studiogan_amd.backbones import stylegan2_dis as SD
    Dn = SD.Discriminator(**D.kwargs_of(D.CASES[tag], **extra))
    Dn.load_state_dict(_sd(fix, tag), strict=True)
    return Dn.to(DEV)


def _bound(fix, tag, what):
    return max(2e-5, 4 * float(fix[f"{tag}/ref32_err/{what}"]))


def _fused_layers(tag):
    """down layers whose head is one sg_act_fir_nhwc launch: conv1 of both blocks, and the skip convolution of a resnet block"""
    return 4 if D.CASES[tag]["architecture"] == "resnet" else 2


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layerwise"])
@pytest.mark.parametrize("tag", list(D.CASES))
def test_network_fp32_matches_fixture(sg, fix, tag, fused):
    Dn = _discriminator(fix, tag, fused_down=fused)
    lib = sg.lib()
    img = fix[f"{tag}/img"].to(DEV).requires_grad_(True)
    n0, m0 = lib.sg_act_fir_launches(), lib.sg_mbstd_launches()
    out = Dn(img, fix[f"{tag}/label"].to(DEV))
    assert lib.sg_act_fir_launches() - n0 == (_fused_layers(tag) if fused else 0), "one sg_act_fir_nhwc launch per fused down layer"
    assert lib.sg_mbstd_launches() - m0 == 1, "one sg_mbstd_fwd per forward"
    assert list(out) == list(D.OUT_KEYS)
    floats = D.float_outputs(out)
    assert set(floats) == {k[len(tag) + 5:] for k in fix if k.startswith(f"{tag}/out/")}
    assert torch.equal(out["label"].cpu(), fix[f"{tag}/label"] * (2 if D.CASES[tag]["aux_cls_type"] == "ADC" else 1))
    name = f"net {tag} {'fused' if fused else 'layerwise'}"
    for k, v in floats.items():
        assert v.dtype == torch.float32 and tuple(v.shape) == tuple(fix[f"{tag}/out/{k}"].shape), k
        check(f"{name} {k} (ref32_err {float(fix[f'{tag}/ref32_err/{k}']):.1e})", v, fix[f"{tag}/out/{k}"], _bound(fix, tag, k), REPORT)
    loss = sum((v * fix[f"{tag}/g_{k}"].to(DEV)).sum() for k, v in floats.items())
    params = dict(Dn.named_parameters())
    gr = torch.autograd.grad(loss, [img] + list(params.values()), allow_unused=True)
    check(f"{name} dimg (ref32_err {float(fix[f'{tag}/ref32_err/dimg']):.1e})", gr[0], fix[f"{tag}/dimg"], _bound(fix, tag, "dimg"), REPORT)
    held = 0
    for (k, _), g in zip(params.items(), gr[1:]):
        if f"{tag}/dp/{k}" not in fix:      # (a heads-only case stores the head's gradients)
            assert tag not in D.FULL_CASES and not D.is_head_key(k), k
            continue
        e = fix[f"{tag}/dp/{k}"]
        held += 1
        if float(e.abs().max()) == 0:
            assert g is None or float(g.abs().max()) == 0, k
            continue
        check(f"{name} d {k} (ref32_err {float(fix[f'{tag}/ref32_err/dp/{k}']):.1e})", g, e, _bound(fix, tag, f"dp/{k}"), REPORT)
    assert held == sum(1 for k in fix if k.startswith(f"{tag}/dp/"))
    if tag == "skip":       # Freeze-D: the frozen layers are buffers and have no gradient
        assert not any(k.startswith(("b16.fromrgb", "b16.conv0")) for k in params)
    if tag == "ac_adc":
        with torch.no_grad():
            fake = Dn(img.detach(), fix[f"{tag}/label"].to(DEV), adc_fake=True)
        assert torch.equal(fake["label"].cpu(), fix[f"{tag}/out_fake/label"])
        check(f"{name} cls_output of the fake copies", fake["cls_output"], fix[f"{tag}/out_fake/cls_output"], _bound(fix, tag, "cls_output"), REPORT)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layerwise"])
@pytest.mark.parametrize("tag", list(D.CASES))
def test_network_bf16_blocks(sg, fix, tag, fused):
    Dn = _discriminator(fix, tag, fused_down=fused, **D.LOWP)
    acts = {}
    hooks = [getattr(Dn, f"b{r}").register_forward_hook(lambda m, i, o: acts.__setitem__(m.resolution, o[0])) for r in (16, 8)]
    lib = sg.lib()
    n0, m0 = lib.sg_act_fir_launches(), lib.sg_mbstd_launches()
    with torch.no_grad():
        out = Dn(fix[f"{tag}/img"].to(DEV), fix[f"{tag}/label"].to(DEV))
    for h in hooks:
        h.remove()
    assert lib.sg_act_fir_launches() - n0 == (_fused_layers(tag) if fused else 0) and lib.sg_mbstd_launches() - m0 == 1
    assert acts[16].dtype == torch.bfloat16 and acts[16].is_contiguous(memory_format=CL) and acts[8].dtype == torch.float32
    floor = float(fix[f"{tag}/bf16_floor"])
    for k, v in D.float_outputs(out).items():
        assert v.dtype == torch.float32
        check(f"net {tag} {'fused' if fused else 'layerwise'} bf16 blocks {k} (bf16_floor {floor:.2e})", v, fix[f"{tag}/lowp/{k}"], 3 * floor, REPORT)


def test_second_order_is_refused(sg, fix):
    Dn = _discriminator(fix, "orig")
    img = fix["orig/img"].to(DEV).requires_grad_(True)
    adv = Dn(img, fix["orig/label"].to(DEV))["adv_output"]
    with pytest.raises(NotImplementedError, match="create_graph"):
        torch.autograd.grad(adv.sum(), img, create_graph=True)
