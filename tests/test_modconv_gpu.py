"""GPU parity of the modulated convolution (csrc/modconv.hip through style_ops.modulated_conv2d) and of the two layers that wrap it.

fp32: every case of tests/golden/modconv*.npz (the reference in fp64), output and all gradients, to 2e-5 of the expected tensor's range -- the bound
tests/test_style_gpu.py holds the other StyleGAN operators to (the reference's own fp32 evaluation sits at 3.4e-7 on a K = 576 case).
bf16: the same cases against tests/modconv_ref.py in fp64 on the inputs rounded to bf16 (x, weight and gy rounded, styles kept fp32), to 1e-2 of range, that
file's bf16 convention (the reference's own bf16 route on the CPU is 5.4e-3 from fp64 on case a, an emulation of this kernel's rounding points 3.5e-3).
Every measured error goes to profiles/modconv_pytest_gpu.txt when the module is done."""
import os

import pytest
import torch

import modconv_ref as R
from util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = []
DTYPES = [torch.float32, torch.bfloat16]


def _tol(dtype):
    return 2e-5 if dtype == torch.float32 else 1e-2


def _name(dtype):
    return "fp32" if dtype == torch.float32 else "bf16"


@pytest.fixture(scope="module")
def fix():
    yield {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in R.load_golden().items()}
    try:
        with open(os.path.join(ROOT, "profiles", "modconv_pytest_gpu.txt"), "w") as f:
            f.write("tests/test_modconv_gpu.py on %s: max |got - expected| / max |expected| of every check\n" % torch.cuda.get_device_name(0))
            for name, e, tol in REPORT:
                f.write(f"{name:56s} err={e:.3e} tol={tol:.1e}\n")
    except OSError:
        pass


def _rb(t):
    """fp64 values of t rounded to bf16"""
    return t.to(torch.bfloat16).double()


def _run(x, w, s, nz, gy, dtype, **kw):
    """the operator on the GPU: (y, dx, dw, ds, dnoise or None); x / gy in dtype, weight, styles and noise fp32"""
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d
    xd = x.to(DEV, dtype).requires_grad_(True)
    wd, sd = w.to(DEV, torch.float32).requires_grad_(True), s.to(DEV, torch.float32).requires_grad_(True)
    nd = None if nz is None else nz.to(DEV, torch.float32).requires_grad_(True)
    y = modulated_conv2d(xd, wd, sd, noise=nd, **kw)
    assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    gr = torch.autograd.grad(y, [xd, wd, sd] + ([nd] if nd is not None else []), gy.to(DEV, dtype))
    return (y.detach(),) + tuple(gr[:3]) + ((gr[3],) if nd is not None else (None,))


def _expected(x, w, s, nz, gy, dtype, up, demod, flip):
    """fp64 restatement on what the kernel is given: bf16 runs see x, weight and gy rounded"""
    if dtype == torch.bfloat16:
        x, w, gy = _rb(x), _rb(w), _rb(gy)
    return (x, w, gy), R.modconv_ref_grads(x.double(), w.double(), s.double(), None if nz is None else nz.double(), gy.double(),
                                           up=up, demodulate=demod, flip_weight=flip, f=R.low_pass().double())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("tag", list(R.OP_CASES))
def test_operator_matches_golden(sg, fix, tag, dtype):
    N, C, Cout, H, k, up, demod, noise, flip = R.OP_CASES[tag]
    g = lambda n: fix.get(f"op/{tag}/{n}")      # noqa: E731
    x, w, s, nz, gy = g("x"), g("w"), g("s"), g("noise"), g("gy")
    if dtype == torch.float32:
        exp = tuple(g(n) for n in ("y", "dx", "dw", "ds", "dnoise"))
    else:
        (x, w, gy), exp = _expected(x, w, s, nz, gy, dtype, up, demod, flip)
    got = _run(x, w, s, nz, gy, dtype, up=up, padding=k // 2, resample_filter=R.low_pass().to(DEV), demodulate=demod, flip_weight=flip)
    for name, a, e in zip(("y", "dx", "dw", "ds", "dnoise"), got, exp):
        if e is not None:
            check(f"op {tag} {_name(dtype)} {name}", a, e, _tol(dtype), REPORT)


@pytest.fixture(scope="module")
def large():
    """N=4, C=128, Cout=96, 32 x 32, 3 x 3, per-sample noise: several tiles per sample, a ragged cout tile, K = 1152"""
    g = torch.Generator().manual_seed(7)
    N, C, Cout, H = 4, 128, 96, 32
    x, w = torch.randn(N, C, H, H, generator=g), torch.randn(Cout, C, 3, 3, generator=g)
    s = 1 + torch.randn(N, C, generator=g)
    s[torch.rand(N, C, generator=g) < 0.1] = 0.0
    nz, gy = torch.randn(N, 1, H, H, generator=g), torch.randn(N, Cout, H, H, generator=g)
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = _expected(x, w, s, nz, gy, dtype, 1, True, True)
        return (s, nz) + cache[dtype]
    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_operator_larger_random_shape(sg, large, dtype):
    s, nz, (x, w, gy), exp = large(dtype)
    got = _run(x, w, s, nz, gy, dtype, padding=1)
    for name, a, e in zip(("y", "dx", "dw", "ds", "dnoise"), got, exp):
        check(f"op 4x128x96x32x32 {_name(dtype)} {name}", a, e, _tol(dtype), REPORT)


def test_up2_without_resample_filter(sg, fix):
    """resample_filter=None at up = 2: the identity filter, i.e. zero insertion times 4 and the crop of conv2d_resample's padding arithmetic"""
    tag = "e"
    N, C, Cout, H, k, up, demod, noise, flip = R.OP_CASES[tag]
    g = lambda n: fix.get(f"op/{tag}/{n}")      # noqa: E731
    exp = R.modconv_ref_grads(g("x").double(), g("w").double(), g("s").double(), g("noise").double(), g("gy").double(), up=2, demodulate=demod, flip_weight=flip, f=None)
    got = _run(g("x"), g("w"), g("s"), g("noise"), g("gy"), torch.float32, up=2, padding=1, resample_filter=None, demodulate=demod, flip_weight=flip)
    for name, a, e in zip(("y", "dx", "dw", "ds", "dnoise"), got, exp):
        check(f"op {tag} fp32 no filter {name}", a, e, 2e-5, REPORT)


@pytest.mark.parametrize("up", [1, 2])
def test_zero_styles_have_finite_gradients(sg, fix, up):
    """styles[n, c] == 0 exactly: dstyles there is sum_p x gxs - 0, finite and within the bound (a kernel that recovers anything by dividing by s fails here)"""
    tag = "a" if up == 1 else "e"
    N, C, Cout, H, k, _, demod, noise, flip = R.OP_CASES[tag]
    g = lambda n: fix.get(f"op/{tag}/{n}")      # noqa: E731
    zero = g("s") == 0
    assert int(zero.sum()) >= 2
    got = _run(g("x"), g("w"), g("s"), g("noise"), g("gy"), torch.float32, up=up, padding=1, resample_filter=R.low_pass().to(DEV), flip_weight=flip)
    for a in got:
        assert a is None or bool(torch.isfinite(a).all())
    ds, e = got[3].cpu().double(), g("ds")
    err = float((ds - e)[zero].abs().max() / e.abs().max())
    REPORT.append((f"zero styles up={up}: ds at s == 0", err, 2e-5))
    assert err <= 2e-5, err
    assert float(e[zero].abs().max()) > 0, "the expected gradient at a zero style is not itself zero"


def test_up1_forward_is_one_launch(sg, fix):
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d
    g = lambda n: fix[f"op/a/{n}"].to(DEV, torch.float32)      # noqa: E731
    lib = sg.lib()
    for dtype in DTYPES:
        with torch.no_grad():
            n0 = lib.sg_modconv_launches()
            modulated_conv2d(g("x").to(dtype), g("w"), g("s"), noise=g("noise"), padding=1)
            assert lib.sg_modconv_launches() - n0 == 1


def test_no_per_sample_weights(sg):
    """N=16, C=Cout=256, 3 x 3, 8 x 8, fp32: activations 1 MB each, the packed weight image 2.4 MB; a [N, Cout, C, 3, 3] tensor would be 37.7 MB"""
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d
    x = torch.randn(16, 256, 8, 8, device=DEV)
    w, s = torch.randn(256, 256, 3, 3, device=DEV), torch.randn(16, 256, device=DEV)
    with torch.no_grad():
        modulated_conv2d(x, w, s, padding=1)      # first call: library / allocator warm-up outside the measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = modulated_conv2d(x, w, s, padding=1)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    REPORT.append(("no per-sample weights: peak rise in MB (bound 8)", rise / 2 ** 20, 8.0))
    assert rise < 8 * 2 ** 20, rise
    assert bool(torch.isfinite(y).all())


def _layer(fix, tag, dtype):
    from studiogan_amd.backbones import stylegan2_layers as SL
    cls, kw, res_in, mode = R.LAYER_CASES[tag]
    p = f"layer/{tag}/"
    sd = {k[len(p) + 3:]: v for k, v in fix.items() if k.startswith(p + "sd/")}
    layer = getattr(SL, cls)(**kw)
    layer.load_state_dict(sd, strict=True)
    return layer.to(DEV), cls, kw, mode, sd, p


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("tag", list(R.LAYER_CASES))
def test_layer_matches_golden(sg, fix, tag, dtype):
    layer, cls, kw, mode, sd, p = _layer(fix, tag, dtype)
    x, wl, gy = fix[p + "x"], fix[p + "w"], fix[p + "gy"]
    if dtype == torch.float32:
        exp_y = fix[p + "y"]
        exp = {"x": fix[p + "dx"], "wl": fix[p + "dwl"], **{k: fix[p + "dp/" + k] for k, _ in layer.named_parameters()}}
    else:       # x, gy and the convolution's weight image rounded to bf16; parameters, latents and styles stay fp32
        x, gy = _rb(x), _rb(gy)
    xd, wd = x.to(DEV, dtype).requires_grad_(True), wl.to(DEV, torch.float32).requires_grad_(True)
    y = layer(xd, wd, noise_mode=mode) if cls == "SynthesisLayer" else layer(xd, wd)
    if dtype == torch.bfloat16:
        sd64 = {k: v.double() for k, v in sd.items()}
        exp_y = R.layer_ref(cls, kw, sd64, x, wl.double(), mode, conv_weight=_rb(sd["weight"]))[0].detach()
        # The leaky ReLU's derivative jumps at 0. A bf16 run whose pre-activation lies within its rounding error of 0 may sit on the other side than
        # the fp64 restatement, and its gradient then differs by 0.8 sqrt(2) gy at that element however exact the kernels are (an emulation of the
        # rounding points on the CPU: 8 such elements of 12288 in syn_up, 9e-2 of range in dx). So the expected GRADIENT is taken on the side the
        # device was on -- and the device may differ from fp64 only where fp64's own value is below the bound; the forward check knows no mask.
        mask = None
        if cls == "SynthesisLayer":
            mask = (y.detach() > 0).cpu()
            moved = mask != (exp_y > 0)
            assert float(exp_y[moved].abs().max() if bool(moved.any()) else 0.0) <= _tol(dtype) * float(exp_y.abs().max()), "a sign differs where the value is not small"
            # and only a few may: a bf16 value lands on the other side when |pre-activation| is below its error, ~4e-3 of range here, which is under
            # 0.5 % of the elements of a unit-scale output; a kernel that biases values near zero moves more
            limit = 0.005 * exp_y.numel()
            REPORT.append((f"layer {tag} bf16 lrelu sides that differ from fp64 (count, of {exp_y.numel()})", float(moved.sum()), limit))
            assert int(moved.sum()) <= limit, int(moved.sum())
        ym, leaves = R.layer_ref(cls, kw, sd64, x, wl.double(), mode, conv_weight=_rb(sd["weight"]), act_mask=mask)
        names = list(leaves)
        gr = torch.autograd.grad(ym, [leaves[k] for k in names], gy, allow_unused=True)
        exp = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(names, gr)}
    check(f"layer {tag} {_name(dtype)} y", y, exp_y, _tol(dtype), REPORT)
    params = dict(layer.named_parameters())
    gr = torch.autograd.grad(y, [xd, wd] + list(params.values()), gy.to(DEV, dtype), allow_unused=True)
    for k, g in zip(["x", "wl"] + list(params), gr):
        e = exp[k]
        if g is None:
            assert float(e.abs().max()) == 0, (tag, k)
            continue
        if float(e.abs().max()) == 0:
            assert float(g.abs().max()) == 0, (tag, k)
            continue
        check(f"layer {tag} {_name(dtype)} d{k}", g, e, _tol(dtype), REPORT)


def test_random_noise_of_strength_zero_is_no_noise(sg, fix):
    for tag in ("syn", "syn_up"):
        layer, cls, kw, mode, sd, p = _layer(fix, tag, torch.float32)
        with torch.no_grad():
            layer.noise_strength.zero_()
            x, wl = fix[p + "x"].to(DEV, torch.float32), fix[p + "w"].to(DEV, torch.float32)
            assert torch.equal(layer(x, wl, noise_mode="random"), layer(x, wl, noise_mode="none"))


def test_second_order_is_refused(sg, fix):
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d
    g = lambda n: fix[f"op/g/{n}"].to(DEV, torch.float32).requires_grad_(True)      # noqa: E731
    x, w, s = g("x"), g("w"), g("s")
    y = modulated_conv2d(x, w, s, padding=1, flip_weight=False)
    with pytest.raises(NotImplementedError, match="modulated_conv2d"):
        torch.autograd.grad(y.square().sum(), [s], create_graph=True)
