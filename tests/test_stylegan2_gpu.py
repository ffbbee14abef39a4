"""GPU parity of the StyleGAN2 generator networks (backbones/stylegan2.py) and of the two launches they add: the fused up = 2 layer tail
(csrc/style_fir.hip through style_ops.modulated_conv2d_act) and the grouped style affines (sg_linear_group_scaled).

Bounds. fp32 operators: 2e-5 of the expected tensor's range, the standing bound of tests/test_style_gpu.py and tests/test_modconv_gpu.py. bf16 operators: that
file's convention -- x, weight and gy rounded to bf16, the fp64 restatement on the rounded values, 1e-2 of range. fp32 networks: max(2e-5, 4 * ref32_err) of
range per quantity, ref32_err = the reference's own fp32 distance from the fp64 expectation (tests/make_golden_stylegan2.py; the factor 4 covers another fp32
summation order over seven layers). bf16 networks: 3 * bf16_floor, the floor = the restatement with bf16 activation storage on the CPU.
Every measured error goes to profiles/stylegan2_pytest_gpu.txt when the module is done."""
import os

import pytest
import torch

import modconv_ref as R
import stylegan2_ref as S
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


def _rb(t):
    return t.to(torch.bfloat16).double()


@pytest.fixture(scope="module")
def fix():
    yield {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in S.load_golden().items()}
    try:
        with open(os.path.join(ROOT, "profiles", "stylegan2_pytest_gpu.txt"), "w") as f:
            f.write("tests/test_stylegan2_gpu.py on %s: max |got - expected| / max |expected| of every check (networks: bound = max(2e-5, 4 ref32_err), bf16: 3 bf16_floor)\n"
                    % torch.cuda.get_device_name(0))
            for name, e, tol in REPORT:
                f.write(f"{name:72s} err={e:.3e} tol={tol:.2e}\n")
    except OSError:
        pass


# ---- the fused tail ---------------------------------------------------------------------------------------------------------------------------------------

def _tail_device(x, w, s, nz, bias, gy, dtype, fused, gain, clamp):
    from studiogan_amd.style_ops.bias_act import bias_act
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d, modulated_conv2d_act
    lv = {"x": x.to(DEV, dtype), "w": w.to(DEV, torch.float32), "s": s.to(DEV, torch.float32), "bias": bias.to(DEV, torch.float32)}
    if nz is not None:
        lv["noise"] = nz.to(DEV, torch.float32)
    lv = {k: v.requires_grad_(True) for k, v in lv.items()}
    kw = dict(noise=lv.get("noise"), up=2, padding=1, resample_filter=R.low_pass().to(DEV), flip_weight=False)
    if fused:
        y = modulated_conv2d_act(lv["x"], lv["w"], lv["s"], bias=lv["bias"], act="lrelu", gain=S.SQRT2 * gain, clamp=clamp, **kw)
    else:
        y = modulated_conv2d(lv["x"], lv["w"], lv["s"], **kw)
        y = bias_act(y, lv["bias"].to(y.dtype), act="lrelu", gain=S.SQRT2 * gain, clamp=clamp)
    assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    names = list(lv)
    return y.detach(), dict(zip(names, torch.autograd.grad(y, [lv[k] for k in names], gy.to(DEV, dtype))))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("epi", list(S.TAIL_EPI))
@pytest.mark.parametrize("noise", S.TAIL_NOISE, ids=lambda n: f"noise-{n}")
@pytest.mark.parametrize("shape", list(S.TAIL_SHAPES))
def test_fused_tail_matches_chain_and_restatement(sg, fix, shape, noise, epi, dtype):
    gain, clamp = S.TAIL_EPI[epi]["gain"], S.TAIL_EPI[epi]["clamp"]
    x, w, s, nz, bias, gy = S.tail_inputs(shape, noise)
    if dtype == torch.bfloat16:      # (the demodulation coefficients come from the weight the operator is given: the rounded one)
        x, w, gy = _rb(x), _rb(w), _rb(gy)
    tol, tag = _tol(dtype), f"tail {shape} noise={noise} {epi} {_name(dtype)}"
    lib = sg.lib()
    n0 = lib.sg_fir_bias_act_launches()
    y, g = _tail_device(x, w, s, nz, bias, gy, dtype, True, gain, clamp)
    assert lib.sg_fir_bias_act_launches() - n0 == 2, "forward and data gradient are one sg_fir_bias_act_nhwc launch each"
    yc, gc = _tail_device(x, w, s, nz, bias, gy, dtype, False, gain, clamp)
    assert lib.sg_fir_bias_act_launches() - n0 == 2, "the chain does not run the fused kernel"
    (ey, pre), _ = S.tail_grads(x, w, s, nz, bias, gy, gain=gain, clamp_=clamp)
    if clamp is not None:
        assert bool((ey.abs() == clamp).any()) and bool((ey.abs() < clamp).any()), "the clamp does not bite"
    for which, yy, gg in (("fused", y, g), ("chain", yc, gc)):
        check(f"{tag} {which} y", yy, ey, tol, REPORT)
        mask = inside = None
        if dtype == torch.bfloat16:
            # Both derivatives jump: the leaky ReLU's at 0, the clamp's at +-c. A bf16 run may sit on the other side than fp64 where fp64's own value is within
            # the bound of the jump, and its gradient then differs there by O(gy) however exact the kernels are. The expected GRADIENT is taken on the side the
            # device was on; the device may differ only within the bound of the jump and on at most 0.5 % of the elements (tests/make_golden_stylegan2.py
            # checks that the restatement with the device's rounding points stays under that cap on these seeds). The forward check knows no mask.
            yd = yy.cpu().double()
            mask = yd > 0
            moved = mask != (pre > 0)
            assert float(pre[moved].abs().max() if bool(moved.any()) else 0.0) <= tol * float(pre.abs().max()), "a sign differs where the value is not small"
            if clamp is not None:
                inside = yd.abs() < clamp
                unclamped = lambda m: S.tail_ref(x, w, s, nz, bias, gain=gain, clamp_=None, mask=m)[0]      # noqa: E731
                moved_c = inside != (ey.abs() < clamp)
                dist = (unclamped(None).abs() - clamp).abs()
                assert float(dist[moved_c].max() if bool(moved_c.any()) else 0.0) <= tol * float(ey.abs().max()), "a clamp side differs away from the bound"
                moved = moved | moved_c
            limit = 0.005 * pre.numel()
            REPORT.append((f"{tag} {which} lrelu / clamp sides that differ from fp64 (count, of {pre.numel()})", float(moved.sum()), limit))
            assert int(moved.sum()) <= limit, int(moved.sum())
        _, eg = S.tail_grads(x, w, s, nz, bias, gy, mask=mask, inside=inside, gain=gain, clamp_=clamp)
        for k in eg:
            check(f"{tag} {which} d{k}", gg[k], eg[k], tol, REPORT)
    if dtype == torch.float32:      # two fp32 evaluations: the same bound between them
        check(f"{tag} fused vs chain y", y, yc.double(), tol, REPORT)
        for k in g:
            check(f"{tag} fused vs chain d{k}", g[k], gc[k].double(), tol, REPORT)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [12, 13, 40])
def test_plain_fir_is_upfirdn2d_bit_for_bit(sg, C, dtype):
    """no epilogue: the NHWC kernel keeps sg_upfirdn2d's tap order (per row an FMA chain over the taps, rows added in order), so it equals upfirdn2d on the NCHW
    copy of the same tensor BIT FOR BIT, fp32 and bf16 (12: a whole number of fp32 vectors, the scalar path in bf16; 13: scalar; 40: vectors)"""
    from studiogan_amd.style_ops.fir_bias_act import fir_nhwc_raw
    from studiogan_amd.style_ops.upfirdn2d import upfirdn2d
    g = torch.Generator().manual_seed(11 + C)
    x = torch.randn(3, C, 9, 11, generator=g).to(DEV, dtype)
    xh = x.permute(0, 2, 3, 1).contiguous()
    f43 = torch.randn(4, 3, generator=g).to(DEV)
    for f, pad, flip, gain in ((R.low_pass().to(DEV), (1, 1, 1, 1), False, 4.0), (R.low_pass().to(DEV), (2, 2, 2, 2), True, 4.0), (f43, (2, 0, 1, 3), False, 1.0),
                               (f43, (0, 1, -1, 3), True, 0.5), (torch.ones(1, 1, device=DEV), (0, -1, 0, 0), False, 4.0)):
        a = fir_nhwc_raw(xh, f, pad, flip, gain).permute(0, 3, 1, 2)
        b = upfirdn2d(x, f, padding=list(pad), flip_filter=flip, gain=gain)
        assert a.shape == b.shape and torch.equal(a.contiguous(), b), (C, pad, flip, float((a.float() - b.float()).abs().max()))
    # a strip boundary: more rows than the tallest strip
    x = torch.randn(1, C, 70, 5, generator=g).to(DEV, dtype)
    a = fir_nhwc_raw(x.permute(0, 2, 3, 1).contiguous(), R.low_pass().to(DEV), (1, 1, 1, 1), False, 4.0).permute(0, 3, 1, 2)
    assert torch.equal(a.contiguous(), upfirdn2d(x, R.low_pass().to(DEV), padding=[1, 1, 1, 1], gain=4.0))


def test_fir_refuses_what_it_does_not_serve(sg):
    from studiogan_amd import _lib as L
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    f = torch.ones(5, 5, device=DEV)
    y = torch.empty(1, 4, 4, 8, device=DEV)
    args = lambda fh, act: (L.F32, x.data_ptr(), f.data_ptr(), y.data_ptr(), None, 0, None, 1, 4, 4, 8, fh, fh, fh // 2, fh - 1 - fh // 2, fh // 2, fh - 1 - fh // 2,      # noqa: E731
                            0, 1.0, act, 0.2, 1.0, -1.0, L.stream())
    with pytest.raises(RuntimeError, match="1..4 taps"):
        L.call("sg_fir_bias_act_nhwc", *args(5, 1))
    with pytest.raises(RuntimeError, match="linear .1. or lrelu"):
        L.call("sg_fir_bias_act_nhwc", *args(3, 4))
    L.call("sg_fir_bias_act_nhwc", *args(3, 3))


# ---- the grouped style affines ----------------------------------------------------------------------------------------------------------------------------

def _generator(fix, tag, **extra):
    from studiogan_amd.backbones import stylegan2 as SG
    G = SG.Generator(**S.kwargs_of(S.CASES[tag], **extra))
    p = f"{tag}/sd/"
    G.load_state_dict({k[len(p):]: v.float() for k, v in fix.items() if k.startswith(p)}, strict=True)
    return G.to(DEV)


def test_grouped_affines_match_the_layers_in_one_launch(sg, fix):
    G = _generator(fix, "skip")
    syn = G.synthesis
    g = torch.Generator().manual_seed(5)
    ws = torch.randn(7, syn.num_ws, syn.w_dim, generator=g)
    lib = sg.lib()
    with torch.no_grad():
        n0 = lib.sg_linear_group_scaled_launches()
        got = [t for blk in syn.prefetch_styles(ws.to(DEV)) for t in blk]
        assert lib.sg_linear_group_scaled_launches() - n0 == 1
        layers = syn.style_layers()
        assert len(got) == len(layers) == 8
        eps = 2.0 ** -24
        for i, ((row, fc, oscale), s) in enumerate(zip(layers, got)):
            own = fc(ws[:, row].to(DEV)) * oscale
            W, b, y = fc.weight.detach().cpu().double() * fc.weight_gain, fc.bias.detach().cpu().double() * fc.bias_gain, ws[:, row].double()
            exp = (y @ W.t() + b) * oscale
            # fp32 rounding: a K-term FMA chain and four scalings, each within eps of the magnitudes it adds
            bound = (W.shape[1] + 4) * eps * (y.abs() @ W.abs().t() + b.abs()) * oscale
            for name, t in (("grouped", s), ("layer", own)):
                d = (t.cpu().double() - exp).abs()
                REPORT.append((f"style affine {i} {name}: max |err| / bound", float((d / bound).max()), 1.0))
                assert bool((d <= bound).all()), (i, name, float((d / bound).max()))
        n0, f0 = lib.sg_linear_group_scaled_launches(), lib.sg_fir_bias_act_launches()
        syn(ws.to(DEV), noise_mode="const")
        assert lib.sg_linear_group_scaled_launches() - n0 == 1, "one launch per synthesis forward"
        assert lib.sg_fir_bias_act_launches() - f0 == 2, "one fused tail per up = 2 layer (b8.conv0, b16.conv0)"
        syn.grouped_styles = False
        for b in syn.blocks():
            b.fused_resample = False
        n0, f0 = lib.sg_linear_group_scaled_launches(), lib.sg_fir_bias_act_launches()
        syn(ws.to(DEV), noise_mode="const")
        assert lib.sg_linear_group_scaled_launches() == n0 and lib.sg_fir_bias_act_launches() == f0


# ---- the networks -----------------------------------------------------------------------------------------------------------------------------------------

def _bound(fix, tag, what):
    return max(2e-5, 4 * float(fix[f"{tag}/ref32_err/{what}"]))


@pytest.mark.parametrize("switches", ["default", "unfused"])
@pytest.mark.parametrize("tag", list(S.CASES))
def test_network_fp32_matches_fixture(sg, fix, tag, switches):
    G = _generator(fix, tag)
    if switches == "unfused":       # the layer-by-layer evaluation: per-layer affines, the chain of operators behind an up = 2 convolution
        G.synthesis.grouped_styles = False
        for b in G.synthesis.blocks():
            b.fused_resample = False
    z, c, gy = (fix[f"{tag}/{k}"].to(DEV) for k in ("z", "c", "gy"))
    z.requires_grad_(True)
    img = G(z, c, noise_mode="const")
    assert img.dtype == torch.float32 and tuple(img.shape) == (S.BATCH, 3, 16, 16)
    check(f"net {tag} {switches} img (ref32_err {float(fix[f'{tag}/ref32_err/img']):.1e})", img, fix[f"{tag}/img"], _bound(fix, tag, "img"), REPORT)
    if tag != "skip":
        return
    with torch.no_grad():
        check(f"net skip {switches} img noise_mode=none", G(z, c, noise_mode="none"), fix["skip/img_none"], _bound(fix, tag, "img_none"), REPORT)
        check(f"net skip {switches} img truncated", G(z, c, noise_mode="const", truncation_psi=0.7, truncation_cutoff=2), fix["skip/img_trunc"],
              _bound(fix, tag, "img_trunc"), REPORT)
        w_avg = G.mapping.w_avg.clone()
        G.mapping(z, c, update_emas=True)
        check(f"net skip {switches} w_avg after one update", G.mapping.w_avg, fix["skip/w_avg_after"], 2e-5, REPORT)
        G.mapping.w_avg.copy_(w_avg)
    params = dict(G.named_parameters())
    gr = torch.autograd.grad(img, [z] + list(params.values()), gy, allow_unused=True)
    check(f"net skip {switches} dz (ref32_err {float(fix['skip/ref32_err/dz']):.1e})", gr[0], fix["skip/dz"], _bound(fix, tag, "dz"), REPORT)
    for (k, _), g in zip(params.items(), gr[1:]):
        e = fix[f"skip/dp/{k}"]
        if float(e.abs().max()) == 0:
            assert g is None or float(g.abs().max()) == 0, k
            continue
        check(f"net skip {switches} d {k} (ref32_err {float(fix[f'skip/ref32_err/dp/{k}']):.1e})", g, e, _bound(fix, tag, f"dp/{k}"), REPORT)


@pytest.mark.parametrize("tag", list(S.CASES))
def test_network_bf16_blocks(sg, fix, tag):
    G = _generator(fix, tag, **S.LOWP)
    acts = {}
    hooks = [b.register_forward_hook(lambda m, i, o: acts.__setitem__(m.resolution, o[0])) for b in G.synthesis.blocks()]
    with torch.no_grad():
        img = G(fix[f"{tag}/z"].to(DEV), fix[f"{tag}/c"].to(DEV), noise_mode="const")
    for h in hooks:
        h.remove()
    assert img.dtype == torch.float32 and img.is_contiguous()
    assert acts[4].dtype == torch.float32
    for r in (8, 16):
        assert acts[r].dtype == torch.bfloat16 and acts[r].is_contiguous(memory_format=torch.channels_last), r
    floor = float(fix[f"{tag}/bf16_floor"])
    check(f"net {tag} bf16 blocks img (bf16_floor {floor:.2e})", img, fix[f"{tag}/img_lowp"], 3 * floor, REPORT)


def test_random_noise_and_the_two_halves(sg, fix):
    G = _generator(fix, "skip")
    z, c = fix["skip/z"].to(DEV), fix["skip/c"].to(DEV)
    with torch.no_grad():
        a, b = G(z, c), G(z, c)      # noise_mode defaults to 'random'
        assert a.dtype == torch.float32 and tuple(a.shape) == (S.BATCH, 3, 16, 16) and bool(torch.isfinite(a).all())
        assert not torch.equal(a, b)
        # sampling code calls the two networks separately
        ws = G.mapping(z, c, truncation_psi=0.7, truncation_cutoff=2)
        assert tuple(ws.shape) == (S.BATCH, G.num_ws, 40)
        assert torch.equal(G.synthesis(ws, noise_mode="const"), G(z, c, noise_mode="const", truncation_psi=0.7, truncation_cutoff=2))
