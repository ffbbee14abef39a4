"""GPU: the one-launch filtered_lrelu backward (sg_filtered_lrelu_gate / sg_filtered_lrelu_bwd) on the operator cases of tests/stylegan3_opcases.py, and the
StyleGAN3 generator (backbones/stylegan3.py) against the fixture tests/golden/stylegan3_gen.npz (tests/make_golden_stylegan3.py).
Operator, fp32: 3e-5 of the largest expected element, the bound tests/test_style_gpu.py holds the same quantities to. bf16: 3 x what bf16 storage alone costs the fp64
restatement (stylegan3_opcases.bf16_floor), gate flips against fp64 at most 0.5 %. Networks: fp32 max(2e-5, 4 ref32_err), bf16 layers 3 x bf16_floor.
Every measured error goes to profiles/stylegan3_pytest_gpu.txt when the module is done."""
import os

import numpy as np
import pytest
import torch

import stylegan3_opcases as OC
import stylegan3_ref as R3
from util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "stylegan3_gen.npz")
REPORT = []
FP32_TOL = 3e-5
FLIP_CAP = 0.005


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    try:
        with open(os.path.join(HERE, "..", "profiles", "stylegan3_pytest_gpu.txt"), "w") as f:
            f.write("tests/test_stylegan3_gpu.py on %s: max |got - expected| / max |expected| of every check (operator fp32: 3e-5; bf16: 3 x the floor of bf16 "
                    "storage; networks: max(2e-5, 4 ref32_err), bf16 layers 3 bf16_floor; gate flips: share of gates)\n" % torch.cuda.get_device_name(0))
            for name, e, tol in REPORT:
                f.write(f"{name:84s} err={e:.3e} tol={tol:.2e}\n")
    except OSError:
        pass


def _launches():
    from studiogan_amd import _lib as L
    lib = L.lib()
    return np.array([lib.sg_filtered_lrelu_launches(0), lib.sg_filtered_lrelu_launches(1), lib.sg_filtered_lrelu_launches(2), lib.sg_upfirdn2d_launches()])


def _op(tag, dtype, fused_bwd=True, grad=True, fd2d=False, create_graph=False):
    """the public operator on a case: y, dx, db, the launches (plain forward, gate forward, backward, sg_upfirdn2d) it made, the gate plane if one was written"""
    from studiogan_amd.style_ops import filtered_lrelu as FL
    shape, nu, nd, up, down, pad, gain, slope, clamp, flip = OC.CASES[tag]
    c = OC.inputs(tag)
    x, b = c["x"].to(DEV, dtype).requires_grad_(grad), c["b"].to(DEV, dtype).requires_grad_(grad)
    fu, fd = (None if c["fu"] is None else c["fu"].to(DEV)), (None if c["fd"] is None else c["fd"].to(DEV))
    if fd2d:
        fd = torch.outer(fd, fd)
    seen, keep, keep_flag = {}, FL._fused_backward, FL._FUSED_BWD[0]

    def spy(dy, x_, gate, *a):
        seen["gate"] = gate
        return keep(dy, x_, gate, *a)
    FL._fused_backward, FL._FUSED_BWD[0] = spy, fused_bwd
    n0 = _launches()
    try:
        y = FL.filtered_lrelu(x, fu=fu, fd=fd, b=b, up=up, down=down, padding=pad, gain=gain, slope=slope, clamp=clamp, flip_filter=flip)
        dx = db = None
        if grad:
            dx, db = torch.autograd.grad(y, [x, b], c["gy"].to(DEV, dtype), create_graph=create_graph)
    finally:
        FL._fused_backward, FL._FUSED_BWD[0] = keep, keep_flag
    torch.cuda.synchronize()
    gate = OC.unpack_gate(seen["gate"].cpu(), c["gate"].shape[-1]) if "gate" in seen else None
    return y, dx, db, tuple(_launches() - n0), gate, (x, b)


@pytest.mark.parametrize("tag", list(OC.CASES))
def test_fused_backward_fp32(sg, tag):
    c = OC.inputs(tag)
    y, dx, db, n, gate, _ = _op(tag, torch.float32)
    assert n == (0, 1, 1, 0), f"one gate-writing forward, one sg_filtered_lrelu_bwd, no sg_upfirdn2d: saw {n}"
    check(f"filtered_lrelu {tag} y", y, c["y"], FP32_TOL, REPORT)
    check(f"filtered_lrelu {tag} fused dx", dx, c["dx"], FP32_TOL, REPORT)
    check(f"filtered_lrelu {tag} fused db", db, c["db"], FP32_TOL, REPORT)
    assert torch.equal(gate, c["gate"]), f"{int((gate != c['gate']).sum())} gates differ from fp64"
    y1, dx1, db1, n1, _, _ = _op(tag, torch.float32, fused_bwd=False)
    assert n1[:3] == (1, 0, 0) and n1[3] >= 4, f"the chain route: a plain forward, then the two upfirdn2d operators each way (one or two launches each): saw {n1}"
    check(f"filtered_lrelu {tag} fused vs chain dx", dx, dx1.detach().double().cpu(), FP32_TOL, REPORT)
    check(f"filtered_lrelu {tag} fused vs chain db", db, db1.detach().double().cpu(), FP32_TOL, REPORT)
    y0, _, _, n0, _, _ = _op(tag, torch.float32, grad=False)
    assert n0 == (1, 0, 0, 0), "no gradient wanted: the plain forward, no gate plane"
    assert torch.equal(y, y0) and torch.equal(y1, y0), "the gate-writing forward changes y"


@pytest.mark.parametrize("tag", list(OC.CASES))
def test_fused_backward_bf16(sg, tag):
    c, floor = OC.inputs(tag), OC.bf16_floor(tag)
    assert floor["flips"] <= FLIP_CAP
    y, dx, db, n, gate, _ = _op(tag, torch.bfloat16)
    assert n == (0, 1, 1, 0)
    flips = float((gate != c["gate"]).double().mean())
    REPORT.append((f"filtered_lrelu {tag} bf16 gate flips against fp64", flips, FLIP_CAP))
    assert flips <= FLIP_CAP
    check(f"filtered_lrelu {tag} bf16 y (floor {floor['y']:.2e})", y.float(), c["y"], 3 * floor["y"], REPORT)
    check(f"filtered_lrelu {tag} bf16 fused dx (floor {floor['dx']:.2e})", dx.float(), c["dx"], 3 * floor["dx"], REPORT)
    check(f"filtered_lrelu {tag} bf16 fused db (floor {floor['db']:.2e})", db.float(), c["db"], 3 * floor["db"], REPORT)


def test_which_backward_runs(sg):
    """separable filters: one sg_filtered_lrelu_bwd and no sg_upfirdn2d; a 2-D filter and create_graph: the chain"""
    assert _op("critical", torch.float32)[3] == (0, 1, 1, 0)
    n = _op("critical", torch.float32, fd2d=True)[3]
    assert n[:3] == (0, 0, 0) and n[3] >= 4, f"a 2-D down filter runs the chain under autograd, two upfirdn2d operators each way: saw {n}"
    n = _op("critical", torch.float32, create_graph=True)[3]
    assert n[:3] == (0, 1, 0) and n[3] >= 4, f"create_graph: the backward re-runs and differentiates the chain: saw {n}"


@pytest.mark.parametrize("tag", ["critical", "clamp_flip"])
def test_double_backward_under_create_graph(sg, tag):
    """the operator is piecewise linear in x: the gradient of <dx, r> with respect to gy is the forward's Jacobian applied to r (fp64: autograd on the
    restatement); first order under create_graph still meets the expectation"""
    from oracle import style_ref as SR
    shape, nu, nd, up, down, pad, gain, slope, clamp, flip = OC.CASES[tag]
    c = OC.inputs(tag)
    from studiogan_amd.style_ops import filtered_lrelu as FL
    x, b = c["x"].to(DEV, torch.float32).requires_grad_(True), c["b"].to(DEV, torch.float32).requires_grad_(True)
    gy = c["gy"].to(DEV, torch.float32).requires_grad_(True)
    y = FL.filtered_lrelu(x, fu=c["fu"].to(DEV), fd=c["fd"].to(DEV), b=b, up=up, down=down, padding=pad, gain=gain, slope=slope, clamp=clamp, flip_filter=flip)
    dx, = torch.autograd.grad(y, x, gy, create_graph=True)
    check(f"filtered_lrelu {tag} create_graph dx", dx, c["dx"], FP32_TOL, REPORT)
    r = (torch.randn(shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 16).round() / 16
    ggy, = torch.autograd.grad(dx, gy, r.to(DEV, torch.float32))
    x64, gy64 = c["x"].clone().requires_grad_(True), c["gy"].clone().requires_grad_(True)
    y64 = SR.filtered_lrelu(x64, fu=c["fu"].double(), fd=c["fd"].double(), b=c["b"], up=up, down=down, padding=pad, gain=gain, slope=slope, clamp=clamp, flip_filter=flip)
    dx64, = torch.autograd.grad(y64, x64, gy64, create_graph=True)
    ggy64, = torch.autograd.grad(dx64, gy64, r)
    check(f"filtered_lrelu {tag} double backward", ggy, ggy64, FP32_TOL, REPORT)


# ---- the generator ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fix():
    return R3.load_golden()


def _generator(fix, tag):
    from studiogan_amd.backbones import stylegan3
    G = stylegan3.Generator(**R3.kwargs_of(R3.CASES[tag]))
    G.load_state_dict({str(k): torch.from_numpy(fix[f"{tag}/sd/{k}"]) for k in fix[f"{tag}/keys"]}, strict=True)
    return G.to(DEV)


def _bound(fix, tag, what):
    return max(2e-5, 4 * float(fix[f"{tag}/ref32_err/{what}"]))


def _t(fix, key):
    return torch.from_numpy(fix[key])


@pytest.mark.parametrize("fused", [True, False], ids=["fused_bwd", "chain_bwd"])
@pytest.mark.parametrize("tag", list(R3.CASES))
def test_generator_matches_fixture_fp32(sg, fix, tag, fused):
    """img, dz and every parameter gradient in fp32 (low-precision layers forced to fp32) against the fp64 expectation, at max(2e-5, 4 ref32_err)"""
    from studiogan_amd.style_ops import filtered_lrelu as FL
    G = _generator(fix, tag)
    z, c, gy = (_t(fix, f"{tag}/{k}").to(DEV) for k in "z c gy".split())
    z.requires_grad_(True)
    params = dict(G.named_parameters())
    FL._FUSED_BWD[0] = fused
    n0 = _launches()
    try:
        img = G(z, c, force_fp32=True)
        gr = torch.autograd.grad(img, [z] + list(params.values()), gy, allow_unused=True)
    finally:
        FL._FUSED_BWD[0] = True
    n = _launches() - n0
    assert (n[2] > 0) == fused and (fused or n[1] == 0), f"launches {tuple(n)}"
    name = f"net {tag} {'fused' if fused else 'chain'} backward"
    check(f"{name} img (ref32_err {float(fix[f'{tag}/ref32_err/img']):.1e})", img, _t(fix, f"{tag}/img"), _bound(fix, tag, "img"), REPORT)
    check(f"{name} dz (ref32_err {float(fix[f'{tag}/ref32_err/dz']):.1e})", gr[0], _t(fix, f"{tag}/dz"), _bound(fix, tag, "dz"), REPORT)
    for (k, p), g in zip(params.items(), gr[1:]):
        e = _t(fix, f"{tag}/dp/{k}")
        g = torch.zeros_like(p) if g is None else g
        if float(e.abs().max()) == 0:
            assert float(g.abs().max()) == 0.0, k
            continue
        check(f"{name} d {k} (ref32_err {float(fix[f'{tag}/ref32_err/dp/{k}']):.1e})", g, e, _bound(fix, tag, f"dp/{k}"), REPORT)


@pytest.mark.parametrize("fused", [True, False], ids=["fused_bwd", "chain_bwd"])
def test_generator_bf16_layers(sg, fix, fused):
    """the case with low-precision layers, run as built: img, dz and every parameter gradient within 3 x the fixture's bf16_floor of the fp64 expectation"""
    from studiogan_amd.style_ops import filtered_lrelu as FL
    tag = "t32_lowp"
    G = _generator(fix, tag)
    assert any(getattr(G.synthesis, n).use_fp16 for n in G.synthesis.layer_names)
    floor = float(fix[f"{tag}/bf16_floor"])
    z, c, gy = (_t(fix, f"{tag}/{k}").to(DEV) for k in "z c gy".split())
    z.requires_grad_(True)
    params = dict(G.named_parameters())
    FL._FUSED_BWD[0] = fused
    try:
        img = G(z, c)
        gr = torch.autograd.grad(img, [z] + list(params.values()), gy, allow_unused=True)
    finally:
        FL._FUSED_BWD[0] = True
    name = f"net {tag} bf16 layers {'fused' if fused else 'chain'} backward"
    check(f"{name} img (bf16_floor {floor:.2e})", img, _t(fix, f"{tag}/img"), 3 * floor, REPORT)
    check(f"{name} dz", gr[0], _t(fix, f"{tag}/dz"), 3 * floor, REPORT)
    for (k, p), g in zip(params.items(), gr[1:]):
        e = _t(fix, f"{tag}/dp/{k}")
        if float(e.abs().max()) > 0:
            check(f"{name} d {k}", g, e, 3 * floor, REPORT)


def test_generator_emas_and_truncation(sg, fix):
    tag = "t_cond"
    G = _generator(fix, tag)
    z, c = _t(fix, f"{tag}/z").to(DEV), _t(fix, f"{tag}/c").to(DEV)
    with torch.no_grad():
        check("net t_cond ws", G.mapping(z, c), _t(fix, f"{tag}/ws"), 2e-5, REPORT)
        check("net t_cond ws truncated", G.mapping(z, c, truncation_psi=0.7, truncation_cutoff=3), _t(fix, f"{tag}/ws_trunc"), 2e-5, REPORT)
        check("net t_cond img truncated", G(z, c, truncation_psi=0.7, truncation_cutoff=3), _t(fix, f"{tag}/img_trunc"), _bound(fix, tag, "img_trunc"), REPORT)
        check("net t_cond img update_emas", G(z, c, update_emas=True), _t(fix, f"{tag}/img_ema"), _bound(fix, tag, "img_ema"), REPORT)
    check("net t_cond w_avg after one update", G.mapping.w_avg, _t(fix, f"{tag}/w_avg_after"), 2e-5, REPORT)
    for n in G.synthesis.layer_names:
        check(f"net t_cond {n}.magnitude_ema after one update", getattr(G.synthesis, n).magnitude_ema, _t(fix, f"{tag}/magnitude_ema_after/{n}"), 2e-5, REPORT)
