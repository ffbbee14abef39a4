"""CPU: the one-launch filtered_lrelu backward (sg_filtered_lrelu_gate / sg_filtered_lrelu_bwd, csrc/style.hip) through the interpreter (tests/hipemu) on the
operator cases of tests/stylegan3_opcases.py, the operator's routing rules and refusals; the StyleGAN3 networks' contract with the reference (state_dict, argument
lists, geometry, filters) and the fixture tests/golden/stylegan3_gen.npz against the restatement that wrote it; config_map.stylegan3_generator_args over the
reference's configuration files. Bounds are those of tests/test_stylegan3_gpu.py. No GPU."""
import os
import shutil
import sys

import pytest
import torch

import stylegan3_opcases as OC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
emulated = pytest.mark.skipif(shutil.which(os.environ.get("CXX", "g++")) is None, reason="the interpreter needs a host C++ compiler")
FP32_TOL = 3e-5         # of the largest expected element: the bound tests/test_style_gpu.py holds the same quantities to


def _err(a, e):
    return float((a.double() - e).abs().max() / e.abs().max())


def _run(E, tag, dtype, write_gate=True, backward=True):
    """the operator's autograd Function on CPU tensors behind the interpreter: y, dx, db, the gate plane [P, AH, AW]"""
    from studiogan_amd.style_ops import filtered_lrelu as FL
    shape, nu, nd, up, down, pad, gain, slope, clamp, flip = OC.CASES[tag]
    c = OC.inputs(tag)
    x, b = c["x"].to(dtype).requires_grad_(write_gate), c["b"].to(dtype).requires_grad_(write_gate)
    cfg = (up, down, FL._parse_padding(pad), float(gain), float(slope), clamp, flip)
    seen = {}
    keep = FL._fused_backward

    def spy(dy, x_, gate, *a):          # the gate plane is not public: take it where the backward receives it
        seen["gate"] = gate
        return keep(dy, x_, gate, *a)
    FL._fused_backward = spy
    try:
        y = FL._FilteredLRelu.apply(x, b, c["fu"], c["fd"], cfg)
        if not (write_gate and backward):
            return y.detach(), None, None, None
        dx, db = torch.autograd.grad(y, [x, b], c["gy"].to(dtype))
    finally:
        FL._fused_backward = keep
    aw = c["gate"].shape[-1]
    return y.detach(), dx, db, OC.unpack_gate(seen["gate"], aw)


@emulated
@pytest.mark.parametrize("tag", list(OC.CASES))
def test_fused_backward_through_the_interpreter(tag):
    """fp32: y of the gate-writing forward equals the plain forward bit for bit; the gate plane equals the fp64 restatement's gates; dx and db of the one
    backward launch meet the fp64 expectation at the GPU test's bound; one sg_filtered_lrelu_bwd launch and no sg_upfirdn2d launch. Several host threads,
    so that two workgroups storing into one gate byte would show."""
    import fullemu
    c = OC.inputs(tag)
    with fullemu.Installed() as E:
        E.lib.hipemu_threads(4)
        try:
            n = lambda: (E.lib.sg_filtered_lrelu_launches(0), E.lib.sg_filtered_lrelu_launches(1), E.lib.sg_filtered_lrelu_launches(2),      # noqa: E731
                         E.lib.sg_upfirdn2d_launches())
            n0 = n()
            y0 = _run(E, tag, torch.float32, write_gate=False)[0]
            assert tuple(a - b for a, b in zip(n(), n0)) == (1, 0, 0, 0)
            n0 = n()
            y, dx, db, gate = _run(E, tag, torch.float32)
            assert tuple(a - b for a, b in zip(n(), n0)) == (0, 1, 1, 0), "forward with gates and backward are one launch each, the chain does not run"
        finally:
            E.lib.hipemu_threads(1)
    assert torch.equal(y, y0)
    assert _err(y, c["y"]) <= FP32_TOL
    assert torch.equal(gate, c["gate"]), f"{int((gate != c['gate']).sum())} gates differ from fp64"
    assert tuple(dx.shape) == tuple(c["dx"].shape) and _err(dx, c["dx"]) <= FP32_TOL, _err(dx, c["dx"])
    assert _err(db, c["db"]) <= FP32_TOL, _err(db, c["db"])


@emulated
@pytest.mark.parametrize("tag", ["t_layer", "clamp_flip"])
def test_fused_backward_bf16_through_the_interpreter(tag):
    """bf16 storage, fp32 arithmetic in LDS: within 3 x what bf16 storage alone costs the fp64 restatement; gate flips against fp64 under the 0.5 % cap"""
    import fullemu
    c, floor = OC.inputs(tag), OC.bf16_floor(tag)
    assert floor["flips"] <= 0.005
    with fullemu.Installed() as E:
        y, dx, db, gate = _run(E, tag, torch.bfloat16)
    assert float((gate != c["gate"]).double().mean()) <= 0.005
    assert _err(y, c["y"]) <= 3 * floor["y"] and _err(dx, c["dx"]) <= 3 * floor["dx"] and _err(db, c["db"]) <= 3 * floor["db"]


# ---- routing and refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_operator_refusals_and_switches():
    from studiogan_amd.style_ops import filtered_lrelu as FL
    from studiogan_amd.style_ops import modulated_conv2d_full as MF
    assert FL._FUSED_BWD == [True] and FL._FUSED == [True]
    x = torch.randn(2, 4, 8, 8)
    with pytest.raises(RuntimeError):           # CPU tensors: the chain's operators refuse them, there is no CPU path
        FL.filtered_lrelu(x, b=torch.randn(4))
    w, s = torch.randn(5, 4, 3, 3), torch.randn(2, 4)
    with pytest.raises(NotImplementedError, match="float16"):
        MF.modulated_conv2d(x.half(), w, s, padding=2)
    with pytest.raises(NotImplementedError, match="padding"):
        MF.modulated_conv2d(x, w, s, padding=1)
    with pytest.raises(NotImplementedError, match="input_gain"):
        MF.modulated_conv2d(x, w, s, padding=2, input_gain=torch.ones(4))
    with pytest.raises(RuntimeError):           # CPU tensors
        MF.modulated_conv2d(x, w, s, padding=2)


@emulated
def test_create_graph_leaves_the_fused_route():
    """under create_graph the backward does not launch sg_filtered_lrelu_bwd: it re-runs the operator chain, whose first operator refuses the interpreter's CPU
    tensors (the chain itself is tests/test_stylegan3_gpu.py's to check)"""
    import fullemu
    from studiogan_amd.style_ops import filtered_lrelu as FL
    tag = "critical"
    shape, nu, nd, up, down, pad, gain, slope, clamp, flip = OC.CASES[tag]
    c = OC.inputs(tag)
    with fullemu.Installed() as E:
        x, b = c["x"].float().requires_grad_(True), c["b"].float().requires_grad_(True)
        n0 = E.lib.sg_filtered_lrelu_launches(2)
        y = FL._FilteredLRelu.apply(x, b, c["fu"], c["fd"], (up, down, FL._parse_padding(pad), float(gain), float(slope), clamp, flip))
        with pytest.raises(RuntimeError, match="bias_act"):
            torch.autograd.grad(y, x, c["gy"].float(), create_graph=True)
        assert E.lib.sg_filtered_lrelu_launches(2) == n0
        dx, = torch.autograd.grad(y, x, c["gy"].float())
        assert E.lib.sg_filtered_lrelu_launches(2) == n0 + 1 and _err(dx, c["dx"]) <= FP32_TOL


# ---- the networks -----------------------------------------------------------------------------------------------------------------------------------------

import inspect      # noqa: E402

import numpy as np      # noqa: E402

import stylegan3_ref as R3      # noqa: E402

from oracle import ref_import as RI      # noqa: E402

REF = RI.REF_SRC


@pytest.fixture(scope="module")
def fix():
    return R3.load_golden()


def _sd(fix, tag, dtype=torch.float64):
    return {str(k): torch.from_numpy(fix[f"{tag}/sd/{k}"]).to(dtype) for k in fix[f"{tag}/keys"]}


@pytest.mark.parametrize("tag", list(R3.CASES))
def test_restatement_reproduces_the_fixture(fix, tag):
    sd = _sd(fix, tag)
    z, c, gy = (torch.from_numpy(fix[f"{tag}/{k}"]).double() for k in "z c gy".split())
    params = [k for k in fix if k.startswith(f"{tag}/dp/")]
    img, dz, dp = R3.generator_grads(sd, fix, tag, z, c, gy, [k[len(tag) + 4:] for k in params])
    assert _err(img, torch.from_numpy(fix[f"{tag}/img"])) <= 1e-12 and _err(dz, torch.from_numpy(fix[f"{tag}/dz"])) <= 1e-12
    for k in params:
        e = torch.from_numpy(fix[k])
        assert float((dp[k[len(tag) + 4:]] - e).abs().max()) <= 1e-12 * max(float(e.abs().max()), 1e-300), k
    assert _err(R3.generator(sd, fix, tag, z, c, psi=0.7, cutoff=3), torch.from_numpy(fix[f"{tag}/img_trunc"])) <= 1e-12
    # the conditions the fixture was generated under are stored facts: the reference's own fp32 error is small, the bf16 floor belongs to the low-precision case
    assert all(float(fix[k]) < 2e-5 for k in fix if k.startswith(f"{tag}/ref32_err/"))
    assert (f"{tag}/bf16_floor" in fix) == (tag == "t32_lowp")


@pytest.mark.parametrize("tag", list(R3.CASES))
def test_state_dict_contract_and_geometry(fix, tag):
    """the reference's keys in its order, strict loading, num_ws, layer names L{idx}_{size}_{channels}, per-layer factors / paddings / kernels / precision and the
    designed filters, all as recorded from the reference's network"""
    from studiogan_amd.backbones import stylegan3
    G = stylegan3.Generator(**R3.kwargs_of(R3.CASES[tag]))
    keys = [str(k) for k in fix[f"{tag}/keys"]]
    assert list(G.state_dict().keys()) == keys
    for k, v in G.state_dict().items():
        assert tuple(v.shape) == tuple(fix[f"{tag}/sd/{k}"].shape) and v.dtype == torch.float32, k
        if k.endswith(("up_filter", "down_filter")):       # design_lowpass_filter against the reference's filters
            assert float((v - torch.from_numpy(fix[f"{tag}/sd/{k}"])).abs().max()) <= 1e-7, k
    G.load_state_dict(_sd(fix, tag, torch.float32), strict=True)
    assert G.num_ws == int(fix[f"{tag}/num_ws"]) == G.synthesis.num_ws
    layers, (size, rate, band) = R3.layer_meta(fix, tag)
    assert G.synthesis.layer_names == [m[0] for m in layers]
    for name, up, down, pad, k, torgb, lowp in layers:
        m = getattr(G.synthesis, name)
        assert (m.up_factor, m.down_factor, m.padding, m.conv_kernel, m.is_torgb, m.use_fp16) == (up, down, pad, k, torgb, lowp), name
        assert name == f"L{G.synthesis.layer_names.index(name)}_{int(m.out_size[0])}_{m.out_channels}"
        assert (m.down_filter is not None and m.down_filter.dim() == 2) == m.down_radial
    inp = G.synthesis.input
    assert (int(inp.size[0]), float(inp.sampling_rate), float(inp.bandwidth)) == (size, rate, band)
    assert any(getattr(G.synthesis, m[0]).down_radial for m in layers) == (tag == "r")


def test_design_lowpass_filter():
    from studiogan_amd.backbones.stylegan3 import SynthesisLayer, design_lowpass_filter
    assert design_lowpass_filter(1, 2, 1, 8) is None and SynthesisLayer.design_lowpass_filter(1, 2, 1, 8) is None
    f = design_lowpass_filter(12, 2.0, 2.5, 16.0)
    assert f.dtype == torch.float32 and tuple(f.shape) == (12,) and abs(float(f.sum()) - 1) < 1e-6 and torch.equal(f, f.flip(0))
    r = design_lowpass_filter(12, 2.0, 2.5, 16.0, radial=True)
    assert tuple(r.shape) == (12, 12) and abs(float(r.sum()) - 1) < 1e-6 and torch.equal(r, r.t()) and float((r - r.flip(0, 1)).abs().max()) < 1e-8
    with pytest.raises(AssertionError):
        design_lowpass_filter(0, 2, 1, 8)


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout")
def test_argument_lists_match_the_reference():
    import importlib
    from oracle import ref_import as RI
    from studiogan_amd.backbones import stylegan3
    RI._prepare()
    ref = importlib.import_module("models.stylegan3")
    for cls in ("SynthesisInput", "SynthesisLayer", "SynthesisNetwork", "Generator", "MappingNetwork", "FullyConnectedLayer"):
        for fn in ("__init__", "forward"):
            a, b = inspect.signature(getattr(getattr(stylegan3, cls), fn)), inspect.signature(getattr(getattr(ref, cls), fn))
            assert [(p.name, p.default, p.kind) for p in a.parameters.values()] == [(p.name, p.default, p.kind) for p in b.parameters.values()], (cls, fn)


def test_network_refusals():
    from studiogan_amd.backbones import stylegan3
    G = stylegan3.Generator(**R3.kwargs_of(R3.CASES["t_cond"]))
    z, c = torch.randn(2, 16), torch.eye(3)[:2]
    with pytest.raises(RuntimeError):           # CPU tensors: the convolution refuses them
        G(z, c)
    layer = getattr(G.synthesis, G.synthesis.layer_names[0])
    x = torch.randn(2, layer.in_channels, int(layer.in_size[1]), int(layer.in_size[0]))
    with pytest.raises(AssertionError, match="w must be"):
        layer(x, torch.randn(2, 5))
    with pytest.raises(AssertionError, match="x must be"):
        layer(x[:, :, :-1], torch.randn(2, 16))
    with pytest.raises(AssertionError, match="ws must be"):
        G.synthesis(torch.randn(2, 3, 16))
    from studiogan_amd.style_ops import modulated_conv2d_full as MF
    with pytest.raises(NotImplementedError, match="float16"):       # use_fp16 means bfloat16 here
        MF.modulated_conv2d(x.half(), layer.weight, torch.randn(2, layer.in_channels), padding=2)


def test_input_layer_emas_and_truncation_on_the_cpu(fix):
    """what is plain torch runs anywhere: the Fourier-feature input layer under a non-identity transform, the truncation, and the magnitude_ema update (made in
    front of the convolution, which then refuses the CPU tensor) against the fixture"""
    from studiogan_amd.backbones import stylegan3
    tag = "t_cond"
    G = stylegan3.Generator(**R3.kwargs_of(R3.CASES[tag]))
    G.load_state_dict(_sd(fix, tag, torch.float32), strict=True)
    assert not torch.equal(G.synthesis.input.transform, torch.eye(3))
    ws = torch.from_numpy(fix[f"{tag}/ws"])
    layers, geo = R3.layer_meta(fix, tag)
    x0 = R3.synthesis_input(_sd(fix, tag), geo, ws[:, 0])
    with torch.no_grad():
        got = G.synthesis.input(ws[:, 0].float())
    assert tuple(got.shape) == tuple(x0.shape) and _err(got, x0) <= 2e-5
    w = ws[:, 0].float()
    assert _err(G.mapping.broadcast_truncate(w, 0.7, 3), torch.from_numpy(fix[f"{tag}/ws_trunc"])) <= 1e-6
    assert _err(G.mapping.broadcast_truncate(w, update_emas=True), ws) <= 1e-6
    assert _err(G.mapping.w_avg, torch.from_numpy(fix[f"{tag}/w_avg_after"])) <= 1e-6
    layer = getattr(G.synthesis, layers[0][0])
    assert float(layer.magnitude_ema) != 1.0
    with pytest.raises(RuntimeError):
        layer(got, ws[:, 1].float(), update_emas=True)
    assert _err(layer.magnitude_ema, torch.from_numpy(fix[f"{tag}/magnitude_ema_after/{layers[0][0]}"])) <= 2e-5


# ---- configuration ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout")
def test_generator_args_of_every_stylegan3_config():
    import glob
    import yaml
    from studiogan_amd import config_map
    from studiogan_amd.backbones import stylegan3
    ctor = [p for p in inspect.signature(stylegan3.Generator.__init__).parameters if p != "self"]
    seen = []
    for f in sorted(glob.glob(os.path.join(REF, "configs", "*", "*.yaml"))):
        y = yaml.safe_load(open(f))
        if (y.get("MODEL") or {}).get("backbone") != "stylegan3":
            continue
        seen.append("/".join(f.split("/")[-2:]))
        rot = y["STYLEGAN"]["stylegan3_cfg"] == "stylegan3-r"
        for mixed in (False, True):
            kw = config_map.stylegan3_generator_args(y, mixed_precision=mixed)
            assert sorted(kw) == sorted(ctor), f
            s = kw["synthesis_kwargs"]
            assert (s["channel_base"], s["channel_max"], s["conv_kernel"], s["use_radial_filters"]) == ((65536, 1024, 1, True) if rot else (32768, 512, 3, False)), f
            assert (s["num_fp16_res"], s["conv_clamp"]) == ((4, 256) if mixed else (0, None))
            O = y["OPTIMIZATION"]
            assert s["magnitude_ema_beta"] == 0.5 ** (O["batch_size"] * O.get("acml_steps", 1) / 20e3), f
            assert kw["c_dim"] == (y["DATA"]["num_classes"] if y["MODEL"].get("g_cond_mtd", "W/O") == "cAdaIN" else 0), f
            assert kw["img_resolution"] == y["DATA"]["img_size"] and kw["mapping_kwargs"] == {"num_layers": y["STYLEGAN"]["mapping_network"]}
            d = config_map.stylegan2_discriminator_args(y, mixed_precision=mixed)       # the reference pairs it with the StyleGAN2 discriminator at 32768
            assert d["channel_base"] == 32768 and d["img_resolution"] == y["DATA"]["img_size"]
        assert config_map.stylegan2_r1_args(y)["d_reg_interval"] == y["STYLEGAN"]["d_reg_interval"]
        with pytest.raises(NotImplementedError):
            config_map.model_args(y)
        with pytest.raises(NotImplementedError):
            config_map.stylegan2_generator_args(y)
    assert len(seen) == 8 and "CIFAR10/StyleGAN3-t-ADA.yaml" in seen and "AFHQv2/StyleGAN3-r-paper.yaml" in seen, seen
    G = stylegan3.Generator(**config_map.stylegan3_generator_args(yaml.safe_load(open(os.path.join(REF, "configs", "CIFAR10", "StyleGAN3-t-ADA.yaml")))))
    assert G.num_ws == 16 and G.synthesis.layer_names[-1] == "L14_32_3"
    # a StyleGAN2 configuration maps as before
    cifar = yaml.safe_load(open(os.path.join(REF, "configs", "CIFAR10", "StyleGAN2.yaml")))
    assert config_map.stylegan2_discriminator_args(cifar)["channel_base"] == 32768
    kw = config_map.stylegan2_r1_args(cifar)
    assert kw["lr"] == 0.0025 * 16 / 17 and kw["betas"] == [0.0, 0.99 ** (16 / 17)]
    afhq = dict(cifar, DATA=dict(cifar["DATA"], name="AFHQv2", img_size=256))
    assert config_map.stylegan2_discriminator_args(afhq)["channel_base"] == 16384       # (only a stylegan3 configuration lifts it to 32768)
    with pytest.raises(NotImplementedError):
        config_map.stylegan3_generator_args(cifar)
    with pytest.raises(NotImplementedError):
        config_map.stylegan2_discriminator_args({"MODEL": {"backbone": "big_resnet"}})
