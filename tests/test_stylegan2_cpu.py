"""Host-side checks of the StyleGAN2 generator networks (backbones/stylegan2.py): the fixture tests/golden/stylegan2_gen.npz against the restatement that
wrote its expectation, the state_dict contract with the reference, the ws bookkeeping, truncation and the w_avg update on the mapping network's torch path,
the refusals, the table of the grouped style affines, config_map.stylegan2_generator_args over the reference's configuration files, and the fused layer tail
(sg_fir_bias_act_nhwc with its autograd function) through the kernel-source interpreter. No GPU."""
import ctypes
import glob
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu  # noqa: E402
import modconv_ref as R  # noqa: E402
import stylegan2_dis_ref as D  # noqa: E402
import stylegan2_ref as S  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in S.load_golden().items()}


def _sd(fix, tag, dtype=torch.float64):
    p = f"{tag}/sd/"
    return {k[len(p):]: v.to(dtype) for k, v in fix.items() if k.startswith(p)}


def _gen(tag, **extra):
    from studiogan_amd.backbones import stylegan2 as SG
    return SG.Generator(**S.kwargs_of(S.CASES[tag], **extra))


def _err(a, b):
    return float((a.double() - b.double()).abs().max() / float(b.double().abs().max()))


@pytest.mark.parametrize("tag", list(S.CASES))
def test_restatement_reproduces_the_fixture(fix, tag):
    cfg, sd = S.CASES[tag], _sd(fix, tag)
    z, c = fix[f"{tag}/z"].double(), fix[f"{tag}/c"].double()
    assert _err(S.generator(sd, cfg, z, c, "const"), fix[f"{tag}/img"]) <= 1e-12
    assert _err(S.generator(sd, cfg, z, c, "const", **S.LOWP), fix[f"{tag}/img_lowp"]) <= 1e-12
    # the fp32 evaluation of the same statement sits where the reference's own fp32 evaluation does
    sd32 = _sd(fix, tag, torch.float32)
    e32 = _err(S.generator(sd32, cfg, z.float(), c.float(), "const"), fix[f"{tag}/img"])
    assert e32 <= max(2e-5, 4 * float(fix[f"{tag}/ref32_err/img"])), e32
    assert 0 < float(fix[f"{tag}/bf16_floor"]) < 2e-2
    if tag == "skip":
        assert _err(S.generator(sd, cfg, z, c, "none"), fix["skip/img_none"]) <= 1e-12
        assert _err(fix["skip/img_none"], fix["skip/img"]) > 1e-3, "the noise does not reach the image"
        assert _err(S.generator(sd, cfg, z, c, "const", psi=0.7, cutoff=2), fix["skip/img_trunc"]) <= 1e-12
        _, dz, dp = S.generator_grads(sd, cfg, z, c, fix["skip/gy"].double())
        assert _err(dz, fix["skip/dz"]) <= 1e-12
        for k, g in dp.items():
            assert float((g - fix[f"skip/dp/{k}"]).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max())), k


def test_restatement_up2_is_modconv_refs(fix):
    """stylegan2_ref.modconv_up2 (which can round the stored core) is modconv_ref's up = 2 route when nothing is rounded"""
    x, w, s, nz, bias, gy = S.tail_inputs("edge", "sample")
    a = S.modconv_up2(x, w, s, R.low_pass().double()) + nz
    b = R.modconv_ref(x, w, s, nz, up=2, flip_weight=False, f=R.low_pass().double())
    assert _err(a, b) <= 1e-13


@pytest.mark.parametrize("tag", list(S.CASES))
def test_state_dict_keys_and_order_are_the_references(fix, tag):
    G = _gen(tag)
    assert list(G.state_dict()) == [str(k) for k in fix[f"{tag}/keys"]]
    G.load_state_dict(_sd(fix, tag, torch.float32), strict=True)
    for k, v in G.state_dict().items():
        assert torch.equal(v, fix[f"{tag}/sd/{k}"].float()), k
    # the low-precision construction has the same keys
    assert list(_gen(tag, **S.LOWP).state_dict()) == list(G.state_dict())


def test_constructor_and_forward_argument_lists():
    from studiogan_amd.backbones import stylegan2 as SG
    names = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert names(SG.Generator.__init__) == ["self", "z_dim", "c_dim", "w_dim", "img_resolution", "img_channels", "MODEL", "mapping_kwargs", "synthesis_kwargs"]
    assert names(SG.Generator.forward)[:7] == ["self", "z", "c", "eval", "truncation_psi", "truncation_cutoff", "update_emas"]
    assert names(SG.MappingNetwork.forward) == ["self", "z", "c", "truncation_psi", "truncation_cutoff", "update_emas"]
    assert names(SG.MappingNetwork.__init__)[:6] == ["self", "z_dim", "c_dim", "w_dim", "num_ws", "num_layers"]
    assert names(SG.SynthesisNetwork.__init__)[:7] == ["self", "w_dim", "img_resolution", "img_channels", "channel_base", "channel_max", "num_fp16_res"]
    assert names(SG.SynthesisBlock.forward)[:7] == ["self", "x", "img", "ws", "force_fp32", "fused_modconv", "update_emas"]
    assert names(SG.Conv2dLayer.__init__)[:4] == ["self", "in_channels", "out_channels", "kernel_size"]


def test_num_ws_and_block_rows():
    for tag, rows in (("skip", [(0, 2), (1, 3), (3, 3)]), ("resnet", [(0, 1), (1, 2), (3, 3)]), ("orig", [(0, 1), (1, 2), (3, 3)])):
        G = _gen(tag)
        assert G.num_ws == G.synthesis.num_ws == G.mapping.num_ws == S.num_ws(S.CASES[tag]) == 6
        assert G.synthesis.block_rows() == rows, tag
        layers = G.synthesis.style_layers()
        assert [r for r, _, _ in layers] == ([0, 1, 1, 2, 3, 3, 4, 5] if tag == "skip" else [0, 1, 2, 3, 4, 5]), tag
        assert [b.use_fp16 for b in _gen(tag, **S.LOWP).synthesis.blocks()] == [False, True, True]
    G = _gen("skip")
    assert [G.synthesis.b4.conv1.weight.shape[0], G.synthesis.b8.conv1.weight.shape[0], G.synthesis.b16.conv1.weight.shape[0]] == [24, 24, 12]


def test_infogan_codes_widen_z():
    import types
    from studiogan_amd.backbones import stylegan2 as SG
    kw = S.kwargs_of(S.CASES["orig"])
    kw["MODEL"] = types.SimpleNamespace(info_type="both", info_num_discrete_c=2, info_dim_discrete_c=5, info_num_conti_c=3)
    G = SG.Generator(**kw)
    assert G.z_dim == G.mapping.z_dim == 24 + 10 + 3 and G.mapping.fc0.weight.shape[1] == 37 + 40


def test_truncation_and_w_avg_update(fix):
    G = _gen("skip")
    G.load_state_dict(_sd(fix, "skip", torch.float32), strict=True)
    M = G.mapping.double()
    w = fix["skip/w"]
    ws = M.broadcast_truncate(w, 0.7, 2)
    assert tuple(ws.shape) == (S.BATCH, 6, 40) and _err(ws, fix["skip/ws_trunc"]) <= 1e-14
    assert torch.equal(ws[:, 2:], w.unsqueeze(1).expand(-1, 4, -1)) and not torch.equal(ws[:, 0], w)
    full = M.broadcast_truncate(w, 0.7)
    assert _err(full[:, 5], fix["skip/ws_trunc"][:, 0]) <= 1e-14
    before = M.w_avg.clone()
    assert torch.equal(M.broadcast_truncate(w), w.unsqueeze(1).expand(-1, 6, -1)) and torch.equal(M.w_avg, before)
    M.broadcast_truncate(w, update_emas=True)
    assert _err(M.w_avg, fix["skip/w_avg_after"]) <= 1e-14 and not torch.equal(M.w_avg, before)


def test_refusals():
    from studiogan_amd.backbones import stylegan2 as SG
    from studiogan_amd.style_ops.fir_bias_act import fir_bias_act
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d_act
    with pytest.raises(NotImplementedError, match="discriminator"):
        SG.Conv2dLayer(8, 8, 3, down=2)
    x16 = torch.zeros(1, 4, 4, 4, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="float16"):
        modulated_conv2d_act(x16, torch.zeros(4, 4, 3, 3), torch.ones(1, 4), up=2, padding=1, resample_filter=R.low_pass())
    with pytest.raises(NotImplementedError, match="float16"):
        fir_bias_act(x16, R.low_pass(), [1, 1, 1, 1])
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(NotImplementedError, match="fused tail"):
        modulated_conv2d_act(x, torch.zeros(4, 4, 3, 3), torch.ones(1, 4), up=2, padding=1, resample_filter=R.low_pass(), act="tanh")
    with pytest.raises(NotImplementedError, match="taps"):
        fir_bias_act(x, torch.ones(5, 5), [2, 2, 2, 2])
    with pytest.raises(RuntimeError, match="GPU"):      # no CPU fallback on the product path
        fir_bias_act(x, R.low_pass(), [1, 1, 1, 1])
    with pytest.raises(AssertionError, match="architecture"):
        SG.SynthesisBlock(8, 8, 16, 8, 3, False, architecture="unet")


def test_grouped_affine_item_table(fix):
    from studiogan_amd import _lib as L
    from studiogan_amd.backbones import stylegan2 as SG
    G = _gen("skip")
    layers = G.synthesis.style_layers()
    N, n_ws, w_dim = 5, 6, 40
    ws = torch.zeros(N, n_ws, w_dim)
    widths = [fc.weight.shape[0] for _, fc, _ in layers]
    out = torch.zeros(N * sum(widths))
    arr = SG.style_affine_items(ws, layers, out)
    assert ctypes.sizeof(L.LinearItemScaled) == 64 and len(arr) == len(layers) == 8
    off = 0
    for it, (row, fc, oscale), Cn in zip(arr, layers, widths):
        assert it.w == fc.weight.data_ptr() and it.bias == fc.bias.data_ptr()
        assert it.y == ws.data_ptr() + 4 * row * w_dim and it.ldy == n_ws * w_dim       # its row of ws, in place
        assert it.out == out.data_ptr() + 4 * off and it.ldo == Cn and it.rows == Cn and it.K == w_dim
        assert it.wscale == pytest.approx(1 / w_dim ** 0.5) and it.bscale == 1.0 and it.oscale == pytest.approx(oscale)
        off += N * Cn
    # toRGB layers carry their fan-in gain, the convolutions none
    assert [s for _, _, s in layers] == [1.0, pytest.approx(24 ** -0.5), 1.0, 1.0, pytest.approx(24 ** -0.5), 1.0, 1.0, pytest.approx(12 ** -0.5)]
    with pytest.raises(AssertionError):
        SG.style_affine_items(ws, layers, out[:-1])


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/configs"), reason="the reference checkout is only present in the authoring container")
def test_generator_args_of_every_stylegan2_config():
    import yaml
    from studiogan_amd import config_map
    from studiogan_amd.backbones import stylegan2 as SG
    ctor = set(inspect.signature(SG.Generator.__init__).parameters)
    syn = set(inspect.signature(SG.SynthesisNetwork.__init__).parameters) | set(inspect.signature(SG.SynthesisBlock.__init__).parameters)
    seen, base = 0, {}
    for f in sorted(glob.glob("/root/reference/src/configs/*/*.yaml")):
        y = yaml.safe_load(open(f))
        if (y.get("MODEL") or {}).get("backbone") != "stylegan2":
            continue
        seen += 1
        for mixed in (False, True):
            kw = config_map.stylegan2_generator_args(y, mixed_precision=mixed)
            assert not (set(kw) - ctor), f
            assert not (set(kw["synthesis_kwargs"]) - syn), f
            assert set(kw["mapping_kwargs"]) == {"num_layers"} and kw["mapping_kwargs"]["num_layers"] == y["STYLEGAN"]["mapping_network"]
            assert kw["c_dim"] == (y["DATA"]["num_classes"] if y["MODEL"].get("g_cond_mtd") == "cAdaIN" else 0), f
            assert (kw["synthesis_kwargs"]["num_fp16_res"], kw["synthesis_kwargs"]["conv_clamp"]) == ((4, 256) if mixed else (0, None))
            assert kw["synthesis_kwargs"]["channel_max"] == 512 and kw["MODEL"].info_type == y["MODEL"].get("info_type", "N/A")
            assert kw["z_dim"] == y["MODEL"]["z_dim"] and kw["w_dim"] == y["MODEL"]["w_dim"] and kw["img_resolution"] == y["DATA"]["img_size"]
        base[(y["DATA"]["name"], y["DATA"]["img_size"])] = kw["synthesis_kwargs"]["channel_base"]
        with pytest.raises(NotImplementedError):
            config_map.model_args(y)
    assert seen == 43
    # 32768 for CIFAR and from 512 pixels up, 16384 between
    assert base[("CIFAR10", 32)] == 32768 and base[("AFHQv2", 256)] == 16384 and base[("AFHQv2", 512)] == 32768 and base[("FFHQ", 1024)] == 32768
    assert base[("ImageNet", 128)] == 16384 and base[("CIFAR100", 32)] == 32768
    with pytest.raises(NotImplementedError):
        config_map.stylegan2_generator_args({"MODEL": {"backbone": "big_resnet"}})


# ---- the layer tail through the interpreter (tests/hipemu): the store-side epilogue of the kernel whose load side test_stylegan2_dis_cpu.py runs ---------------
emulated = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
FIR_SHAPES = {"vec": (3, 12, 9, 9), "scalar": (2, 13, 10, 6)}       # (N, C, H, W): whole fp32 vectors (the scalar path in bf16) / the scalar path; odd extents
FIR_CASES = {"sample-clamp": ("sample", "clamp"), "plane-noclamp": ("plane", "noclamp"), "plain": (None, "plain")}     # (noise, epilogue of D.HEAD_EPI)
FIR_PAD, FIR_GAIN, FIR_MARGIN = (1, 1, 1, 1), 4.0, 1e-2


def _fir_misses(pre, e):
    """where the fp64 pre-activation sits on the leaky ReLU's kink, or its unclamped output within FIR_MARGIN (relative) of the clamp"""
    miss = pre == 0
    if e["clamp_"] is not None:
        miss = miss | (((D.bias_act(pre, None, e["act"], e["gain"]).abs() - e["clamp_"]).abs()) <= FIR_MARGIN * e["clamp_"])
    return miss


def _fir_inputs(shape, noise, epi):
    """x, noise and gy on the 2^-6 grid, bias on the grid + 2^-7, drawn as stylegan2_dis_ref.head_inputs draws them from one fixed seed. A draw alone does not
    clear the margins the test asserts: of the 2304 outputs of the `vec` shape about nine land within 1e-2 of the clamp, and none of 6000 seeds had none. So
    where the fp64 reference misses a margin, that noise value moves by the next multiple of 1/16 (still on the grid) under which every output it feeds holds."""
    N, C, H, W = FIR_SHAPES[shape]
    g = torch.Generator().manual_seed(5200)
    q = lambda *s, scale=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale * 64).round().clamp(-192, 192) / 64      # noqa: E731
    x = q(N, C, H, W)
    bias = q(C, scale=0.5).clamp(-126 / 64, 126 / 64) + 2.0 ** -7
    Ho, Wo = D.out_hw(H, W, FIR_PAD, 1)
    gy = q(N, C, Ho, Wo)
    if noise is None:
        return x, bias, None, gy
    nz0 = q(N, 1, Ho, Wo) if noise == "sample" else q(Ho, Wo)
    core = D.fir(x, R.low_pass().double(), FIR_PAD, gain=FIR_GAIN) + bias.reshape(1, -1, 1, 1)
    over = (1,) if noise == "sample" else (0, 1)        # the outputs one noise value feeds
    nz = nz0
    for k in (1, -1, 2, -2, 3, -3):
        miss = _fir_misses(core + nz, D.HEAD_EPI[epi]).any(dim=over, keepdim=noise == "sample")
        nz = torch.where(miss, nz0 + k / 16, nz)
    return x, bias, nz, gy


@emulated
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(FIR_CASES))
@pytest.mark.parametrize("shape", list(FIR_SHAPES))
def test_fir_bias_act_through_the_interpreter(shape, case, dtype):
    """fir_bias_act (forward, dx, dnoise through sg_modconv_reduce, dbias) on the kernel sources against fp64 clamp(gain * lrelu(fir(x) + noise + bias)), at the
    tolerances of the head's interpreter test; the plain mode IS upfirdn2d on the NCHW copy, forward and adjoint, bit for bit"""
    import fullemu
    from studiogan_amd.style_ops.fir_bias_act import fir_bias_act
    from studiogan_amd.style_ops.upfirdn2d import upfirdn2d
    noise, epi = FIR_CASES[case]
    e = D.HEAD_EPI[epi]
    f = R.low_pass()
    tol = 2e-5 if dtype == torch.float32 else 1e-2
    x, bias, nz, gy = _fir_inputs(shape, noise, epi)
    leaves = {k: v.clone().requires_grad_(True) for k, v in (("x", x), ("noise", nz), ("bias", bias if e["bias"] else None)) if v is not None}
    pre = D.fir(leaves["x"], f.double(), FIR_PAD, gain=FIR_GAIN)
    if "noise" in leaves:
        pre = pre + leaves["noise"]
    if "bias" in leaves:
        pre = pre + leaves["bias"].reshape(1, -1, 1, 1)
    if e["act"] == "lrelu":     # the two margins, on every element of the reference
        assert float(pre.detach().abs().min()) > 0
    if e["clamp_"] is not None:
        a = D.bias_act(pre.detach(), None, e["act"], e["gain"]).abs()
        assert float(((a - e["clamp_"]).abs() / e["clamp_"]).min()) > FIR_MARGIN and bool((a > e["clamp_"]).any()), "too near the clamp, or it does not bite"
    y64 = D.bias_act(pre, None, e["act"], e["gain"], e["clamp_"])
    g64 = dict(zip(leaves, torch.autograd.grad(y64, list(leaves.values()), gy)))
    with fullemu.Installed() as E:
        dev = {k: (v.to(dtype).contiguous(memory_format=torch.channels_last) if k == "x" else v.float()).detach().requires_grad_(True) for k, v in leaves.items()}
        xd = dev["x"]
        n0, h0 = E.lib.sg_fir_bias_act_launches(), E.lib.sg_act_fir_launches()
        y = fir_bias_act(xd, f, list(FIR_PAD), noise=dev.get("noise"), bias=dev.get("bias"), act=e["act"], gain=e["gain"], clamp=e["clamp_"], filter_gain=FIR_GAIN)
        y.backward(gy.to(dtype))
        assert E.lib.sg_fir_bias_act_launches() - n0 == 2 and E.lib.sg_act_fir_launches() == h0       # forward + data gradient, the tail's entry
        assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last) and tuple(y.shape) == tuple(y64.shape)
        assert _err(y.detach(), y64.detach()) <= tol, (shape, case)
        for k, v in dev.items():
            assert tuple(v.grad.shape) == tuple(g64[k].shape) and _err(v.grad, g64[k]) <= tol, (shape, case, k)
        if epi == "plain":
            xn = x.to(dtype).requires_grad_(True)
            yu = upfirdn2d(xn, f, padding=list(FIR_PAD), gain=FIR_GAIN)
            yu.backward(gy.to(dtype))
            assert torch.equal(yu, y.detach().contiguous()) and torch.equal(xn.grad, xd.grad.contiguous())
