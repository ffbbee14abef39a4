"""Host-side checks of the StyleGAN2 discriminator (backbones/stylegan2_dis.py): the fixture tests/golden/stylegan2_dis.npz against the restatement that wrote its
expectation, the state_dict contract with the reference, the argument lists, the refusals, config_map.stylegan2_discriminator_args over the reference's
configuration files, and the two new kernels (sg_act_fir_nhwc, sg_mbstd_*) with their autograd functions through the kernel-source interpreter. No GPU."""
import glob
import inspect
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import emu  # noqa: E402
import modconv_ref as R  # noqa: E402
import stylegan2_dis_ref as D  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fi" else v) for k, v in D.load_golden().items()}


def _sd(fix, tag, dtype=torch.float64):
    """the case's state: its own keys, the `orig` case's backbone under a heads-only case"""
    out = {}
    for k in (str(k) for k in fix[f"{tag}/keys"]):
        src = f"{tag}/sd/{k}" if f"{tag}/sd/{k}" in fix else f"orig/sd/{k}"
        out[k] = fix[src].to(dtype)
    return out


def _dis(tag, **extra):
    from studiogan_amd.backbones import stylegan2_dis as SD
    return SD.Discriminator(**D.kwargs_of(D.CASES[tag], **extra))


def _err(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


@pytest.mark.parametrize("tag", list(D.CASES))
def test_restatement_reproduces_the_fixture(fix, tag):
    cfg, sd = D.CASES[tag], _sd(fix, tag)
    img, label = fix[f"{tag}/img"].double(), fix[f"{tag}/label"]
    gys = {k[len(tag) + 3:]: v.double() for k, v in fix.items() if k.startswith(f"{tag}/g_")}
    pkeys = [k[len(tag) + 4:] for k in fix if k.startswith(f"{tag}/dp/")]
    out, dimg, dp = D.discriminator_grads(sd, cfg, img, label, gys, pkeys)
    assert list(out) == list(D.OUT_KEYS)
    stored = {k[len(tag) + 5:] for k in fix if k.startswith(f"{tag}/out/")}
    assert stored == set(D.float_outputs(out)) == set(gys)
    for k in stored:
        assert _err(out[k], fix[f"{tag}/out/{k}"]) <= 1e-12, k
    assert _err(dimg, fix[f"{tag}/dimg"]) <= 1e-12
    for k in pkeys:     # (stored as float32)
        assert float((dp[k] - fix[f"{tag}/dp/{k}"]).abs().max()) <= 2e-7 * max(1.0, float(dp[k].abs().max())), k
    lowp = D.float_outputs(D.discriminator(sd, cfg, img, label, **D.LOWP))
    for k, v in lowp.items():
        assert _err(v, fix[f"{tag}/lowp/{k}"]) <= 1e-12, k
    # the fp32 evaluation of the same statement sits where the reference's own fp32 evaluation does
    o32 = D.discriminator(_sd(fix, tag, torch.float32), cfg, img.float(), label)
    for k in stored:
        assert _err(o32[k], fix[f"{tag}/out/{k}"]) <= max(2e-5, 4 * float(fix[f"{tag}/ref32_err/{k}"])), k
    assert 0 < float(fix[f"{tag}/bf16_floor"]) < 2e-2
    if tag == "ac_adc":
        fake = D.discriminator(sd, cfg, img, label, adc_fake=True)
        assert torch.equal(fake["label"], fix[f"{tag}/out_fake/label"]) and _err(fake["cls_output"], fix[f"{tag}/out_fake/cls_output"]) <= 1e-12
    if tag == "skip":       # Freeze-D: the first two layers have no gradient in the fixture
        assert not any(k.startswith(("b16.fromrgb", "b16.conv0")) for k in pkeys) and "b16.conv1.weight" in pkeys


@pytest.mark.parametrize("tag", list(D.CASES))
def test_state_dict_keys_and_order_are_the_references(fix, tag):
    Dn = _dis(tag)
    assert list(Dn.state_dict()) == [str(k) for k in fix[f"{tag}/keys"]]
    Dn.load_state_dict(_sd(fix, tag, torch.float32), strict=True)
    for k, v in Dn.state_dict().items():
        assert torch.equal(v, _sd(fix, tag, torch.float32)[k]), k
    # the low-precision and the layer-by-layer constructions have the same keys
    assert list(_dis(tag, **D.LOWP).state_dict()) == list(Dn.state_dict()) == list(_dis(tag, fused_down=False).state_dict())
    params = {k for k, _ in Dn.named_parameters()}
    if tag == "skip":       # freeze_layers = 2: fromrgb and conv0 of the first block are buffers
        assert not any(k.startswith(("b16.fromrgb", "b16.conv0")) for k in params) and "b16.conv1.weight" in params
        assert {"b16.fromrgb.weight", "b16.fromrgb.bias", "b16.conv0.weight", "b16.conv0.bias"} <= {k for k, _ in Dn.named_buffers()}
    else:
        assert {"b16.fromrgb.weight", "b16.conv0.bias"} <= params


def test_constructor_and_forward_argument_lists():
    """the reference's lists (src/models/stylegan2.py:134-187, 551-924), in order; this package's own switches come behind them"""
    from studiogan_amd.backbones import stylegan2_dis as SD
    names = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert names(SD.Discriminator.__init__) == ["self", "c_dim", "img_resolution", "img_channels", "architecture", "channel_base", "channel_max", "num_fp16_res",
                                                "conv_clamp", "cmap_dim", "d_cond_mtd", "aux_cls_type", "d_embed_dim", "num_classes", "normalize_d_embed",
                                                "block_kwargs", "mapping_kwargs", "epilogue_kwargs", "MODEL"]
    assert names(SD.Discriminator.forward) == ["self", "img", "label", "eval", "adc_fake", "update_emas", "block_kwargs"]
    assert names(SD.DiscriminatorBlock.__init__)[:14] == ["self", "in_channels", "tmp_channels", "out_channels", "resolution", "img_channels", "first_layer_idx",
                                                          "architecture", "activation", "resample_filter", "conv_clamp", "use_fp16", "fp16_channels_last",
                                                          "freeze_layers"]
    assert names(SD.DiscriminatorBlock.__init__)[14:] == ["fused_down"]
    assert names(SD.DiscriminatorBlock.forward) == ["self", "x", "img", "force_fp32"]
    assert names(SD.DiscriminatorEpilogue.__init__) == ["self", "in_channels", "cmap_dim", "resolution", "img_channels", "architecture", "mbstd_group_size",
                                                        "mbstd_num_channels", "activation", "conv_clamp"]
    assert names(SD.DiscriminatorEpilogue.forward) == ["self", "x", "img", "force_fp32"]
    assert names(SD.MinibatchStdLayer.__init__) == ["self", "group_size", "num_channels"] and names(SD.MinibatchStdLayer.forward) == ["self", "x"]
    assert names(SD.DConv2dLayer.__init__) == ["self", "in_channels", "out_channels", "kernel_size", "bias", "activation", "up", "down", "resample_filter",
                                               "conv_clamp", "channels_last", "trainable"]
    assert names(SD.DConv2dLayer.forward)[:3] == ["self", "x", "gain"]
    sig = inspect.signature(SD.Discriminator.__init__).parameters
    assert (sig["architecture"].default, sig["channel_base"].default, sig["channel_max"].default, sig["num_fp16_res"].default) == ("resnet", 32768, 512, 0)
    assert inspect.signature(SD.DiscriminatorEpilogue.__init__).parameters["mbstd_group_size"].default == 4
    assert inspect.signature(SD.DiscriminatorBlock.__init__).parameters["fused_down"].default is True


def test_refusals():
    from studiogan_amd.backbones import stylegan2 as SG
    from studiogan_amd.backbones import stylegan2_dis as SD
    from studiogan_amd.style_ops.act_fir import act_fir
    from studiogan_amd.style_ops.conv2d_resample import conv2d_plain, conv2d_resample
    from studiogan_amd.style_ops.minibatch_std import minibatch_std
    x16 = torch.zeros(1, 4, 4, 4, dtype=torch.float16)
    x = torch.zeros(4, 6, 4, 4)
    for op in (lambda t: act_fir(t, R.low_pass(), [1, 1, 1, 1]), lambda t: minibatch_std(t, 1), lambda t: conv2d_plain(t, torch.zeros(4, 4, 3, 3))):
        with pytest.raises(NotImplementedError, match="float16"):
            op(x16)
    with pytest.raises(NotImplementedError, match="taps"):
        act_fir(x, torch.ones(5, 5), [2, 2, 2, 2])
    with pytest.raises(NotImplementedError, match="act="):
        act_fir(x, R.low_pass(), [2, 2, 2, 2], act="tanh")
    with pytest.raises(NotImplementedError, match="down="):
        act_fir(x, R.low_pass(), [2, 2, 2, 2], down=3)
    with pytest.raises(RuntimeError, match="GPU"):      # no CPU fallback on the product path
        act_fir(x, R.low_pass(), [1, 1, 1, 1])
    with pytest.raises(RuntimeError, match="GPU"):
        minibatch_std(x, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        conv2d_plain(x, torch.zeros(4, 6, 3, 3))
    with pytest.raises(AssertionError, match="divide the batch"):        # N % G
        minibatch_std(torch.zeros(6, 4, 4, 4), 4)
    with pytest.raises(AssertionError, match="divide the channels"):     # C % F
        minibatch_std(x, 2, 4)
    with pytest.raises(NotImplementedError, match="stride"):
        conv2d_plain(x, torch.zeros(4, 6, 1, 1), stride=2)
    with pytest.raises(NotImplementedError, match="up = 1"):
        conv2d_resample(x, torch.zeros(4, 6, 3, 3), up=2, padding=1)
    with pytest.raises(NotImplementedError, match="PD"):
        SD.Discriminator(**dict(D.kwargs_of(D.CASES["resnet"]), d_cond_mtd="PD"))
    with pytest.raises(NotImplementedError, match="generator"):
        SD.DConv2dLayer(8, 8, 3, up=2)
    with pytest.raises(AssertionError, match="architecture"):
        SD.DiscriminatorBlock(8, 8, 8, 8, 3, 0, architecture="unet")
    with pytest.raises(NotImplementedError, match="discriminator"):      # the generator's layer keeps its refusal
        SG.Conv2dLayer(8, 8, 3, down=2)


def test_convolution_entry_dispatch():
    """sg_conv2d_fwd where the input channels fill 16-byte vectors, sg_modconv2d_fwd with NULL tables otherwise; FORCE pins one; record() sees the launches"""
    from studiogan_amd.style_ops import conv2d_resample as CR
    assert CR.ENTRIES == ("sg_conv2d_fwd", "sg_modconv2d_fwd")
    for C, dt, want in ((512, torch.bfloat16, 0), (512, torch.float32, 0), (12, torch.float32, 0), (12, torch.bfloat16, 1), (3, torch.float32, 1), (513, torch.float32, 1),
                        (513, torch.bfloat16, 1), (24, torch.bfloat16, 0)):
        assert CR.entry_for(C, dt) == CR.ENTRIES[want], (C, dt)
    CR.FORCE = CR.ENTRIES[1]
    try:
        assert CR.entry_for(512, torch.bfloat16) == CR.ENTRIES[1]
    finally:
        CR.FORCE = None
    with CR.record() as log:
        assert log == [] and CR._log is log
    assert CR._log is None


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/configs"), reason="the reference checkout is only present in the authoring container")
def test_discriminator_args_of_every_stylegan2_config():
    import yaml
    from studiogan_amd import config_map
    from studiogan_amd.backbones import stylegan2_dis as SD
    ctor = list(inspect.signature(SD.Discriminator.__init__).parameters)[1:]
    seen, base = 0, {}
    for f in sorted(glob.glob("/root/reference/src/configs/*/*.yaml")):
        y = yaml.safe_load(open(f))
        if (y.get("MODEL") or {}).get("backbone") != "stylegan2":
            continue
        seen += 1
        for mixed in (False, True):
            kw = config_map.stylegan2_discriminator_args(y, mixed_precision=mixed)
            assert sorted(kw) == sorted(ctor), f
            cond = y["MODEL"].get("d_cond_mtd", "W/O")
            assert kw["c_dim"] == (y["DATA"]["num_classes"] if cond in ("PD", "SPD", "2C", "D2DCE") else 0), f
            assert (kw["num_fp16_res"], kw["conv_clamp"]) == ((4, 256) if mixed else (0, None))
            assert kw["architecture"] == y["STYLEGAN"]["d_architecture"] and kw["channel_max"] == 512 and kw["cmap_dim"] is None
            assert kw["epilogue_kwargs"] == {"mbstd_group_size": y["STYLEGAN"]["d_epilogue_mbstd_group_size"]}
            assert kw["block_kwargs"] == {} and kw["mapping_kwargs"] == {}
            assert kw["img_resolution"] == y["DATA"]["img_size"] and kw["num_classes"] == y["DATA"]["num_classes"] and kw["d_cond_mtd"] == cond
            assert kw["aux_cls_type"] == y["MODEL"].get("aux_cls_type", "W/O") and kw["MODEL"].info_type == y["MODEL"].get("info_type", "N/A")
            assert kw["channel_base"] == config_map.stylegan2_generator_args(y)["synthesis_kwargs"]["channel_base"]
        base[(y["DATA"]["name"], y["DATA"]["img_size"])] = kw["channel_base"]
        with pytest.raises(NotImplementedError):
            config_map.model_args(y)
    assert seen == 43
    assert base[("CIFAR10", 32)] == 32768 and base[("AFHQv2", 256)] == 16384 and base[("AFHQv2", 512)] == 32768
    with pytest.raises(NotImplementedError):
        config_map.stylegan2_discriminator_args({"MODEL": {"backbone": "big_resnet"}})
    with pytest.raises(NotImplementedError, match="d_architecture"):
        config_map.stylegan2_discriminator_args({"MODEL": {"backbone": "stylegan2"}, "STYLEGAN": {}})


# ---- the kernels through the interpreter (tests/hipemu): the smallest shapes of the GPU test, against fp64 --------------------------------------------------
emulated = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")


@pytest.fixture()
def _one_torch_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@emulated
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("down", [1, 2])
def test_act_fir_through_the_interpreter(_one_torch_thread, down, dtype):
    import fullemu
    from studiogan_amd.style_ops.act_fir import act_fir
    from studiogan_amd.style_ops.upfirdn2d import upfirdn2d
    f = R.low_pass()
    tol = 2e-5 if dtype == torch.float32 else 1e-2
    with fullemu.Installed() as E:
        for shape, pad, epi in (("edge", "p2", "clamp"), ("edge", "p1", "noclamp"), ("odd", "asym", "clamp"), ("odd", "p2", "plain")):
            x, b, gy = D.head_inputs(shape, pad, down)
            e = D.HEAD_EPI[epi]
            y64, dx64, db64 = D.head_ref(x, b, gy, pad, down, epi)
            xd = x.to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            bd = b.float().requires_grad_(True) if e["bias"] else None
            n0 = E.lib.sg_act_fir_launches()
            y = act_fir(xd, f, list(D.HEAD_PADS[pad]), down=down, bias=bd, act=e["act"], gain=e["gain"], clamp=e["clamp_"])
            y.backward(gy.to(dtype))
            assert E.lib.sg_act_fir_launches() - n0 == 2        # forward + data gradient
            assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last) and tuple(y.shape) == tuple(y64.shape)
            assert _err(y, y64) <= tol and _err(xd.grad, dx64) <= tol, (shape, pad, epi)
            if bd is not None:
                assert _err(bd.grad, db64) <= tol, (shape, pad, epi)
            if epi == "plain":      # the plain mode IS upfirdn2d on the NCHW copy, forward and adjoint, bit for bit
                xn = x.to(dtype).requires_grad_(True)
                yu = upfirdn2d(xn, f, down=down, padding=list(D.HEAD_PADS[pad]))
                yu.backward(gy.to(dtype))
                assert torch.equal(yu, y.contiguous()) and torch.equal(xn.grad, xd.grad.contiguous())
        # second order is refused, not silently cut
        xd = x.to(dtype).requires_grad_(True)
        y = act_fir(xd, f, [1, 1, 1, 1], down=down)
        with pytest.raises(NotImplementedError, match="create_graph"):
            torch.autograd.grad(y.sum(), xd, create_graph=True)


@emulated
def test_act_fir_border_is_zero_not_act_of_bias(_one_torch_thread):
    import fullemu
    from studiogan_amd.style_ops.act_fir import act_fir
    x, _, _ = D.head_inputs("edge", "p2", 1)
    bias = torch.full((x.shape[1],), 1.5 + 2.0 ** -7, dtype=torch.float64)      # act(bias) = 2.1: leaking into the padding it would move the border rows by O(1)
    want = D.act_fir(x, R.low_pass().double(), (2, 2, 2, 2), 1, bias, "lrelu", D.SQRT2, None)
    leak = D.fir(D.bias_act(torch.nn.functional.pad(x, [2, 2, 2, 2]), bias, "lrelu", D.SQRT2), R.low_pass().double(), (0, 0, 0, 0))
    assert _err(leak, want) > 0.1
    with fullemu.Installed():
        y = act_fir(x.float().contiguous(memory_format=torch.channels_last), R.low_pass(), [2, 2, 2, 2], bias=bias.float(), act="lrelu")
    assert _err(y, want) <= 2e-5


@emulated
@pytest.mark.parametrize("case", list(D.MBSTD_CASES))
def test_minibatch_std_through_the_interpreter(_one_torch_thread, case):
    import fullemu
    from studiogan_amd.style_ops.minibatch_std import minibatch_std
    N, C, H, W, group, nch = D.MBSTD_CASES[case]
    with fullemu.Installed() as E:
        assert (E.lib.sg_mbstd_splits(N, H, W, C, N if group is None else min(group, N), nch) > 1) == (case == "split"), "the chunked path is the `split` case's"
        for constant in ((False, True) if case in ("g4f2", "g2f1") else (False,)):
            x, gy = D.mbstd_inputs(case, constant)
            o64, dx64 = D.mbstd_ref(x, gy, group, nch)
            xd = x.float().contiguous(memory_format=torch.channels_last).requires_grad_(True)
            n0 = E.lib.sg_mbstd_launches()
            out = minibatch_std(xd, group, nch)
            out.backward(gy.float())
            assert E.lib.sg_mbstd_launches() - n0 == 2
            assert tuple(out.shape) == (N, C + nch, H, W) and out.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(out[:, :C], xd.detach())
            assert _err(out, o64) <= 2e-5 and _err(xd.grad, dx64) <= 2e-5, (case, constant)
            if constant:        # zero variance: s = sqrt(1e-8), no gradient through the statistic, nothing divides by zero
                assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(xd.grad).all())
                assert float((out.detach()[:, C:] - 1e-4).abs().max()) <= 1e-10 and torch.equal(xd.grad, gy.float()[:, :C])
