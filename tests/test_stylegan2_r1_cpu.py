"""Host-side checks of R1 through the StyleGAN2 discriminator: the second-order passes of style_ops.act_fir (sg_act_fir_nhwc_gate), style_ops.minibatch_std
(sg_mbstd_bwd2) and style_ops.conv2d_plain through the kernel-source interpreter against fp64 autograd, the style_ops.second_order() context, the launches
the image-gradient pass does NOT make, config_map.stylegan2_r1_args over the reference's configuration files, and the fixture tests/golden/stylegan2_r1.npz
against the restatement that wrote it. No GPU.

Bounds: the kernels' existing ones (tests/test_stylegan2_dis_cpu.py): 2e-5 of the expected tensor's range in fp32, 1e-2 in bf16 (inputs on grids bf16 holds)."""
import glob
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import emu  # noqa: E402
import stylegan2_dis_ref as D  # noqa: E402
import stylegan2_r1_checks as K  # noqa: E402

emulated = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
DTYPES = [torch.float32, torch.bfloat16]
_name = K.dtype_name


@pytest.fixture()
def _one_torch_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@emulated
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("down", [1, 2])
def test_act_fir_second_order_through_the_interpreter(_one_torch_thread, down, dtype):
    import fullemu
    with fullemu.Installed() as E:
        for shape in ("edge", "odd"):
            K.check_head_second_order(E.lib, "cpu", shape, down, dtype)


@emulated
def test_act_fir_gate_is_zero_outside_the_image(_one_torch_thread):
    import fullemu
    with fullemu.Installed():
        for down in (1, 2):
            K.check_gate_border("cpu", down)


@emulated
@pytest.mark.parametrize("case", list(K.MBSTD_R1_CASES))
def test_minibatch_std_second_order_through_the_interpreter(_one_torch_thread, case):
    import fullemu
    with fullemu.Installed() as E:
        K.check_mbstd_second_order(E.lib, "cpu", case)


@emulated
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", K.CONV_GEOMS, ids=lambda g: f"k{g[0]}s{g[1]}")
def test_conv2d_plain_second_order_through_the_interpreter(_one_torch_thread, geom, dtype):
    import fullemu
    with fullemu.Installed():
        seen = set()
        for C in K.CONV_CHANNELS:
            seen |= K.check_conv_second_order("cpu", geom, C, dtype)
        from studiogan_amd.style_ops import conv2d_resample as CR
        if dtype == torch.float32:      # 12 fills fp32 vectors (the planned dispatch), 3 and 25 do not (the NULL-table modulated entry)
            assert seen == set(CR.ENTRIES)


@emulated
def test_image_gradient_pass_launches_no_weight_gradient(_one_torch_thread, monkeypatch):
    import fullemu
    with fullemu.Installed() as E:
        K.check_no_weight_gradient_in_the_first_pass(E.lib, "cpu", monkeypatch)


def test_context_restores_the_flag():
    from studiogan_amd import style_ops
    from studiogan_amd.functional import _base as B
    assert B._SECOND_ORDER[0] == 0
    with style_ops.second_order():
        assert B._SECOND_ORDER[0] == 1
        with style_ops.second_order():      # re-entrant
            assert B._SECOND_ORDER[0] == 2
        assert B._SECOND_ORDER[0] == 1
    assert B._SECOND_ORDER[0] == 0
    with pytest.raises(ZeroDivisionError):
        with style_ops.second_order():
            1 / 0
    assert B._SECOND_ORDER[0] == 0
    # what the flag lifts: the three operators of the discriminator, by name, and only while a graph is being recorded
    with torch.no_grad():
        assert B._first_order_only("act_fir") is False
    for name in ("act_fir", "conv2d_resample", "minibatch_std", "modulated_conv2d", "fir_bias_act"):
        with pytest.raises(NotImplementedError, match="create_graph"):
            B._first_order_only(name)
    with style_ops.second_order():
        assert all(B._first_order_only(n) is True for n in ("act_fir", "conv2d_resample", "minibatch_std"))
        for name in ("modulated_conv2d", "fir_bias_act", "ConvTransposeFn", "act_fir (third order)"):
            with pytest.raises(NotImplementedError, match="create_graph"):
                B._first_order_only(name)


@emulated
def test_refusals_outside_the_context_and_third_order(_one_torch_thread):
    import fullemu
    with fullemu.Installed():
        K.check_refusals("cpu")


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/configs"), reason="the reference checkout is only present in the authoring container")
def test_r1_args_of_every_stylegan2_config():
    import yaml
    from studiogan_amd import config_map
    seen, intervals = 0, set()
    for f in sorted(glob.glob("/root/reference/src/configs/*/*.yaml")):
        y = yaml.safe_load(open(f))
        if (y.get("MODEL") or {}).get("backbone") != "stylegan2":
            continue
        seen += 1
        kw = config_map.stylegan2_r1_args(y)
        assert sorted(kw) == ["betas", "d_reg_interval", "lr", "r1_lambda", "r1_place"], f
        Ls, O, S = y["LOSS"], y["OPTIMIZATION"], y["STYLEGAN"]
        assert Ls["apply_r1_reg"] is True, f
        assert (kw["r1_lambda"], kw["r1_place"], kw["d_reg_interval"]) == (Ls["r1_lambda"], Ls["r1_place"], S["d_reg_interval"]), f
        n = S["d_reg_interval"]
        ratio = n / (n + 1) if n != 1 else 1
        assert kw["lr"] == O["d_lr"] * ratio and kw["betas"] == [O["beta1"] ** ratio, O["beta2"] ** ratio], f
        assert kw["r1_place"] in ("inside_loop", "outside_loop")
        intervals.add(n)
        with pytest.raises(NotImplementedError):        # the training loop itself is not registered yet
            config_map.model_args(y)
    assert seen == 43 and 16 in intervals
    cifar = yaml.safe_load(open("/root/reference/src/configs/CIFAR10/StyleGAN2.yaml"))
    kw = config_map.stylegan2_r1_args(cifar)
    assert kw["r1_lambda"] == 0.01 and kw["r1_place"] == "outside_loop" and kw["lr"] == 0.0025 * 16 / 17 and kw["betas"] == [0.0, 0.99 ** (16 / 17)]
    with pytest.raises(NotImplementedError):
        config_map.stylegan2_r1_args({"MODEL": {"backbone": "big_resnet"}})
    with pytest.raises(NotImplementedError, match="apply_r1_reg"):
        config_map.stylegan2_r1_args({"MODEL": {"backbone": "stylegan2"}, "STYLEGAN": {"d_reg_interval": 16}})
    with pytest.raises(NotImplementedError, match="d_reg_interval"):
        config_map.stylegan2_r1_args({"MODEL": {"backbone": "stylegan2"}, "LOSS": {"apply_r1_reg": True, "r1_lambda": 10, "r1_place": "outside_loop"}})


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fix():
    return K.load_fixtures()


@pytest.mark.parametrize("tag", list(D.FULL_CASES))
def test_restatement_reproduces_the_r1_fixture(fix, tag):
    import make_golden_stylegan2_r1 as M
    dis, r1 = fix
    cfg = D.CASES[tag]
    sd = {k: v.double() for k, v in K.state(dis, tag).items()}
    pkeys = K.param_keys(dis, tag)
    assert pkeys == [k[len(tag) + 4:] for k in r1 if k.startswith(f"{tag}/dp/")]
    img, label = r1[f"{tag}/img"].double(), r1[f"{tag}/label"]
    assert torch.equal(label, dis[f"{tag}/label"]) and (int(r1[f"{tag}/image_seed"]) > 0 or torch.equal(r1[f"{tag}/img"], dis[f"{tag}/img"]))
    pen, g, dp = M.r1(sd, cfg, img, label, pkeys)
    assert K.err(pen, r1[f"{tag}/penalty"]) <= 1e-12 and K.err(g, r1[f"{tag}/r1_grads"]) <= 1e-12
    for k in pkeys:     # (stored as float32)
        assert float((dp[k] - r1[f"{tag}/dp/{k}"]).abs().max()) <= 2e-7 * float(dp[k].abs().max()), k
        assert (float(dp[k].abs().max()) > 0) == (f"{tag}/ref32_err/dp/{k}" in r1), k
    # a bias behind the last nonlinearity that depends on it only through a slope has an exactly zero gradient; so has every head the penalty does not read
    assert all(float(r1[f"{tag}/dp/{k}"].abs().max()) == 0 for k in ("b4.fc.bias", "linear1.bias"))
    assert 0 < float(r1[f"{tag}/bf16_floor"]) and all(float(v) <= float(r1[f"{tag}/bf16_floor"]) for k, v in r1.items() if k.startswith(f"{tag}/bf16_floor_of/"))
    # no pre-activation within 4 fp32 errors of a kink (the premise of the fp32 bound), and the bf16 emulation alone inside the cap of differing sides
    sd32 = K.state(dis, tag)
    assert M.kink_margin(sd, sd32, cfg, img, label, pkeys) >= M.MARGIN
    assert M.bf16_sides(sd, cfg, img, label, pkeys, True) <= M.FLIP_CAP

