"""Host-side checks of path-length regularisation through the StyleGAN2 generator: the second-order passes of style_ops.modulated_conv2d (sg_modconv2d_jvp
and the launches around it) and style_ops.fir_bias_act (sg_fir_bias_act_nhwc_gate) through the kernel-source interpreter against fp64 autograd, the
style_ops.second_order(generator=True) context, losses.PathLengthRegularizer / stylegan_g_reg_step / stylegan_generate_images on the three generator
architectures, config_map.stylegan2_pl_args over the reference's configuration files, and the fixture tests/golden/stylegan2_pl.npz against the restatement that
wrote it. No GPU.

Bounds: tests/stylegan2_pl_checks.py."""
import ctypes
import glob
import os
import subprocess
import sys
import tempfile

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import emu  # noqa: E402
import stylegan2_pl_checks as K  # noqa: E402
import stylegan2_ref as S  # noqa: E402

emulated = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
DTYPES = [torch.float32, torch.bfloat16]
_name = K.dtype_name


@pytest.fixture()
def _one_torch_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---- the operators ------------------------------------------------------------------------------------------------------------------------------------------

@emulated
@pytest.mark.parametrize("route", ["fused", "composition"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("tag", K.MODCONV_CASES)
def test_modconv_second_order_through_the_interpreter(_one_torch_thread, tag, dtype, route):
    import fullemu
    with fullemu.Installed() as E:
        K.check_modconv_second_order(E.lib, "cpu", tag, dtype, route=route)


@emulated
def test_tangent_route_follows_the_measured_rule(_one_torch_thread):
    import fullemu
    with fullemu.Installed() as E:
        K.check_tangent_rule(E.lib, "cpu")


@emulated
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_modconv_second_order_with_post_gain(_one_torch_thread, dtype):
    import fullemu
    with fullemu.Installed() as E:
        K.check_modconv_second_order(E.lib, "cpu", "g", dtype, gain=0.75)
        K.check_modconv_second_order(E.lib, "cpu", "d", dtype, gain=1.5)        # (no demodulation: the gain alone is the post-scale table)


@emulated
def test_modconv_refuses_a_cotangent_on_the_weight_gradient(_one_torch_thread):
    import fullemu
    with fullemu.Installed():
        K.check_modconv_refuses_weight_cotangent("cpu")


@emulated
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("epi", list(K.TAIL_EPI))
def test_fir_bias_act_second_order_through_the_interpreter(_one_torch_thread, epi, dtype):
    import fullemu
    with fullemu.Installed() as E:
        for noise in S.TAIL_NOISE:
            K.check_tail_second_order(E.lib, "cpu", "edge", noise, epi, dtype)


def test_jvp_entry_points_exported_and_bound(sg):
    from studiogan_amd import _lib as L
    lib = sg.lib()
    for name in ("sg_modconv2d_jvp", "sg_modconv2d_jvp_ok", "sg_modconv_jvp_launches", "sg_fir_bias_act_nhwc_gate"):
        assert name in L.exported_symbols() and hasattr(lib, name), name
    assert lib.sg_modconv_jvp_launches() >= 0
    # the ctypes mirror has the size the C compiler gives the descriptor, and the embedded forward descriptor sits at its start
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sgamd.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(sg_modconv_jvp_desc), '
           'offsetof(sg_modconv_jvp_desc, vx), sizeof(sg_modconv_desc));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "s")], check=True)
        out = subprocess.run([os.path.join(d, "s")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(L.ModConvJvpDesc), L.ModConvJvpDesc.vx.offset, ctypes.sizeof(L.ModConvDesc)]
    # the family of checks: whatever sg_modconv2d_ok refuses, and a tangent without its tables or operands
    j = L.ModConvJvpDesc()
    c = j.m.conv
    c.dtype, c.N, c.Hs, c.Ws, c.C, c.ldx, c.Cout, c.ldo, c.Ho, c.Wo = L.F32, 2, 8, 8, 8, 8, 8, 8, 8, 8
    c.R = c.S = 3
    c.stride, c.pad_h, c.pad_w, c.alpha, c.beta = 1, 1, 1, 1.0, 1.0
    ok = lambda: lib.sg_modconv2d_jvp_ok(ctypes.byref(j))      # noqa: E731
    assert ok() == 0
    j.m.pre = j.vs = j.vx = 64
    assert ok() == 1
    j.e = 64
    assert ok() == 0        # the demodulation term needs the stored result
    j.y, j.ldy = 64, 8
    assert ok() == 1
    j.ldy = 4
    assert ok() == 0
    j.ldy, c.R = 8, 5
    assert ok() == 0 and lib.sg_modconv2d_ok(ctypes.byref(j.m)) == 0


# ---- the context --------------------------------------------------------------------------------------------------------------------------------------------

def test_generator_context_has_its_own_counter():
    K.check_context_flags()


@emulated
def test_refusals_outside_the_generator_context_and_third_order(_one_torch_thread):
    import fullemu
    with fullemu.Installed():
        K.check_refusals("cpu")


# ---- the networks, through the interpreter ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fix():
    return K.load_fixtures()


@emulated
@pytest.mark.parametrize("tag", list(S.CASES))
def test_path_length_step_matches_the_fixture_through_the_interpreter(_one_torch_thread, fix, tag):
    import fullemu
    with fullemu.Installed() as E, K.bias_act_on_the_interpreter():
        K.check_network_fp32(E.lib, "cpu", fix, tag)


@emulated
def test_path_length_step_with_bf16_blocks_through_the_interpreter(_one_torch_thread, fix):
    import fullemu
    import make_golden_stylegan2_pl as M
    with fullemu.Installed() as E, K.bias_act_on_the_interpreter():
        K.check_network_bf16(E.lib, "cpu", fix, M.LOWP_CASE)


@emulated
def test_g_reg_step_accumulates_the_scaled_gradients(_one_torch_thread, fix):
    import fullemu
    with fullemu.Installed() as E, K.bias_act_on_the_interpreter():
        K.check_g_reg_step(E.lib, "cpu", fix)


@emulated
def test_style_mixing_and_truncation_of_generate_images(_one_torch_thread, fix):
    import fullemu
    with fullemu.Installed(), K.bias_act_on_the_interpreter():
        K.check_style_mixing("cpu", fix)


# ---- the configuration files -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.isdir("/root/reference/src/configs"), reason="the reference checkout is only present in the authoring container")
def test_pl_args_of_every_stylegan2_config():
    import yaml
    from studiogan_amd import config_map
    seen, applied = 0, 0
    for f in sorted(glob.glob("/root/reference/src/configs/*/*.yaml")):
        y = yaml.safe_load(open(f))
        if (y.get("MODEL") or {}).get("backbone") != "stylegan2":
            continue
        seen += 1
        kw = config_map.stylegan2_pl_args(y)
        assert sorted(kw) == ["apply_pl_reg", "betas", "g_reg_interval", "lr", "pl_no_weight_grad", "pl_weight", "style_mixing_p"], f
        O, St = y["OPTIMIZATION"], y["STYLEGAN"]
        assert (kw["apply_pl_reg"], kw["pl_weight"], kw["g_reg_interval"], kw["style_mixing_p"]) == (St["apply_pl_reg"], St["pl_weight"], St["g_reg_interval"],
                                                                                                      St["style_mixing_p"]), f
        assert kw["pl_no_weight_grad"] is True
        n = St["g_reg_interval"]
        ratio = n / (n + 1) if n != 1 else 1
        assert kw["lr"] == O["g_lr"] * ratio and kw["betas"] == [O["beta1"] ** ratio, O["beta2"] ** ratio], f
        applied += bool(kw["apply_pl_reg"])
    assert seen == 43 and applied == 20
    cifar = yaml.safe_load(open("/root/reference/src/configs/CIFAR10/StyleGAN2.yaml"))
    kw = config_map.stylegan2_pl_args(cifar)
    assert kw["apply_pl_reg"] is False and kw["style_mixing_p"] == 0.0 and kw["g_reg_interval"] == 4 and kw["lr"] == 0.0025 * 4 / 5 and kw["betas"] == [0.0, 0.99 ** (4 / 5)]
    afhq = yaml.safe_load(open("/root/reference/src/configs/AFHQ/StyleGAN2-SPD-ADA.yaml"))
    kw = config_map.stylegan2_pl_args(afhq)
    assert kw["apply_pl_reg"] is True and kw["pl_weight"] == 2 and kw["style_mixing_p"] == 0.9
    with pytest.raises(NotImplementedError):
        config_map.stylegan2_pl_args({"MODEL": {"backbone": "big_resnet"}})
    with pytest.raises(NotImplementedError):
        config_map.stylegan2_pl_args({"MODEL": {"backbone": "stylegan3"}, "STYLEGAN": {"g_reg_interval": 4, "style_mixing_p": 0.0}})
    with pytest.raises(NotImplementedError, match="g_reg_interval"):
        config_map.stylegan2_pl_args({"MODEL": {"backbone": "stylegan2"}, "STYLEGAN": {"style_mixing_p": 0.0}})
    with pytest.raises(NotImplementedError, match="pl_weight"):
        config_map.stylegan2_pl_args({"MODEL": {"backbone": "stylegan2"}, "STYLEGAN": {"g_reg_interval": 4, "style_mixing_p": 0.9, "apply_pl_reg": True}})


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", list(S.CASES))
def test_restatement_reproduces_the_pl_fixture(fix, tag):
    import make_golden_stylegan2_pl as M
    gen, pl = fix
    cfg = S.CASES[tag]
    sd32 = K.state(gen, tag)
    sd = {k: v.double() for k, v in sd32.items()}
    pkeys = M.param_keys(sd)
    assert pkeys == [k[len(tag) + 4:] for k in pl if k.startswith(f"{tag}/dp/")]
    z, c, noise = pl[f"{tag}/z"].double(), pl[f"{tag}/c"].double(), pl[f"{tag}/pl_noise"].double()
    want = M.inputs(list(S.CASES).index(tag), cfg, int(pl[f"{tag}/z_seed"]))
    assert all(torch.equal(a, b) for a, b in zip((z, c, noise), want)) and z.shape[0] == M.BATCH == 4
    lens, loss, mean, dp = M.pl(sd, cfg, z, c, noise, pkeys)
    err = lambda a, b: float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))      # noqa: E731
    assert err(lens, pl[f"{tag}/pl_lengths"]) <= 1e-12 and err(loss, pl[f"{tag}/loss"]) <= 1e-12 and err(mean, pl[f"{tag}/pl_mean"]) <= 1e-12
    zeros = []
    for k in pkeys:     # (stored as float32)
        assert float((dp[k] - pl[f"{tag}/dp/{k}"]).abs().max()) <= 2e-7 * float(dp[k].abs().max()), k
        assert (float(dp[k].abs().max()) > 0) == (f"{tag}/ref32_err/dp/{k}" in pl), k
        if float(dp[k].abs().max()) == 0:
            zeros.append(k)
    # exactly zero: every output bias (behind it nothing but linear maps lead to the image), and nothing else
    assert zeros and all(k.endswith("torgb.bias") for k in zeros)
    # no pre-activation within 4 fp32 errors of a kink (the premise of the fp32 bound), and the bf16 emulation alone inside the cap of differing sides
    assert M.kink_margin(sd, sd32, cfg, z, c, noise, pkeys) >= M.MARGIN
    if tag == M.LOWP_CASE:
        assert M.kink_margin(sd, sd32, cfg, z, c, noise, pkeys, **S.LOWP) >= M.MARGIN
        assert M.bf16_sides(sd, cfg, z, c, noise, pkeys) <= M.FLIP_CAP
        want, floors = M.lowp_floors(sd, cfg, z, c, noise, pkeys)
        assert err(want[1], pl[f"{tag}/lowp/loss"]) <= 1e-12
        assert 0 < float(pl[f"{tag}/bf16_floor"]) == max(floors.values())
        assert all(abs(float(pl[f"{tag}/bf16_floor_of/{k}"]) - v) <= 1e-9 * max(v, 1e-30) for k, v in floors.items())
