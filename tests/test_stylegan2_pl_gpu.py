"""GPU parity of path-length regularisation through the StyleGAN2 generator: the second-order passes of style_ops.modulated_conv2d (csrc/modconv.hip
sg_modconv2d_jvp and the launches around it) and of the fused up = 2 layer tail (csrc/style_fir.hip sg_fir_bias_act_nhwc_gate), the
style_ops.second_order(generator=True) context, and losses.PathLengthRegularizer / stylegan_g_reg_step / stylegan_generate_images through the networks of
tests/golden/stylegan2_pl.npz. The checks are tests/stylegan2_pl_checks.py's, which the CPU suite runs through the kernel-source interpreter.

Bounds. fp32 operators: 2e-5 of the expected tensor's range; bf16 operators: 1e-2 against fp64 on bf16-rounded inputs. fp32 networks: max(2e-5, 4 ref32_err) per
quantity, ref32_err = the reference's own fp32 distance from the fp64 expectation (tests/make_golden_stylegan2_pl.py, which also shows that no pre-activation
is within 4 fp32 errors of a kink: the loss's parameter gradient jumps there). bf16 networks: 3 x the quantity's share of bf16_floor (3 x bf16_floor for a
one-element parameter), parameter gradients in relative L2 per tensor. Every measured error goes to profiles/stylegan2_pl_pytest_gpu.txt when the module is done."""
import os

import pytest
import torch

import make_golden_stylegan2_pl as M
import stylegan2_pl_checks as K
import stylegan2_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = []
DTYPES = [torch.float32, torch.bfloat16]
_name = K.dtype_name


@pytest.fixture(scope="module")
def fix():
    yield K.load_fixtures()
    try:
        with open(os.path.join(ROOT, "profiles", "stylegan2_pl_pytest_gpu.txt"), "w") as f:
            f.write("tests/test_stylegan2_pl_gpu.py on %s: max |got - expected| / max |expected| of every check (networks: bound = max(2e-5, 4 ref32_err), "
                    "bf16: 3 x the quantity's share of bf16_floor; [rel L2]: ||got - expected|| / ||expected||)\n" % torch.cuda.get_device_name(0))
            for name, e, tol in REPORT:
                f.write(f"{name:96s} err={e:.3e} tol={tol:.2e}\n")
    except OSError:
        pass


@pytest.mark.parametrize("route", ["fused", "composition"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("tag", K.MODCONV_CASES)
def test_modconv_second_order(sg, fix, tag, dtype, route):
    K.check_modconv_second_order(sg.lib(), DEV, tag, dtype, REPORT, route=route)


def test_tangent_route_follows_the_measured_rule(sg, fix):
    K.check_tangent_rule(sg.lib(), DEV, REPORT)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_modconv_second_order_with_post_gain(sg, fix, dtype):
    K.check_modconv_second_order(sg.lib(), DEV, "g", dtype, REPORT, gain=0.75)
    K.check_modconv_second_order(sg.lib(), DEV, "d", dtype, REPORT, gain=1.5)


def test_modconv_refuses_a_cotangent_on_the_weight_gradient(sg, fix):
    K.check_modconv_refuses_weight_cotangent(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("epi", list(K.TAIL_EPI))
@pytest.mark.parametrize("shape", list(S.TAIL_SHAPES))
def test_fir_bias_act_second_order(sg, fix, shape, epi, dtype):
    for noise in S.TAIL_NOISE:
        K.check_tail_second_order(sg.lib(), DEV, shape, noise, epi, dtype, REPORT)


def test_refusals_outside_the_generator_context_and_third_order(sg, fix):
    K.check_context_flags()
    K.check_refusals(DEV)


@pytest.mark.parametrize("tag", list(S.CASES))
def test_network_path_length_fp32_matches_fixture(sg, fix, tag):
    K.check_network_fp32(sg.lib(), DEV, fix, tag, REPORT)


def test_network_path_length_bf16_blocks(sg, fix):
    K.check_network_bf16(sg.lib(), DEV, fix, M.LOWP_CASE, REPORT)


def test_g_reg_step(sg, fix):
    K.check_g_reg_step(sg.lib(), DEV, fix, REPORT)


def test_style_mixing_and_truncation_of_generate_images(sg, fix):
    K.check_style_mixing(DEV, fix)
