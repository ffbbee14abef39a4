"""GPU parity of R1 through the StyleGAN2 discriminator: the second-order passes of the head of a down layer (csrc/style_fir.hip sg_act_fir_nhwc_gate), of
the minibatch standard deviation (csrc/mbstd.hip sg_mbstd_bwd2) and of the plain convolutions, and losses.stylegan_cal_r1_reg / stylegan_d_reg_step through the
networks of tests/golden/stylegan2_r1.npz. The checks are tests/stylegan2_r1_checks.py's, which the CPU suite runs through the kernel-source interpreter.

Bounds. fp32 operators: 2e-5 of the expected tensor's range; bf16 operators: 1e-2 (inputs on grids bf16 holds, so no activation side differs from fp64).
fp32 networks: max(2e-5, 4 ref32_err) per quantity, ref32_err = the reference's own fp32 distance from the fp64 expectation (tests/make_golden_stylegan2_r1.py,
which also shows that no pre-activation is within 4 fp32 errors of a kink: the penalty's parameter gradient jumps there). bf16 networks: 3 x the quantity's share
of bf16_floor, parameter gradients in relative L2 per tensor. Every measured error goes to profiles/stylegan2_r1_pytest_gpu.txt when the module is done."""
import os

import pytest
import torch

import stylegan2_dis_ref as D
import stylegan2_r1_checks as K

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
        with open(os.path.join(ROOT, "profiles", "stylegan2_r1_pytest_gpu.txt"), "w") as f:
            f.write("tests/test_stylegan2_r1_gpu.py on %s: max |got - expected| / max |expected| of every check (networks: bound = max(2e-5, 4 ref32_err), "
                    "bf16: 3 x the quantity's share of bf16_floor; [rel L2]: ||got - expected|| / ||expected||)\n" % torch.cuda.get_device_name(0))
            for name, e, tol in REPORT:
                f.write(f"{name:96s} err={e:.3e} tol={tol:.2e}\n")
    except OSError:
        pass


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("down", [1, 2])
@pytest.mark.parametrize("shape", list(D.HEAD_SHAPES))
def test_head_second_order(sg, fix, shape, down, dtype):
    K.check_head_second_order(sg.lib(), DEV, shape, down, dtype, REPORT)


def test_head_gate_is_zero_outside_the_image(sg, fix):
    for down in (1, 2):
        K.check_gate_border(DEV, down, REPORT)


@pytest.mark.parametrize("case", list(K.MBSTD_R1_CASES))
def test_minibatch_std_second_order(sg, fix, case):
    K.check_mbstd_second_order(sg.lib(), DEV, case, REPORT)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", K.CONV_GEOMS, ids=lambda g: f"k{g[0]}s{g[1]}")
def test_conv2d_plain_second_order(sg, fix, geom, dtype):
    from studiogan_amd.style_ops import conv2d_resample as CR
    seen = set()
    for C in K.CONV_CHANNELS:
        seen |= K.check_conv_second_order(DEV, geom, C, dtype, REPORT)
    if dtype == torch.float32:
        assert seen == set(CR.ENTRIES)


def test_image_gradient_pass_launches_no_weight_gradient(sg, fix, monkeypatch):
    K.check_no_weight_gradient_in_the_first_pass(sg.lib(), DEV, monkeypatch)


def test_refusals_outside_the_context_and_third_order(sg, fix):
    K.check_refusals(DEV)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layerwise"])
@pytest.mark.parametrize("tag", list(D.FULL_CASES))
def test_network_r1_fp32_matches_fixture(sg, fix, tag, fused):
    K.check_network_fp32(sg.lib(), DEV, fix, tag, fused, REPORT)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layerwise"])
@pytest.mark.parametrize("tag", list(D.FULL_CASES))
def test_network_r1_bf16_blocks(sg, fix, tag, fused):
    K.check_network_bf16(sg.lib(), DEV, fix, tag, fused, REPORT)


def test_launch_counters_of_one_r1_step(sg, fix):
    K.check_launch_counters(sg.lib(), DEV, fix)


def test_d_reg_step(sg, fix):
    K.check_d_reg_step(sg.lib(), DEV, fix, REPORT)
