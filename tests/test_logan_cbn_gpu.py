"""GPU: latent optimisation (LOGAN) on class-conditional generators -- the second-order pass through conditional batch norm (csrc/norm.hip sg_cbn_bwd2_*,
functional.CBNBwdFn), the affine products' differentiable data gradient (CbnAffineDgradFn) and the channel-slice skip's (SliceUpBwdFn) -- against torch autograd's fp64
double backward and the fp64 oracle's whole updates. The checks, their inputs and their bounds: tests/logan_cbn_checks.py (the measured reference-side errors behind
the operator-level bounds: profiles/logan_cbn_bounds.txt). Nothing here reads the reference checkout."""
import pytest
import torch

import logan_cbn_checks as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("shape", LC.BN_SHAPES + LC.BN_EXTRA_SHAPES, ids=str)
def test_cbn_double_backward_vs_fp64_autograd(sg, dev, shape):
    """relu x batch / running statistics x packed / separate rows, plus A = B = 0 and u = 0"""
    LC.bn_case(shape, dev)


@pytest.mark.parametrize("shape", LC.BN_SHAPES + LC.BN_EXTRA_SHAPES, ids=str)
def test_cbn_double_backward_bf16(sg, dev, shape):
    LC.bn_case(shape, dev, bf16=True)


def test_cbn_equal_rows_match_the_per_channel_pass(sg, dev):
    LC.bn_equal_rows_case(dev)


@pytest.mark.parametrize("C", [8, 24])
def test_cbn_affine_operators_double_backward(sg, dev, C):
    LC.affine_case(C, dev)


@pytest.mark.parametrize("side", ["d", "g"])
@pytest.mark.parametrize("name", ["biggan32", "bigdeep32"])
def test_logan_update_vs_fp64_oracle(sg, dev, name, side):
    LC.logan_update_case(name, side, dev)


def test_logan_latent_step_at_evaluation_time(sg, dev):
    LC.logan_eval_case(dev)


def test_logan_mixed_precision_updates(sg, dev):
    LC.logan_mixed_case(dev)


def test_first_order_path_issues_the_same_library_calls(sg, dev):
    LC.first_order_case(dev)
