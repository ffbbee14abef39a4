"""GPU: the batch-norm kernels (csrc/norm.hip) on every path their entry points dispatch to, stage by stage against fp64 restatements on given inputs, end to end
against the fp64 oracle, byte for byte between the kernels of one entry point, and element for element on the ReLU mask; sg_bn_path_launches() proves which kernel
ran. The cases and their bounds: tests/bn_checks.py."""
import pytest
import torch

import bn_checks as BC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("param", BC.params(gpu=True), ids=BC.param_id)
def test_batchnorm(sg, param):
    case, dtype = param
    BC.run_case(case, torch.device("cuda:0"), dtype)
