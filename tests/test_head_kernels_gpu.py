"""GPU: the head, loss and penalty kernels (csrc/heads.hip, csrc/ext/losses.hip, the head / loss / WGAN-GP / LeCam sections of csrc/elementwise.hip,
sg_softmax_rows_bwd2) against an fp64 torch restatement at the shapes where a wave-per-row or one-block reduction goes wrong: more than one trip of the
lane-strided loop, partly filled blocks of four row-waves, ties for an arg-max, exact kinks, capped grids that wrap. The cases, the bound and the guards:
tests/head_checks.py; the same table runs on the CPU interpreter in tests/test_head_kernels_cpu.py."""
import pytest
import torch

import head_checks as HC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", HC.CASES, ids=HC.case_id)
def test_head_kernel_vs_fp64(sg, case):
    HC.run_case(case, torch.device("cuda:0"))
