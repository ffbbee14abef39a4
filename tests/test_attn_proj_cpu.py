"""The attention block's fused projection kernels (csrc/attn_proj.hip) on the CPU interpreter at tiny shapes: LDS-DMA completing late, waves scheduled greedily
in a seeded order (tests/hipemu/README.md). The same checks run on the GPU at BigGAN-128's shapes in tests/test_attn_proj_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu  # noqa: E402
import attn_proj_checks as AP  # noqa: E402

needs_emu = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")


@pytest.fixture(scope="module")
def installed():
    import fullemu
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    with fullemu.Installed(dma_late=1, greedy=1, seed=7) as E:
        yield E
    torch.set_num_threads(n)


@needs_emu
@pytest.mark.parametrize("case", AP.TINY_SHAPES)
def test_emulated_forward_equals_separate_launches(installed, case):
    c0 = installed.counters()["launches"]
    AP.forward_case(case, torch.device("cpu"))
    assert installed.counters()["launches"] >= c0 + 7


@needs_emu
@pytest.mark.parametrize("case", AP.TINY_SHAPES)
@pytest.mark.parametrize("with_res", [True, False])
def test_emulated_data_gradient_matches_fp64(installed, case, with_res):
    AP.bwd_data_case(case, torch.device("cpu"), with_res)


@needs_emu
def test_emulated_predicate_rejects_other_shapes(installed):
    for B, H, C, Dp, Cg in AP.REJECTED:
        assert installed.lib.sg_attn_proj_ok(B, H, H, C, C, Dp, Cg) == 0
