"""Sign planes on the kernel interpreter (tests/hipemu): every check of tests/sign_plane_checks.py at its tiny shapes, LDS-DMA completing late, waves scheduled
greedily in a seeded order -- before the first GPU launch. The same checks run on the GPU in tests/test_sign_plane_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu  # noqa: E402
import sign_plane_checks as SP  # noqa: E402

needs_emu = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def installed():
    import fullemu
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    with fullemu.Installed(dma_late=1, greedy=1, seed=11) as E:
        E.lib.sg_sign_plane_launches.restype = fullemu.C.c_longlong
        yield E
    torch.set_num_threads(n)


@needs_emu
@pytest.mark.parametrize("case", SP.PRODUCERS, ids=lambda c: "-".join(str(v) for v in c))
def test_emulated_producer_writes_the_plane_of_what_it_returns(installed, case):
    SP.producer_case(case, CPU)


@needs_emu
@pytest.mark.parametrize("case", SP.NON_PRODUCERS, ids=lambda c: "-".join(str(v) for v in c))
def test_emulated_engine_without_tile_epilogue_writes_no_plane(installed, case):
    SP.non_producer_case(case, CPU)


@needs_emu
@pytest.mark.parametrize("case", SP.CONSUMERS + SP.IGNORERS, ids=lambda c: "-".join(str(v) for v in c))
def test_emulated_consumer_plane_equals_activation(installed, case):
    SP.consumer_case(case, CPU)


@needs_emu
def test_emulated_blocks_switch_on_equals_off(installed):
    SP.block_case(CPU)
