"""The elementwise kernels with a scalar and a 16-byte instantiation of one body (csrc/elementwise.hip), host side: the counter's C ABI, and the checks of
tests/ew_checks.py through the kernel sources on the CPU interpreter (tests/hipemu); the same checks run on the GPU in tests/test_ew_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu  # noqa: E402
import ew_checks as EC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
needs_emu = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
CPU = torch.device("cpu")


def test_counter_is_declared_and_bound(sg):
    from studiogan_amd import _lib
    assert "sg_ew_vec_launches" in _lib._PROTOS
    assert "long long sg_ew_vec_launches(void);" in open(os.path.join(os.path.dirname(HERE), "include", "sgamd.h")).read()
    assert sg.lib().sg_ew_vec_launches() >= 0


def test_case_table_covers_both_paths_of_every_entry_point():
    for op in {c[0] for c in EC.CASES}:
        paths = {c[3] for c in EC.CASES if c[0] is op}
        assert paths == {True, False}, op.__name__
    assert len({c[0] for c in EC.CASES}) == 8 and len({EC.case_id(c) for c in EC.CASES}) == len(EC.CASES)


@pytest.fixture(scope="module")
def installed():
    import fullemu
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    with fullemu.Installed(dma_late=1, greedy=1, seed=5) as E:
        yield E
    torch.set_num_threads(n)


@needs_emu
@pytest.mark.parametrize("dtype", EC.DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_emulated_elementwise_exact_on_both_paths(installed, case, dtype):
    EC.run_case(case, CPU, dtype)
