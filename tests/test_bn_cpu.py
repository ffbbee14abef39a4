"""The batch-norm kernels (csrc/norm.hip), host side: the C ABI of the path counters and of the streaming-variant setter, the case table's coverage of every
(entry point, kernel) pair, and the checks of tests/bn_checks.py through the kernel sources on the CPU interpreter (tests/hipemu); the same checks run on the GPU
in tests/test_bn_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu  # noqa: E402
import bn_checks as BC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
needs_emu = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
CPU = torch.device("cpu")


def test_hooks_are_declared_and_bound(sg):
    from studiogan_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sgamd.h")).read()
    assert "sg_bn_path_launches" in _lib._PROTOS and "long long sg_bn_path_launches(int path);" in hdr
    assert "sg_bn_apply_variant" in _lib._PROTOS and "int sg_bn_apply_variant(int variant, int workgroups);" in hdr
    lib = sg.lib()
    paths, count = BC.header_paths()
    assert paths == BC.PATHS and count == sum(len(v) for v in BC.PATHS.values()), "tests/bn_checks.py PATHS does not follow the header's enum"
    for p in range(count):
        assert lib.sg_bn_path_launches(p) >= 0
    assert lib.sg_bn_path_launches(-1) == -1 and lib.sg_bn_path_launches(count) == -1
    assert lib.sg_bn_apply_variant(4, 8) != 0, "a variant above 3 is refused"
    for v in (0, 1, 2, 3, -1):
        assert lib.sg_bn_apply_variant(v, 8) == 0


@pytest.mark.parametrize("gpu", (False, True), ids=("interpreter", "gpu"))
def test_case_table_covers_every_path_of_every_entry_point(gpu):
    seen = BC.paths_in_table(gpu)
    assert seen == {e: set(k) for e, k in BC.PATHS.items()}, seen
    ids = [BC.param_id(p) for p in BC.params(gpu)]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]


@pytest.fixture(scope="module")
def installed():
    import fullemu
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    with fullemu.Installed(dma_late=1, greedy=1, seed=5) as E:
        yield E
    torch.set_num_threads(n)


@needs_emu
@pytest.mark.parametrize("param", BC.params(gpu=False), ids=BC.param_id)
def test_emulated_batchnorm(installed, param):
    case, dtype = param
    BC.run_case(case, CPU, dtype)
