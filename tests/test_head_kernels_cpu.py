"""The head, loss and penalty kernels through their sources on the CPU interpreter (tests/hipemu): the table of tests/head_checks.py, the same cases, bounds
and guards as on the GPU (tests/test_head_kernels_gpu.py), and a test of the table itself: which ABI entry points, kinds and dtypes its cases reach.
No case is GPU only: the four cases of 4096 * 256 + 3 elements, where a capped grid wraps, take well under a second each on the interpreter."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu  # noqa: E402
import head_checks as HC  # noqa: E402

needs_emu = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
CPU = torch.device("cpu")


def test_case_ids_are_unique():
    assert len({HC.case_id(c) for c in HC.CASES}) == len(HC.CASES)


def test_case_table_reaches_every_entry_point_kind_and_dtype(sg, monkeypatch):
    """every case launched once with _lib.call replaced by a recorder (nothing runs: no GPU, no interpreter and no built library are needed): the ABI names reached are
    exactly the entry points in scope, each with every kind / dtype / accumulate value it has"""
    L = sg._lib
    seen = {}
    monkeypatch.setattr(L, "call", lambda name, *args: seen.setdefault(name, []).append(args))
    monkeypatch.setattr(L, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(L, "stream", lambda: None)
    for case in HC.CASES:
        HC.case_launch(case, CPU)()
    assert set(seen) == set(HC.ENTRY_POINTS)
    for name, want in HC.ENTRY_POINTS.items():
        if want is not None:
            assert {a[want[0]] for a in seen[name]} == want[1], name
    assert {a[2] is None for a in seen["sg_pd_head_fwd"]} == {True, False} and {a[3] is None for a in seen["sg_pd_head_fwd"]} == {True, False}      # b1, emb


@pytest.fixture(scope="module")
def installed():
    import fullemu
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    with fullemu.Installed(dma_late=1, greedy=1, seed=5) as E:
        yield E
    torch.set_num_threads(n)


@needs_emu
@pytest.mark.parametrize("case", HC.CASES, ids=HC.case_id)
def test_emulated_head_kernel_vs_fp64(installed, case):
    HC.run_case(case, CPU)
