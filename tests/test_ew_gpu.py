"""GPU: the eight elementwise entry points whose scalar and 16-byte instantiations share one kernel body (csrc/elementwise.hip), byte for byte against an exact
torch restatement, with sentinels around every output and sg_ew_vec_launches() proving which instantiation ran. The cases: tests/ew_checks.py."""
import pytest
import torch

import ew_checks as EC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", EC.DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_elementwise_exact_on_both_paths(sg, case, dtype):
    EC.run_case(case, torch.device("cuda:0"), dtype)
