"""GPU: sign planes (tests/sign_plane_checks.py) -- producers, consumers and a stack of discriminator blocks, all bit-exact. The same checks run on the
kernel interpreter in tests/test_sign_plane_cpu.py."""
import pytest
import torch

import sign_plane_checks as SP

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", SP.PRODUCERS, ids=lambda c: "-".join(str(v) for v in c))
def test_producer_writes_the_plane_of_what_it_returns(sg, case):
    SP.producer_case(case, _dev())


@pytest.mark.parametrize("case", SP.NON_PRODUCERS, ids=lambda c: "-".join(str(v) for v in c))
def test_engine_without_tile_epilogue_writes_no_plane(sg, case):
    SP.non_producer_case(case, _dev())


@pytest.mark.parametrize("case", SP.CONSUMERS + SP.IGNORERS, ids=lambda c: "-".join(str(v) for v in c))
def test_consumer_plane_equals_activation(sg, case):
    SP.consumer_case(case, _dev())


def test_blocks_switch_on_equals_off(sg):
    SP.block_case(_dev())
