"""Latent optimisation on class-conditional generators, host side: the C ABI of the conditional second-order batch-norm pass, and the checks of
tests/logan_cbn_checks.py through the kernel sources on the CPU interpreter (tests/hipemu); the same checks run on the GPU in tests/test_logan_cbn_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu  # noqa: E402
import logan_cbn_checks as LC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
needs_emu = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
NEW_SYMBOLS = ("sg_cbn_bwd2_reduce", "sg_cbn_bwd2_finalize", "sg_cbn_bwd2_apply", "sg_cbn_bwd2_dgain")
CPU = torch.device("cpu")


def test_new_symbols_are_declared_and_bound(sg):
    from studiogan_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sgamd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib._PROTOS and name + "(" in hdr, name


def test_recorded_bounds_follow_the_rule():
    """profiles/logan_cbn_bounds.txt: every recorded bound is max(4 x measured, 1e-6), the file lists exactly the outputs the checks bound, and the reference-side
    errors measured here are fp32 rounding like the recorded ones (below 2e-6; their exact size depends on the summation order of the torch build at hand)"""
    rec = {}
    sect = None
    for line in open(os.path.join(os.path.dirname(HERE), "profiles", "logan_cbn_bounds.txt")):
        if line.startswith("test "):
            sect = line.split()[1].rstrip(",") + (" bf16" if "bf16-rounded" in line else "")
        elif line.startswith("    ") and " measured " in line:
            p = line.split()
            k, m, b = " ".join(p[:p.index("measured")]), float(p[p.index("measured") + 1]), float(p[p.index("bound") + 1])
            assert abs(b - max(LC.MARGIN * m, LC.FLOOR)) <= 1e-3 * b, line
            rec[(sect, k)] = m
    live = {("1", k): v[0] for k, v in LC.bn_bounds(False).items()}
    live.update({("1 bf16", k): v[0] for k, v in LC.bn_bounds(True).items()})
    live.update({("2", k): v[0] for k, v in LC.affine_bounds().items()})
    assert sorted(rec) == sorted(live)
    for k, m in live.items():
        assert 0.0 < m <= 2e-6 and 0.0 < rec[k] <= 2e-6, (k, m, rec[k])


@pytest.fixture(scope="module")
def installed():
    import fullemu
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    with fullemu.Installed(dma_late=1, greedy=1, seed=5) as E:
        yield E
    torch.set_num_threads(n)


@needs_emu
@pytest.mark.parametrize("shape", LC.BN_SHAPES + LC.BN_EXTRA_SHAPES, ids=str)
def test_emulated_cbn_double_backward_vs_fp64_autograd(installed, shape):
    LC.bn_case(shape, CPU)


@needs_emu
@pytest.mark.parametrize("shape", LC.BN_SHAPES + LC.BN_EXTRA_SHAPES, ids=str)
def test_emulated_cbn_double_backward_bf16(installed, shape):
    LC.bn_case(shape, CPU, bf16=True)


@needs_emu
def test_emulated_cbn_equal_rows_match_the_per_channel_pass(installed):
    LC.bn_equal_rows_case(CPU)


@needs_emu
@pytest.mark.parametrize("C", [8, 24])
def test_emulated_cbn_affine_operators_double_backward(installed, C):
    LC.affine_case(C, CPU)


@needs_emu
@pytest.mark.parametrize("side", ["d", "g"])
@pytest.mark.parametrize("name", ["biggan32", "bigdeep32"])
def test_emulated_logan_update_vs_fp64_oracle(installed, name, side):
    LC.logan_update_case(name, side, CPU)


@needs_emu
def test_emulated_logan_latent_step_at_evaluation_time(installed):
    LC.logan_eval_case(CPU)


@needs_emu
def test_emulated_logan_mixed_precision_updates(installed):
    LC.logan_mixed_case(CPU)


@needs_emu
def test_emulated_first_order_path_issues_the_same_library_calls(installed):
    LC.first_order_case(CPU)


@needs_emu
def test_emulated_dcgan_generator_keeps_raising(installed):
    """the DCGAN generator's transposed convolutions have no differentiable backward: latent optimisation on it says so instead of cutting the graph"""
    from util import load_golden, sub
    from studiogan_amd import losses as SL
    fix, meta = load_golden("dcgan32")
    y = meta["yaml"]
    G, D = LC.build_pair(y, sub(fix, "G_init/"), sub(fix, "D_init/"), CPU)
    z, fl = sub(fix, "in/")["z0"], sub(fix, "in/")["fl0"]
    with pytest.raises(NotImplementedError, match="ConvTransposeFn"):
        SL.latent_optimise(zs=z, fake_labels=fl, generator=G, discriminator=D, batch_size=z.shape[0], lo_rate=0.8, lo_steps=2, lo_alpha=0.9, lo_beta=0.1, eval=False,
                           cal_trsp_cost=True, device=CPU)
