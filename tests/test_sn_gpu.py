"""GPU: spectral norm at the kernel level (VERDICT r5 missing #5): sg_sn_forward / sg_sn_backward through the C ABI against torch.nn.utils.spectral_norm in fp64
(reference src/utils/ops.py:195-224) -- u, v, sigma, their snapshots, both operand images (forward [Cout][R][S][Cin_pad], data gradient [Cin][R'][S'][rows_pad],
flipped or not), the fp32 natural image of linear / embedding layers, and dW_orig = (G - <G, W/sigma> u v^T) / sigma accumulated into a non-zero gradient, for
plain / RGB-padded / transposed / 1x1 / 4x4 / eval-mode / un-normalised layers in ONE batched table per call."""
import pytest
import torch

import sn_checks as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sn_forward_backward_against_torch_spectral_norm(sg, dtype):
    from studiogan_amd import _lib as L
    rows = SC.run(torch.device("cuda:0"), dtype, L, L.call, L.ptr, L.stream)
    bad = [(n, e, t) for n, e, t in rows if not e <= t]
    for n, e, t in rows:
        print(f"{n:60s} err {e:.3e} (tol {t:.0e})")
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sn_table_with_a_row_wider_than_the_lds_row_buffer(sg, dtype):
    """SC.WIDE_LAYERS: one 30744-column layer sends the whole table to the fallback pack kernel k_sn_pack -- the same checks, the zero-filled padding of the forward
    image among them (the image buffers are pre-filled with 3.0)"""
    from studiogan_amd import _lib as L
    rows = SC.run(torch.device("cuda:0"), dtype, L, L.call, L.ptr, L.stream, layers=SC.WIDE_LAYERS)
    bad = [(n, e, t) for n, e, t in rows if not e <= t]
    for n, e, t in rows:
        print(f"{n:60s} err {e:.3e} (tol {t:.0e})")
    assert not bad, bad


def test_sn_forward_table_longer_than_one_flat_tile_table(sg):
    """csrc/sn.hip walks a table in runs of SN_MAXL = 64 layers (one flat tile table per run): 70 layers in ONE call = the same table handed over as [0, 37) + [37, 70), bit for bit."""
    from studiogan_amd import _lib as L
    dev = torch.device("cuda:0")
    shapes = [(16 + 8 * (i % 3), 8 + 8 * (i % 2), 3 if i % 5 else 1) for i in range(70)]
    one = SC.forward_table(dev, torch.bfloat16, L, L.call, L.ptr, L.stream, shapes, seed=5)
    two = SC.forward_table(dev, torch.bfloat16, L, L.call, L.ptr, L.stream, shapes, seed=5, split_at=37)
    for i, (a, b) in enumerate(zip(one, two)):
        for name, x, y in zip(("u", "v", "sigma", "w_fwd", "w_dgrad"), a, b):
            assert torch.equal(x, y), (i, shapes[i], name)
    assert all(float(a[2]) > 0 for a in one)
