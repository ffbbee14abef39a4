"""CPU: the "bf16x6" fp32 mode (csrc/gemm_core.h SPLIT == 6) without a GPU -- the switch through every layer, the split's rounding rule restated in torch,
and the kernel itself on the interpreter (tests/hipemu) at the GPU tests' bounds (tests/test_f32x6_gpu.py has the same cases on the MI355X)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import f32x6_checks as X  # noqa: E402


def test_switch_through_every_layer(sg):
    from studiogan_amd import functional as F, _lib as L, metrics as M
    assert F.f32_mode.MODES == {"exact": 0, "bf16x3": 3, "bf16x6": 6}
    assert "sg_f32_split_launches" in L.exported_symbols()
    with open(os.path.join(os.path.dirname(HERE), "include", "sgamd.h")) as f:
        assert "long long sg_f32_split_launches(int mode);" in f.read()
    lib = L.lib()
    assert lib.sg_get_f32_mode() == 0
    assert lib.sg_f32_split_launches(3) >= 0 and lib.sg_f32_split_launches(6) >= 0 and lib.sg_f32_split_launches(5) == -1
    assert lib.sg_set_f32_mode(6) == 0 and lib.sg_get_f32_mode() == 6
    assert lib.sg_set_f32_mode(5) != 0 and lib.sg_get_f32_mode() == 6, "an unknown mode is refused and changes nothing"
    assert b"bf16x6" in lib.sg_last_error()
    assert lib.sg_set_f32_mode(0) == 0
    with F.f32_mode("bf16x6"):
        assert lib.sg_get_f32_mode() == 6
        with F.f32_mode("bf16x3"):
            assert lib.sg_get_f32_mode() == 3
        assert lib.sg_get_f32_mode() == 6
    assert lib.sg_get_f32_mode() == 0
    with pytest.raises(ValueError):
        F.f32_mode("bf16x9")
    # the evaluation models validate the name before they touch a device or a weight
    for cls in (M.InceptionV3, M.DINOViT):
        with pytest.raises(ValueError, match="f32_mode"):
            cls({}, torch.device("cpu"), torch.float32, f32_mode="bf16x9")


def test_environment_switch_in_a_fresh_process():
    """SG_F32_MODE is read once, when the library is loaded: a child process per value"""
    import subprocess
    root = os.path.dirname(HERE)
    for value, want in (("bf16x6", 6), ("bf16x3", 3), ("exact", 0)):
        r = subprocess.run([sys.executable, "-c", "import studiogan_amd._lib as L; print(L.lib().sg_get_f32_mode())"], cwd=root, text=True,
                           env=dict(os.environ, SG_F32_MODE=value, PYTHONPATH=root), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.strip().splitlines()[-1] == str(want), (value, r.stdout)


def test_three_term_split_is_exact():
    """h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest even, remainders in fp32: h + m + l == x on 2^16 seeded values over 80 binades with
    every significand bit in use -- the rounding rule f32x8_split3 (csrc/gemm_core.h) must follow. Also in the order the kernel's accumulator sees the terms of
    x * 1 (smallest first, fp32 additions), which is what lets the identity tests on the GPU ask for bit equality."""
    x = X.full_significand((1 << 16,), 7, -40, 40)
    assert float(x.abs().min()) >= 2.0 ** -40 and float(x.abs().max()) < 2.0 ** 40
    h, m, lo = X.split3(x)
    for t in (h, m, lo):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    assert torch.equal(h.double() + m.double() + lo.double(), x.double())
    assert torch.equal((lo + m) + h, x)
    # two terms are not enough: the bf16x3 split leaves a remainder on almost every such value
    assert int(((h + m) != x).sum()) > (1 << 15)


# the ragged case of the GPU parity test (K = 216: a tail inside a 16-wide k-tile; 35 pixels and 40 couts: ragged rows of the 128 x 128 tile in both dimensions; H != W),
# F32_SPLIT_CASES[1] (32 x 256 forward tile, 256 x 32 weight-gradient tile) and F32_SPLIT_CASES[0] at 9 x 9 (96 x 256 forward tile, 256 x 96 weight-gradient tile)
EMU_CASES = [(1, 24, 40, 7, 5, 3, 3, 1, (1, 1)), (2, 192, 32, 9, 9, 1, 1, 1, (0, 0)), (2, 64, 96, 9, 9, 3, 3, 1, (1, 1))]


@pytest.mark.parametrize("case", EMU_CASES)
def test_emulated_conv_in_bf16x6_mode(case):
    """forward and weight gradient in mode 6 on the interpreter, at the exact path's GPU bounds (2e-6 / 4e-6 of the largest output against fp64): the kernel uses
    no builtin the interpreter lacks, its indexing is right in both LDS forms, and the launches are counted as mode 6's. (The interpreter sums an MFMA's
    products in fp32, k ascending: what the hardware does inside the instruction is the GPU test's question.)"""
    import fullemu
    cpu = torch.device("cpu")
    with fullemu.Installed(dma_late=1, greedy=1, seed=4):
        e6 = X.conv_fwd(cpu, case, "bf16x6", lambda: None)
        e3 = X.conv_fwd(cpu, case, "bf16x3", lambda: None)
        w6, _ = X.conv_wgrad(cpu, case, "bf16x6", lambda: None)
        w3, _ = X.conv_wgrad(cpu, case, "bf16x3", lambda: None)
    print(f"{case}: forward bf16x6 {e6:.2e} bf16x3 {e3:.2e}; weight gradient bf16x6 {w6:.2e} bf16x3 {w3:.2e}")
    assert e6 <= 2e-6 and w6 <= 4e-6, (e6, w6)
    assert e6 < e3 and w6 < w3, "the six-product mode must be finer than the three-product one"


@pytest.mark.parametrize("pf,qf", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_emulated_gemm_in_bf16x6_mode(pf, qf):
    """sg_gemm in mode 6 on the interpreter: every operand-form pair on the all-vector path (44 x 76 x 72: all extents multiples of 4), batched with a bias;
    the bound is the GPU test's (relative L2 <= 1e-6 against fp64)"""
    import fullemu
    with fullemu.Installed(dma_late=1, greedy=1, seed=5):
        e = X.gemm(torch.device("cpu"), 44, 76, 72, pf, qf, "bf16x6", lambda: None, batch=2, bias=True)
    assert e <= 1e-6, e
