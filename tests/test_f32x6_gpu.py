"""GPU: the "bf16x6" fp32 mode (csrc/gemm_core.h SPLIT == 6; functional.f32_mode, sg_set_f32_mode(6)): fp32 tensors, every operand element split into three
bf16 terms whose sum is the element exactly, six bf16 MFMAs per 16-wide k-tile (hl, lh, mm, mh, hm, hh), fp32 accumulation. What is dropped is at most 2^-25
of a product, so the mode is held to the EXACT path's bounds everywhere below: none of them is derived from what this kernel gives.
  1. identity: x * 1 comes back bit for bit (settles whether the 16-deep bf16 MFMA keeps the low terms)
  2. convolution forward / transposed / data gradient / weight gradient at the bounds test_kernels_gpu.py holds the exact path to (2e-6 / 4e-6 against fp64)
  3. sg_gemm: operand forms, batch, epilogues, split-K at relative L2 <= 1e-6 against fp64 (per-product error <= 2^-25 plus the fp32 accumulation of K <= 136
     terms, ~sqrt(K) * 2^-24 / sqrt(3) ~ 4e-7 at most in L2; the exact MFMA measures 0.75-1.5e-7)
  4. bf16x6 is at least 4x finer than bf16x3 on the same input
  5-7. InceptionV3, the DINO ViT and one fp32 training step in the mode, each at the bound its exact-mode test has
sg_f32_split_launches proves which arithmetic ran in every one of them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import f32x6_checks as X
from test_kernels_gpu import F32_SPLIT_CASES, rnd, nhwc, nchw
from util import check, one_launch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("exact", "bf16x3", "bf16x6")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device(DEV)


def sync():
    torch.cuda.synchronize()


# ---- 1. identity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def identity_input():
    """[2, 9, 9, 128] fp32, |x| in [2^-10, 2^10), every one of the 24 significand bits in use; shared, never written"""
    return X.full_significand((2, 9, 9, 128), 3, -10, 10)


def _identity_report(what, got, x):
    """(equal bit for bit?, a line saying how far off it is when not)"""
    same = torch.equal(got.view(torch.int32), x.view(torch.int32))
    bad = got != x
    worst = float(((got.double() - x.double()).abs() / x.double().abs()).max())
    line = f"identity {what}: {'bit-identical' if same else f'{int(bad.sum())} of {x.numel()} elements differ, worst relative {worst:.3e} (2^{np.log2(max(worst, 1e-300)):.1f})'}"
    print(line)
    return same, line


@pytest.mark.parametrize("path", ["conv", "gemm", "wgrad"])
def test_identity_is_bit_exact(sg, identity_input, path):
    """A contraction with the 128 x 128 identity returns its other operand: bit for bit in modes exact and bf16x6, NOT in bf16x3 (two terms keep 16 of the 24
    bits). Per output element one k carries x * 1 and every other product is a zero, so the accumulator sees l, then l + m, then (l + m) + h: each sum is exact
    in fp32 (tests/test_f32x6_cpu.py::test_three_term_split_is_exact), and the result is x if and only if the MFMA adds its products into the fp32 accumulator
    without truncating the low terms.
      conv : 1 x 1 convolution, weight = I (forward engine, [row][k] LDS images: frag_kc_f32_split3)
      gemm : sg_gemm form 0/0, P = I, Q = x as [162][128]
      wgrad: dy one-hot over pixels (cout c has its one at pixel (37 c + 5) mod 162), so dw[c][ci] = x[that pixel][ci] is a single contribution
             ([k][row] LDS images: frag_mc_f32_split3)"""
    from studiogan_amd import functional as F, _lib as L
    d = dev()
    x = identity_input
    xd = x.to(d)
    eye = torch.eye(128, dtype=torch.float32, device=d)
    pix = x.reshape(162, 128)
    sel = (37 * torch.arange(128) + 5) % 162
    assert len(set(sel.tolist())) == 128
    got = {}
    for mode in MODES:
        with X.split_launches(L, mode if (mode == "bf16x6" or path != "gemm") else "exact"), F.f32_mode(mode):      # (mode 3 does not reach sg_gemm)
            if path == "conv":
                y = F.conv2d_raw(xd, eye.data_ptr(), 128, 128, 1, 1)
                want = x
            elif path == "gemm":
                y = torch.empty((162, 128), dtype=torch.float32, device=d)
                F.gemm_raw(L.F32, eye, 0, 128, xd, 0, 128, y, 128, 128, 162, 128)
                want = pix
            else:
                dy = torch.zeros((162, 128), dtype=torch.float32)
                dy[sel, torch.arange(128)] = 1.0
                y = torch.zeros((128, 1, 1, 128), dtype=torch.float32, device=d)
                F.conv2d_wgrad_raw(xd, dy.reshape(2, 9, 9, 128).to(d), y.data_ptr(), 128, 128, 1, 1, 9, 9)
                want = pix[sel]
        sync()
        got[mode] = _identity_report(f"{path} {mode}", y.cpu().reshape(want.shape), want)
    assert got["exact"][0], got["exact"][1]
    assert got["bf16x6"][0], got["bf16x6"][1]
    if path != "gemm":
        assert not got["bf16x3"][0], "bf16x3 cannot return all 24 bits: the mode did not run"
    else:
        assert got["bf16x3"][0], "sg_gemm is outside mode 3's scope and stays exact"


# ---- 2. parity at the exact path's bounds -----------------------------------------------------------------------------------------------------------
# F32_SPLIT_CASES[0], [1], [5]: couts 96 / 32 / 384 = forward tiles 96 x 256, 32 x 256, 128 x 128, a stride of 2, K from 192 to 2592; then K = 216 (a tail inside a
# 16-wide k-tile), 35 pixels and 40 couts (ragged rows in both tile dimensions), H != W; then 8 input channels (I = 8: the 32 x 256 weight-gradient tile).
RAGGED = (1, 24, 40, 7, 5, 3, 3, 1, (1, 1))
PARITY_CASES = [F32_SPLIT_CASES[0], F32_SPLIT_CASES[1], F32_SPLIT_CASES[5], RAGGED, (2, 8, 64, 9, 9, 1, 1, 1, (0, 0))]
# weight gradient of each case: (tile, splits) -- the split count is asserted against sg_conv2d_wgrad_plan; the tile is an ASSUMPTION (X.wgrad_tile, a copy of
# conv_wgrad.hip's rule: the ABI does not report it), checked only against that copy so that the table cannot drift from it
WGRAD_PLANS = [((256, 96), 2), ((256, 32), 1), ((128, 128), 1), ((128, 128), 1), ((32, 256), 1)]
FWD_BOUND, WGRAD_BOUND = 2e-6, 4e-6          # test_kernels_gpu.py::test_conv_fwd_f32_bf16x3_split's bounds for the EXACT mode


@pytest.mark.parametrize("case,plan", list(zip(PARITY_CASES, WGRAD_PLANS)))
def test_conv_parity_at_the_exact_bounds(sg, case, plan):
    d = dev()
    with one_launch("gemm", f"forward {case}"):
        e = X.conv_fwd(d, case, "bf16x6", sync)
    print(f"{case}: forward bf16x6 {e:.2e} (bound {FWD_BOUND:.0e})")
    N, Cin, Cout, H, W, R, S, stride, pad = case
    assert X.wgrad_tile(R * S * Cin, Cout) == plan[0]      # (the table against the copied rule, not against the library)
    with one_launch("wgrad_gemm", f"weight gradient {case}"):
        w, splits = X.conv_wgrad(d, case, "bf16x6", sync)
    print(f"{case}: weight gradient bf16x6 {w:.2e} (bound {WGRAD_BOUND:.0e}), tile {plan[0]}, splits {splits}")
    assert splits == plan[1], (splits, plan)
    assert e <= FWD_BOUND, e
    assert w <= WGRAD_BOUND, w


def test_transposed_conv_and_its_data_gradient(sg):
    """test_kernels_gpu.py::test_conv_transpose's (3, 64, 32, 8, 8, 4, 2, 1): the transposed gather (the form a strided convolution's data gradient runs in) and
    the transposed convolution's own data gradient (a strided convolution), both forward-engine launches: the forward bound"""
    from studiogan_amd import functional as F, _lib as L
    N, Cin, Cout, H, W, R, stride, pad = 3, 64, 32, 8, 8, 4, 2, 1
    d = dev()
    x = rnd((N, Cin, H, W), torch.float32, 21)
    w = rnd((Cin, Cout, R, R), torch.float32, 22, 0.2)
    xr = x.double().requires_grad_(True)
    yref = TF.conv_transpose2d(xr, w.double(), None, stride=stride, padding=pad)
    Ho, Wo = yref.shape[2], yref.shape[3]
    gy = rnd(tuple(yref.shape), torch.float32, 24)
    yref.backward(gy.double())
    w_fwd = w.permute(1, 2, 3, 0).contiguous().to(d)
    w_dg = w.permute(0, 2, 3, 1).contiguous().to(d)
    xd, gyd = nhwc(x).to(d), nhwc(gy).to(d)
    with one_launch("gemm", "deconv forward"), X.split_launches(L, "bf16x6"), F.f32_mode("bf16x6"):
        y = F.conv2d_raw(xd, w_fwd.data_ptr(), Cin, Cout, R, R, stride, pad, pad, L.PIX_TRANSPOSED, transposed_out_hw=(Ho, Wo))
    with one_launch("gemm", "deconv data gradient"), X.split_launches(L, "bf16x6"), F.f32_mode("bf16x6"):
        dx = F.conv2d_raw(gyd, w_dg.data_ptr(), Cout, Cin, R, R, stride, pad, pad)
    sync()
    e_y, e_dx = X.max_err(nchw(y.cpu()), yref.detach()), X.max_err(nchw(dx.cpu()), xr.grad)
    print(f"transposed convolution bf16x6 {e_y:.2e}, its data gradient {e_dx:.2e} (bound {FWD_BOUND:.0e})")
    assert e_y <= FWD_BOUND and e_dx <= FWD_BOUND, (e_y, e_dx)


# ---- 3. sg_gemm ---------------------------------------------------------------------------------------------------------------------------------------
# the two shapes reach the all-vector path in form 0 only where K % 4 == 0 (both) and in form 1 only where the row count is a multiple of 4 (I = 40); the
# third shape has every extent a multiple of 4, so all four form pairs run mode 6. Which path a launch takes is asserted inside X.gemm from that rule.
GEMM_SHAPES = [(40, 70, 72), (130, 257, 136), (44, 76, 72)]
GEMM_BOUND = 1e-6


@pytest.mark.parametrize("I,J,K", GEMM_SHAPES)
@pytest.mark.parametrize("pf,qf", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_forms(sg, I, J, K, pf, qf):
    e = X.gemm(dev(), I, J, K, pf, qf, "bf16x6", sync)
    print(f"sg_gemm bf16x6 p{pf}q{qf} {I}x{J}x{K}: {e:.2e}")
    assert e <= GEMM_BOUND, e


@pytest.mark.parametrize("I,J,K", GEMM_SHAPES)
@pytest.mark.parametrize("what,kw", [("batch 3", dict(batch=3)), ("bias + residual, beta", dict(bias=True, res_beta=0.5)), ("alpha", dict(alpha=0.37)),
                                     ("alpha and alpha_ptr", dict(alpha=0.5, alpha_ptr=1.7)), ("atomic split-K", dict(splits=2)),
                                     ("batch 3, bias + residual", dict(batch=3, bias=True, res_beta=-1.25))])
def test_gemm_batch_epilogues_split_k(sg, I, J, K, what, kw):
    e = X.gemm(dev(), I, J, K, 0, 0, "bf16x6", sync, **kw)
    print(f"sg_gemm bf16x6 {what} {I}x{J}x{K}: {e:.2e}")
    assert e <= GEMM_BOUND, e


@pytest.mark.parametrize("I,J,K", GEMM_SHAPES)
def test_gemm_unaligned_operand_keeps_the_exact_mfma(sg, I, J, K):
    """P starts 4 bytes past a 16-byte boundary: the all-vector path declines, sg_f32_split_launches(6) stays (asserted in X.gemm), the result is the exact path's"""
    e = X.gemm(dev(), I, J, K, 0, 0, "bf16x6", sync, misalign=True)
    assert e <= GEMM_BOUND, e


# ---- 4. the modes are distinguishable -------------------------------------------------------------------------------------------------------------------
def test_bf16x6_is_four_times_finer_than_bf16x3(sg):
    """F32_SPLIT_CASES[5] (K = 2592), relative L2 against fp64 (the metric the 6-20x of the torch emulation was taken in): bf16x6 <= bf16x3 / 4"""
    d = dev()
    e = {m: X.conv_fwd(d, F32_SPLIT_CASES[5], m, sync, metric=X.l2_err) for m in MODES}
    mx = {m: X.conv_fwd(d, F32_SPLIT_CASES[5], m, sync) for m in MODES}
    print("relative L2: " + "  ".join(f"{m} {v:.2e}" for m, v in e.items()) + " | max of range: " + "  ".join(f"{m} {v:.2e}" for m, v in mx.items()))
    assert e["bf16x6"] <= e["bf16x3"] / 4, e


# ---- 5. InceptionV3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_inception_in_bf16x6_mode(sg):
    """InceptionV3 at 299^2, B = 4, seeded synthetic weights: pool3 features and logits in mode bf16x6 within the project's 2e-4 of the CPU oracle (the bound of
    test_eval_gpu.py for both existing modes); the distances to the exact mode's output are printed for both split modes."""
    from oracle import inception as OI
    from studiogan_amd import metrics as M, _lib as L
    d = dev()
    sd = OI.random_state_dict(1)
    g = torch.Generator().manual_seed(8)
    x = torch.rand(4, 3, 299, 299, generator=g) * 2 - 1
    feat_o, logit_o = OI.inception_forward(x, sd)
    xn = x.to(d).permute(0, 2, 3, 1).contiguous()
    out = {}
    for mode in MODES:
        model = M.InceptionV3(sd, d, torch.float32, f32_mode=mode)
        with X.split_launches(L, mode, want=None) as s:
            out[mode] = model.forward_nhwc(xn)
            sync()
            d3, d6 = (a - b for a, b in zip(s.counts(), s.before))
        assert (d3 > 0, d6 > 0) == (mode == "bf16x3", mode == "bf16x6"), (mode, d3, d6)
    for i, name in enumerate(("pool3 features", "logits")):
        dist = {m: float((out[m][i] - out["exact"][i]).abs().max() / out["exact"][i].abs().max()) for m in ("bf16x3", "bf16x6")}
        print(f"299^2 B=4 {name}: distance to the exact mode, of range: bf16x3 {dist['bf16x3']:.2e}  bf16x6 {dist['bf16x6']:.2e}")
    check("299^2 B=4 pool3 features fp32 bf16x6", out["bf16x6"][0], feat_o, 2e-4)
    check("299^2 B=4 logits fp32 bf16x6", out["bf16x6"][1], logit_o, 2e-4)


# ---- 6. DINO ---------------------------------------------------------------------------------------------------------------------------------------------
def test_dino_small_model_in_bf16x6_mode(sg):
    """tests/golden/vit_small.npz (the reference module's own outputs): DINOViT(fp32, f32_mode="bf16x6") within the fp32 bound of
    test_vit_gpu.py::test_small_model_against_reference_fixture (2e-4); the default mode leaves the split counters alone"""
    import vit_ref as VR
    import make_golden_vit as MG
    from studiogan_amd import metrics as M, _lib as L
    z = np.load(MG.FIXTURE)
    x, embed, logits = torch.from_numpy(z["x"]), torch.from_numpy(z["embed"]), torch.from_numpy(z["logits"])
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    sd = VR.random_state_dict(MG.SEED, VR.SMALL)
    with X.split_launches(L, "exact"):
        M.DINOViT(sd, torch.device(DEV), torch.float32).forward_nhwc(xn)
        sync()
    model = M.DINOViT(sd, torch.device(DEV), torch.float32, f32_mode="bf16x6")
    with X.split_launches(L, "bf16x6", want=None) as s:
        e, l = model.forward_nhwc(xn)
        sync()
        d3, d6 = (a - b for a, b in zip(s.counts(), s.before))
    # per block qkv, proj, fc1, fc2 and the q k^T product of each head, then the head (the 3-channel patch embedding and, at 17 tokens, the P V products
    # miss the all-vector path and keep the exact MFMA)
    assert d3 == 0 and d6 == (4 + VR.SMALL["heads"]) * VR.SMALL["depth"] + 1, (d3, d6)
    check("small ViT fp32 bf16x6 embed vs the reference's module", e.cpu(), embed, 2e-4)
    check("small ViT fp32 bf16x6 logits vs the reference's module", l.cpu(), logits, 2e-4)
    assert M.DINOViT(sd, torch.device(DEV), torch.bfloat16, f32_mode="bf16x6").f32_mode == "exact", "bf16 tensors ignore the mode"
    with pytest.raises(ValueError, match="f32_mode"):
        M.DINOViT(sd, torch.device(DEV), torch.float32, f32_mode="bf16x5")


def test_load_eval_model_routes_the_mode_to_dino(sg):
    import vit_ref as VR
    from studiogan_amd import metrics as M, _lib as L
    sd = VR.random_state_dict(22, VR.VIT_S8)
    assert M.LoadEvalModel("DINO_torch", device=DEV, state_dict=sd).model.f32_mode == "exact"
    model = M.LoadEvalModel("DINO_torch", device=DEV, state_dict=sd, f32_mode="bf16x6")
    assert model.model.f32_mode == "bf16x6"
    g = torch.Generator().manual_seed(9)
    with X.split_launches(L, "bf16x6", want=None) as s:
        e, l = model.get_outputs((torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).to(DEV), quantize=True)
        sync()
        assert s.counts()[1] > s.before[1] and s.counts()[0] == s.before[0]
    assert e.shape == (1, 1536) and l.shape == (1, 1000) and bool(torch.isfinite(e).all()) and bool(torch.isfinite(l).all())
    with pytest.raises(ValueError, match="f32_mode"):
        M.LoadEvalModel("DINO_torch", device=DEV, state_dict=sd, f32_mode="bf16x5")


# ---- 7. one fp32 training step --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def forced(monkeypatch):
    """the dispatch switches of test_fullwidth_gpu.py's fixture of the same name"""
    for k in ("SG_CONV_V4", "SG_CONV_V3", "SG_CONV_V2", "SG_CONV_SK", "SG_CONV_RS", "SG_CONV_RS96", "SG_WGRAD_BJ256", "SG_WGRAD_V3"):
        monkeypatch.setenv(k, "force")


def test_fp32_training_step_in_bf16x6_mode_vs_golden(sg, forced):
    """The helper behind test_fullwidth_gpu.py::test_fp32_training_step_in_bf16x3_mode_vs_golden on the smallest fixture that test uses (sngan32, width 8), in mode
    bf16x6 with gscale = 1: the EXACT arithmetic's bounds against the real reference's fp32 golden vectors (bf16x3 needs x8 on the gradients of this fixture)."""
    from test_model_gpu import step_vs_golden
    from studiogan_amd import functional as F, _lib as L
    with X.split_launches(L, "bf16x6", want=None) as s, F.f32_mode("bf16x6"):
        step_vs_golden("sngan32", False, gscale=1.0)
        assert s.counts()[1] > s.before[1] and s.counts()[0] == s.before[0]
