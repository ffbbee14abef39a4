"""GPU tests of the DINO ViT evaluation backbone: every new kernel against an fp64 computation on the host, the whole model in both dtypes
against tests/vit_ref.py (the reference checkout is not needed here), the LoadEvalModel("DINO_torch") seam and the feature loop."""
import math

import numpy as np
import pytest
import torch

import vit_ref as VR
import make_golden_vit as MG
from util import check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _bf(t):
    return t.to(torch.bfloat16)


@pytest.mark.parametrize("C", [64, 384, 768])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_layernorm_rows(sg, C, out_dtype):
    from studiogan_amd import _lib as L
    g = torch.Generator().manual_seed(C)
    rows, pitch = 37, 3 * C + 8                                    # pitched rows: only the first C of every 3 C + 8 floats belong to a row
    buf = torch.randn(rows, pitch, generator=g) * 3.0 + 1.5
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
    ref = torch.nn.functional.layer_norm(buf[:, :C].double(), (C,), gamma.double(), beta.double(), 1e-6)
    x, gd, bd = buf.to(DEV), gamma.to(DEV), beta.to(DEV)
    out = torch.full((rows, 2 * C), 7.0, dtype=out_dtype, device=DEV)
    L.call("sg_layernorm_rows", L.dt(out_dtype), L.ptr(x), pitch, L.ptr(gd), L.ptr(bd), L.ptr(out), 2 * C, rows, C, 1e-6, L.stream())
    torch.cuda.synchronize()
    check(f"layernorm C={C} {out_dtype}", out[:, :C].float().cpu(), ref.float(), 5e-6 if out_dtype == torch.float32 else 5e-3)
    assert bool((out[:, C:] == 7.0).all()), "columns beyond C of the output pitch must stay untouched"


@pytest.mark.parametrize("M", [3 * 785, 17])
@pytest.mark.parametrize("K,N", [(384, 1152), (384, 384), (384, 1536), (1536, 384), (64, 192)])
def test_tok_gemm_epilogues(sg, M, K, N):
    from studiogan_amd import _lib as L
    g = torch.Generator().manual_seed(M + K + N)
    a, w, bias = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(N, K, generator=g) / math.sqrt(K)), torch.randn(N, generator=g)
    lin = a.double() @ w.double().t() + bias.double()
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    n0 = L.lib().sg_tok_gemm_launches()
    for epi, ref in ((0, lin), (1, torch.nn.functional.gelu(lin))):
        out = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
        L.call("sg_tok_gemm", epi, L.ptr(ad), K, L.ptr(wd), L.ptr(bd), L.ptr(out), N, M, N, K, L.stream())
        torch.cuda.synchronize()
        check(f"tok_gemm epi {epi} M={M} K={K} N={N}", out.float().cpu(), ref.float(), 6e-3)
    res = torch.randn(M, N, generator=g) * 2.0
    xs = res.to(DEV)
    for rep in (1, 2):                                             # in place: a second call accumulates onto the first
        L.call("sg_tok_gemm", 2, L.ptr(ad), K, L.ptr(wd), L.ptr(bd), L.ptr(xs), N, M, N, K, L.stream())
        torch.cuda.synchronize()
        check(f"tok_gemm fp32 residual x{rep} M={M} K={K} N={N}", xs.cpu(), (res.double() + rep * lin).float(), 2e-5)
    assert L.lib().sg_tok_gemm_launches() - n0 == 4


def _mha_case(N, H, B, seed, spike=False):
    from studiogan_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    C = 64 * H
    qkv = torch.randn(B, N, 3, H, 64, generator=g)
    qkv[:, :, :2] *= 1.6                                           # score rows spread over several units
    if spike:                                                      # one key of the LAST, partial key block dominates one query row
        kq, qq = N - 1, min(5, N - 1)
        qkv[:, kq, 1] = qkv[:, qq, 0] * 1.5
    qkv = _bf(qkv)
    q, k, v = (qkv[:, :, i].double().permute(0, 2, 1, 3) for i in range(3))
    ref = (((q @ k.transpose(-2, -1)) * 0.125).softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, N, C)
    # the activation is carved out of a larger buffer filled with NaN: a read past row N of the last image lands in the output
    big = torch.full((B * N * 3 * C + 4096 * 3 * C,), float("nan"), dtype=torch.bfloat16, device=DEV)
    big[:B * N * 3 * C] = qkv.reshape(-1).to(DEV)
    out = torch.full((B * N * C + 4096,), 3.0, dtype=torch.bfloat16, device=DEV)
    n0 = L.lib().sg_mha_launches()
    L.call("sg_mha_fwd", L.ptr(big), L.ptr(out), B, N, H, 64, 0.125, L.stream())
    torch.cuda.synchronize()
    assert L.lib().sg_mha_launches() - n0 == 1
    got = out[:B * N * C].float().cpu().reshape(B, N, C)
    assert bool(torch.isfinite(got).all()), "NaN / inf in the attention output: a read beyond row N"
    assert bool((out[B * N * C:] == 3.0).all()), "query rows beyond N were stored"
    check(f"mha N={N} H={H} B={B} spike={spike}", got, ref.float(), 1.5e-2)
    if spike:
        p = ((q @ k.transpose(-2, -1)) * 0.125).softmax(-1)[:, :, min(5, N - 1), N - 1]
        assert float(p.min()) > 0.9, "the spiked key does not dominate its row: the case tests nothing"


@pytest.mark.parametrize("N", [17, 128, 785])
@pytest.mark.parametrize("H", [1, 6])
def test_mha_fwd(sg, N, H):
    _mha_case(N, H, 2, 100 * H + N)


@pytest.mark.parametrize("N", [17, 785, 1])
def test_mha_fwd_spike_in_partial_block(sg, N):
    _mha_case(N, 2, 2, N, spike=N > 1)


def test_patch_convolution_8x8_stride_8(sg):
    from studiogan_amd import functional as F, _lib as L
    g = torch.Generator().manual_seed(8)
    x, w, b = torch.randn(3, 3, 64, 64, generator=g), torch.randn(128, 3, 8, 8, generator=g) / math.sqrt(192), torch.randn(128, generator=g)
    for dtype, tol in ((torch.float32, 2e-5), (torch.bfloat16, 8e-3)):
        xr, wr = x.to(dtype).double(), w.to(dtype).double()
        ref = torch.nn.functional.conv2d(xr, wr, b.double(), stride=8).permute(0, 2, 3, 1)
        wd = w.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)
        out = F.conv2d_raw(x.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV), wd.data_ptr(), 3, 128, 8, 8, stride=8,
                           epi_flags=L.EPI_OUT_F32 if dtype == torch.bfloat16 else 0, bias=b.to(DEV))
        torch.cuda.synchronize()
        assert out.dtype == torch.float32 and out.shape == (3, 8, 8, 128)
        check(f"8x8 / stride 8 patch convolution {dtype}", out.cpu(), ref.float(), tol)


def test_vit_tokens(sg):
    from studiogan_amd import _lib as L
    g = torch.Generator().manual_seed(2)
    B, N, C = 3, 17, 128
    patch, cls, pos = torch.randn(B, N - 1, C, generator=g), torch.randn(C, generator=g), torch.randn(N, C, generator=g)
    ref = torch.cat((cls.expand(B, 1, C), patch), 1) + pos
    pd, cd, posd = patch.to(DEV), cls.to(DEV), pos.to(DEV)
    x = torch.empty((B, N, C), dtype=torch.float32, device=DEV)
    L.call("sg_vit_tokens", L.ptr(pd), L.ptr(cd), L.ptr(posd), L.ptr(x), B, N, C, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), ref)


def test_normalise_ms_entry_points_keep_the_old_results(sg):
    """The (0.5, 0.5) entry points and the _ms ones with mean = std = 0.5 agree bit for bit, and per-channel constants do what they say. (Both now
    run the same kernel: that the OLD entry points still give their old values is what the untouched pre-processing tests of test_eval_gpu.py hold.)"""
    from studiogan_amd import metrics as M
    g = torch.Generator().manual_seed(6)
    for src, size in ((32, 299), (128, 224), (300, 224)):
        imgs = (torch.rand(2, 3, src, src, generator=g) * 2.4 - 1.2).to(DEV)
        for dtype in (torch.float32, torch.bfloat16):
            assert torch.equal(M.preprocess(imgs, dtype, True, size), M.preprocess(imgs, dtype, True, size, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)))
            for filt in ("bicubic", "bilinear"):
                assert torch.equal(M.preprocess_pil(imgs, dtype, filt, True, size),
                                   M.preprocess_pil(imgs, dtype, filt, True, size, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)))
    a = M.preprocess(imgs, torch.float32, True, 224)
    b = M.preprocess(imgs, torch.float32, True, 224, mean=M.IMAGENET_MEAN, std=M.IMAGENET_STD)
    want = ((a * 0.5 + 0.5) - torch.tensor(M.IMAGENET_MEAN, device=DEV)) / torch.tensor(M.IMAGENET_STD, device=DEV)
    check("per-channel mean / std", b.cpu(), want.cpu(), 1e-6)


def _small_model(dtype):
    from studiogan_amd import metrics as M
    return M.DINOViT(VR.random_state_dict(MG.SEED, VR.SMALL), torch.device(DEV), dtype)


def test_small_model_against_reference_fixture(sg):
    from studiogan_amd import _lib as L
    z = np.load(MG.FIXTURE)
    x, embed, logits = torch.from_numpy(z["x"]), torch.from_numpy(z["embed"]), torch.from_numpy(z["logits"])
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    g0, a0 = L.lib().sg_tok_gemm_launches(), L.lib().sg_mha_launches()
    e, l = _small_model(torch.float32).forward_nhwc(xn)
    torch.cuda.synchronize()
    assert (L.lib().sg_tok_gemm_launches(), L.lib().sg_mha_launches()) == (g0, a0), "the fp32 path must not touch the fused kernels"
    check("small ViT fp32 embed vs the reference's module", e.cpu(), embed, 2e-4)
    check("small ViT fp32 logits vs the reference's module", l.cpu(), logits, 2e-4)
    e, l = _small_model(torch.bfloat16).forward_nhwc(xn.to(torch.bfloat16))
    torch.cuda.synchronize()
    assert (L.lib().sg_tok_gemm_launches() - g0, L.lib().sg_mha_launches() - a0) == (4 * VR.SMALL["depth"], VR.SMALL["depth"])
    print(f"small ViT bf16 relative L2: embed {rel_l2(e, embed):.3e} logits {rel_l2(l, logits):.3e}")
    assert rel_l2(e, embed) <= BF16_REL_L2 and rel_l2(l, logits) <= BF16_REL_L2
    with pytest.raises(ValueError, match="interpolation"):
        _small_model(torch.float32).forward_nhwc(torch.zeros((1, 40, 40, 3), device=DEV))


# relative L2 of the bf16 path on embed / logits against the reference: measured on MI355X 6.0e-3 (ViT-S/8, B = 8), 5.7e-3 - 6.0e-3 through the three
# resizers, 7.3e-3 on the small geometry (the tests below print them); the bound is the largest of them x 1.5
BF16_REL_L2 = 1.1e-2


def test_vit_s8_full_size_both_dtypes(sg):
    from studiogan_amd import metrics as M, _lib as L
    geo = VR.VIT_S8
    sd = VR.random_state_dict(21, geo)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 224, 224, generator=g)
    e64, l64 = VR.vit_forward_f64(sd, x, geo["heads"])
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    g0, a0 = L.lib().sg_tok_gemm_launches(), L.lib().sg_mha_launches()
    e, l = M.DINOViT(sd, torch.device(DEV), torch.float32).forward_nhwc(xn)
    torch.cuda.synchronize()
    assert e.shape == (8, 1536) and l.shape == (8, 1000)
    assert (L.lib().sg_tok_gemm_launches(), L.lib().sg_mha_launches()) == (g0, a0)
    check("ViT-S/8 224^2 B=8 fp32 embed", e.cpu(), e64.float(), 2e-4)
    check("ViT-S/8 224^2 B=8 fp32 logits", l.cpu(), l64.float(), 2e-4)
    eb, lb = M.DINOViT(sd, torch.device(DEV), torch.bfloat16).forward_nhwc(xn.to(torch.bfloat16))
    torch.cuda.synchronize()
    assert (L.lib().sg_tok_gemm_launches() - g0, L.lib().sg_mha_launches() - a0) == (48, 12)
    re, rl = rel_l2(eb, e64), rel_l2(lb, l64)
    print(f"ViT-S/8 bf16 relative L2: embed {re:.3e} logits {rl:.3e} (bound {BF16_REL_L2:.1e})")
    assert re <= BF16_REL_L2 and rl <= BF16_REL_L2


@pytest.mark.parametrize("resizer", ["legacy", "clean", "friendly"])
def test_load_eval_model_dino(sg, resizer):
    """LoadEvalModel("DINO_torch", resizer) against the host pre-processing (reference-quantised uint8 image, the reference's resizer, ImageNet
    mean / std) + the restatement."""
    from PIL import Image
    from oracle import inception as OI
    from studiogan_amd import metrics as M
    geo = VR.VIT_S8
    sd = VR.random_state_dict(22, geo)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 64, 64, generator=g) * 2.2 - 1.1
    _, q = OI.quantize_resize_normalize(x, quantize=True, size=8)
    if resizer == "legacy":
        pre = torch.nn.functional.interpolate(torch.from_numpy(q.astype(np.float32)), size=(224, 224), mode="bilinear", align_corners=False).clamp(0, 255)
    else:
        flt = {"clean": Image.BICUBIC, "friendly": Image.BILINEAR}[resizer]
        pre = torch.zeros(2, 3, 224, 224)
        for n in range(2):
            for c in range(3):
                pre[n, c] = torch.from_numpy(np.asarray(Image.fromarray(q[n, c].astype(np.float32), mode="F").resize((224, 224), resample=flt)).copy())
    pre = (pre / 255.0 - torch.tensor(VR.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(VR.IMAGENET_STD).view(1, 3, 1, 1)
    _, qd = M.preprocess(x.to(DEV), torch.float32, True, 224, want_uint8=True, mean=M.IMAGENET_MEAN, std=M.IMAGENET_STD)
    assert np.array_equal(qd.cpu().numpy(), q), "uint8 quantisation must be bit-exact"
    e64, l64 = VR.vit_forward_f64(sd, pre, geo["heads"])
    model = M.LoadEvalModel("DINO_torch", resizer, 1, False, DEV, state_dict=sd, dtype=torch.float32)
    assert model.res == 224 and not model.weights_pinned
    e, l = model.get_outputs(x.to(DEV), quantize=True)
    torch.cuda.synchronize()
    check(f"DINO_torch {resizer} fp32 embed", e.cpu(), e64.float(), 2e-4)
    check(f"DINO_torch {resizer} fp32 logits", l.cpu(), l64.float(), 2e-4)
    eb, lb = M.LoadEvalModel("DINO_torch", resizer, 1, False, DEV, state_dict=sd, dtype=torch.bfloat16).get_outputs(x.to(DEV), quantize=True)
    torch.cuda.synchronize()
    print(f"DINO_torch {resizer} bf16 relative L2: embed {rel_l2(eb, e64):.3e} logits {rel_l2(lb, l64):.3e}")
    assert rel_l2(eb, e64) <= BF16_REL_L2 and rel_l2(lb, l64) <= BF16_REL_L2


def test_feature_loop_with_generator_dino(sg):
    """generate_images_and_stack_features + FeatureMoments(1536) end to end with the small BigGAN generator (reference features.py:17-65)."""
    from studiogan_amd import metrics as M
    from util import load_golden, sub
    from test_model_gpu import build_from_yaml
    dev = torch.device(DEV)
    fix, meta = load_golden("biggan32")
    G, _ = build_from_yaml(meta["yaml"], False, dev)
    G.load_state_dict({k: v.to(dev) for k, v in sub(fix, "G_init/").items()}, strict=True)
    G.eval()
    model = M.LoadEvalModel("DINO_torch", device=dev, state_dict=VR.random_state_dict(23, VR.VIT_S8), dtype=torch.bfloat16)
    mom = M.FeatureMoments(1536, dev)
    feats, probs, labels = M.generate_images_and_stack_features(G, model, 10, 4, 40, 10, quantize=True, device=dev, moments=mom)
    assert feats.shape == (12, 1536) and probs.shape == (12, 1000) and len(labels) == 12
    assert torch.isfinite(feats).all() and abs(float(probs.sum(1).mean()) - 1) < 1e-4
    mu, sigma = mom.finalize()
    assert mom.n == 10
    kept = feats[:10].double().cpu().numpy()
    check("DINO loop moments mean", torch.from_numpy(mu), torch.from_numpy(kept.mean(0)), 1e-5)
    check("DINO loop moments cov", torch.from_numpy(sigma), torch.from_numpy(np.cov(kept, rowvar=False)), 1e-4)


def test_top_k_accuracy_on_torch_backbone_columns(sg):
    """1000-column logits, classes at columns 0..999 (c0 = 0, reference ins.py:57-66), through eval_features(is_torch_backbone=True)."""
    from studiogan_amd import metrics as M
    g = torch.Generator().manual_seed(4)
    probs = torch.softmax(torch.randn(64, 1000, generator=g) * 3, 1)
    labels = torch.randint(0, 1000, (64,), generator=g)
    labels[:20] = probs[:20].argmax(1)
    order = probs.argsort(1, descending=True)
    want1 = float((order[:, 0] == labels).float().mean())
    want5 = float((order[:, :5] == labels[:, None]).any(1).float().mean())
    pd = probs.to(DEV)
    assert abs(M.top_k_accuracy(pd, labels.tolist(), 1, c0=0) - want1) < 1e-6
    assert abs(M.top_k_accuracy(pd, labels.tolist(), 5, c0=0) - want5) < 1e-6
    ident = {i: f"n{i:04d}" for i in range(1000)}
    _, _, t1, t5 = M.eval_features(pd, labels.tolist(), 64, 1, True, class_to_idx={v: k for k, v in ident.items()}, folder_label_dict={v: k for k, v in ident.items()},
                                   is_torch_backbone=True)
    assert abs(t1 - want1) < 1e-6 and abs(t5 - want5) < 1e-6
