"""Writes tests/golden/stylegan2_dis.npz: the REAL reference's StyleGAN2 Discriminator (src/models/stylegan2.py:551-924) on seeded parameters fp32 holds exactly
(multiples of 2^-6, nonzero biases), next to the fp64 expectation of tests/stylegan2_dis_ref.py.

The reference computes in float32. The script asserts that the restatement in fp32 agrees with it to fp32 rounding (2e-6), then stores the restatement's fp64
values as the expectation, with
    <case>/ref32_err/<what>   the reference's own distance from them (max |ref - fp64| / max |fp64|)
    <case>/bf16_floor         the distance of the restatement with bf16 storage in block b16 (conv_clamp 256), in the device's evaluation order with and
                              without fused_down (the larger of the two), from the fp64 run with the clamp: the largest over the outputs
Per case (stylegan2_dis_ref.CASES): <case>/keys (the reference's state_dict key list, in order), <case>/sd/<key>, <case>/{img,label}, <case>/g_<output> (the
upstream gradient of every returned tensor), <case>/out/<output> (fp64), <case>/lowp/<output> (fp64 with the clamp), <case>/dimg, <case>/dp/<parameter>
(stored as float32: the bound they are held to is 2e-5). The heads-only cases share the `orig` case's backbone state: they store the head's keys and
gradients only. It also checks, on the seeded inputs of the kernel tests, that rounding to bfloat16 moves no activation side and no clamp decision (cap 0).

    python tests/make_golden_stylegan2_dis.py      (needs the reference checkout: imported through oracle/ref_import.py)

Data only; TEST INFRASTRUCTURE ONLY."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import modconv_ref as R            # noqa: E402
import stylegan2_dis_ref as D      # noqa: E402

BF = torch.bfloat16


def err(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


def seeded_state(Dn, seed):
    """every entry of the state_dict (the filter constants aside) <- multiples of 2^-6; the label-embedding networks' layers at the scale their 0.01 lr
    multiplier implies"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in Dn.state_dict().items():
            if name.endswith("resample_filter"):
                continue
            v = (torch.randn(t.shape, generator=g, dtype=torch.float64) * 64).round() / 64
            if name.split(".")[0] in ("mapping", "embedding", "embedding_mi") and ".fc" in name:
                v = v * (128 if name.endswith("weight") else 32)
            if name.endswith("bias"):
                v = torch.where(v == 0, torch.full_like(v, 2.0 ** -6), v)
            t.copy_(v)


def compute():
    from oracle import ref_import as RI
    RI._prepare()
    sg2 = importlib.import_module("models.stylegan2")
    fix, backbone = {}, None
    for i, (tag, cfg) in enumerate(D.CASES.items()):
        full = tag in D.FULL_CASES
        Dn = sg2.Discriminator(**D.kwargs_of(cfg))
        seeded_state(Dn, 4000 + i)
        if tag == "orig":
            backbone = {k: v.detach().clone() for k, v in Dn.state_dict().items() if not D.is_head_key(k)}
        elif not full:
            Dn.load_state_dict(backbone, strict=False)
        sd32 = {k: v.detach().clone() for k, v in Dn.state_dict().items()}
        sd = {k: v.double() for k, v in sd32.items()}
        fix[f"{tag}/keys"] = np.array(list(sd32))
        for k, v in sd32.items():
            if full or D.is_head_key(k):
                fix[f"{tag}/sd/{k}"] = v.numpy()
        img, label, q = D.case_inputs(i, cfg)
        fix[f"{tag}/img"], fix[f"{tag}/label"] = img.float().numpy(), label.numpy()
        params = dict(Dn.named_parameters())
        pkeys = list(params)
        # the reference (fp32), the restatement in fp32 and in fp64
        il = img.float().requires_grad_(True)
        ref = Dn(il, label)
        assert list(ref) == list(D.OUT_KEYS)
        r32 = D.discriminator(sd32, cfg, img.float(), label)
        gys = {k: q(*v.shape) for k, v in D.float_outputs(r32).items()}
        out, dimg, dp = D.discriminator_grads(sd, cfg, img, label, gys, pkeys)
        assert {k for k, v in ref.items() if v is not None} == {k for k, v in out.items() if v is not None}, tag
        assert torch.equal(ref["label"], out["label"])
        for k, v in D.float_outputs(out).items():
            assert tuple(ref[k].shape) == tuple(v.shape), (tag, k, tuple(ref[k].shape), tuple(v.shape))
            assert err(r32[k], ref[k].detach()) <= 2e-6, (tag, k, err(r32[k], ref[k].detach()))
            fix[f"{tag}/out/{k}"] = v.numpy()
            fix[f"{tag}/g_{k}"] = gys[k].float().numpy()
            fix[f"{tag}/ref32_err/{k}"] = np.float64(err(ref[k].detach(), v))
        loss = sum((ref[k] * gys[k].float()).sum() for k in gys)
        gr = torch.autograd.grad(loss, [il] + list(params.values()), allow_unused=True)
        fix[f"{tag}/dimg"] = dimg.numpy()
        fix[f"{tag}/ref32_err/dimg"] = np.float64(err(gr[0], dimg))
        for k, gk in zip(pkeys, gr[1:]):
            if not (full or D.is_head_key(k)):
                continue
            fix[f"{tag}/dp/{k}"] = dp[k].float().numpy()
            gk = torch.zeros_like(params[k]) if gk is None else gk
            if float(dp[k].abs().max()) > 0:
                fix[f"{tag}/ref32_err/dp/{k}"] = np.float64(err(gk, dp[k]))
        if tag == "ac_adc":     # the fake copies of the classes
            fake = D.discriminator(sd, cfg, img, label, adc_fake=True)
            rf = Dn(img.float(), label, adc_fake=True)
            assert torch.equal(rf["label"], fake["label"]) and err(rf["cls_output"].detach(), fake["cls_output"]) <= 1e-5
            fix[f"{tag}/out_fake/cls_output"], fix[f"{tag}/out_fake/label"] = fake["cls_output"].numpy(), fake["label"].numpy()
        # low precision: fp64 with the clamp, and the same with bf16 storage in b16, in both evaluation orders of the device
        lowp = D.float_outputs(D.discriminator(sd, cfg, img, label, **D.LOWP))
        floor = 0.0
        for fused in (True, False):
            emu = D.discriminator(sd, cfg, img, label, act_dtype=BF, fused=fused, **D.LOWP)
            floor = max(floor, max(err(emu[k], v) for k, v in lowp.items()))
        for k, v in lowp.items():
            fix[f"{tag}/lowp/{k}"] = v.numpy()
        fix[f"{tag}/bf16_floor"] = np.float64(floor)
        worst = max(float(v) for k, v in fix.items() if k.startswith(f"{tag}/ref32_err/"))
        print(f"{tag}: worst ref32_err {worst:.2e}, bf16_floor {floor:.2e}")
    return fix


def check_head_seeds():
    """the kernel tests allow NO element on another side of the leaky ReLU or the clamp than fp64 (cap 0): the seeded inputs must survive the device's only
    rounding point in front of the activation, the bf16 storage of x (the bias enters in fp32), with every side unchanged and clear of the clamp"""
    for shape in D.HEAD_SHAPES:
        for pad in D.HEAD_PADS:
            for down in (1, 2):
                x, bias, gy = D.head_inputs(shape, pad, down)
                assert torch.equal(x.to(BF).double(), x) and torch.equal(bias.to(BF).double(), bias) and torch.equal(gy.to(BF).double(), gy), (shape, pad, down)
                pre = x + bias.reshape(1, -1, 1, 1)
                assert torch.equal(pre.float().double(), pre) and float(pre.abs().min()) > 0
                for epi, e in D.HEAD_EPI.items():
                    D.head_ref(x, bias, gy, pad, down, epi)     # (asserts the clamp margin and that the clamp bites)
    for case, (N, C, H, W, group, nch) in D.MBSTD_CASES.items():
        D.mbstd_inputs(case)        # (asserts every group's variance >= 2^-6)
    print("kernel-test seeds: every activation side and clamp decision survives bf16 storage (cap 0)")


if __name__ == "__main__":
    check_head_seeds()
    fix = compute()
    for key, v in fix.items():      # what fp32 holds exactly is stored as fp32; expectations stay fp64
        if v.dtype == np.float64 and "/sd/" in key:
            fix[key] = v.astype(np.float32)
    np.savez_compressed(D.GOLDEN, **fix)
    print(f"wrote {D.GOLDEN}: {len(fix)} arrays, {os.path.getsize(D.GOLDEN)} bytes")
    assert os.path.getsize(D.GOLDEN) < (1 << 20)
