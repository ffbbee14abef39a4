"""Writes tests/golden/stylegan2_gen.npz: the REAL reference's StyleGAN2 Generator (src/models/stylegan2.py:512-548) on seeded parameters fp32 holds exactly
(nonzero noise_strength and w_avg), next to the fp64 expectation of tests/stylegan2_ref.py.

The reference casts to float32 inside its networks, so its output is an fp32 evaluation. The script asserts that the restatement in fp32 agrees with it to
fp32 rounding, then stores the restatement's fp64 values as the expectation, with
    <case>/ref32_err/<what>   the reference's own distance from them (max |ref - fp64| / max |fp64|)
    <case>/bf16_floor         the distance of the restatement with bf16 activation storage (blocks b8, b16; conv_clamp 256) from <case>/img_lowp
Per case (stylegan2_ref.CASES): <case>/sd/<key> (the reference's state_dict), <case>/keys (its key list, in order), <case>/{z,c,gy}, <case>/img (noise_mode
const). For `skip` also img_none (noise_mode none), dz and dp/<parameter>, w (the mapping layers' output), ws_trunc (truncation_psi 0.7, cutoff 2) and
w_avg_after (one update_emas=True call). It also checks that the seeded inputs of the fused-tail GPU test keep the bf16 leaky-ReLU side flips of the
restatement itself under the 0.5 % cap that test allows the device.

    python tests/make_golden_stylegan2.py      (needs the reference checkout: imported through oracle/ref_import.py)

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
import stylegan2_ref as S      # noqa: E402

BF = torch.bfloat16


def err(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


def seeded_state(G, seed):
    """every entry of G's state_dict (the filter constants aside) <- multiples of 2^-6; the mapping layers at the scale their 0.01 lr multiplier implies"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in G.state_dict().items():
            if name.endswith("resample_filter"):
                continue
            v = (torch.randn(t.shape, generator=g, dtype=torch.float64) * 64).round() / 64
            if name.startswith("mapping.fc"):
                v = v * (128 if name.endswith("weight") else 32)
            if name.endswith("noise_strength"):
                v = v * 0.5 if float(v) != 0 else v + 0.5
            if name.endswith("affine.bias"):
                v = v * 0.25 + 1
            if name.endswith("w_avg"):
                v = v * 0.5
            t.copy_(v)


def compute():
    from oracle import ref_import as RI
    RI._prepare()
    sg2 = importlib.import_module("models.stylegan2")
    fix = {}
    for i, (tag, cfg) in enumerate(S.CASES.items()):
        G = sg2.Generator(**S.kwargs_of(cfg))
        seeded_state(G, 3000 + i)
        sd32 = {k: v.detach().clone() for k, v in G.state_dict().items()}
        sd = {k: v.double() for k, v in sd32.items()}
        fix[f"{tag}/keys"] = np.array(list(sd32))
        for k, v in sd32.items():
            fix[f"{tag}/sd/{k}"] = v.numpy()
        g = torch.Generator().manual_seed(3100 + i)
        q = lambda *s: (torch.randn(*s, generator=g, dtype=torch.float64) * 64).round() / 64      # noqa: E731
        z = q(S.BATCH, cfg["z_dim"])
        c = torch.eye(max(cfg["c_dim"], 1), dtype=torch.float64)[torch.arange(S.BATCH) % max(cfg["c_dim"], 1)][:, :cfg["c_dim"]]
        gy = q(S.BATCH, cfg["img_channels"], cfg["img_resolution"], cfg["img_resolution"])
        fix[f"{tag}/z"], fix[f"{tag}/c"], fix[f"{tag}/gy"] = z.float().numpy(), c.float().numpy(), gy.float().numpy()

        def both(noise_mode, what, **kw):
            """the reference (fp32), the restatement in fp32 and in fp64; stores the fp64 image"""
            ref = G(z.float(), c.float(), noise_mode=noise_mode, **kw).detach()
            r32 = S.generator(sd32, cfg, z.float(), c.float(), noise_mode, psi=kw.get("truncation_psi", 1), cutoff=kw.get("truncation_cutoff"))
            r64 = S.generator(sd, cfg, z, c, noise_mode, psi=kw.get("truncation_psi", 1), cutoff=kw.get("truncation_cutoff"))
            assert err(r32, ref) <= 2e-6, (tag, what, err(r32, ref))       # two fp32 evaluations of the same network
            fix[f"{tag}/{what}"] = r64.numpy()
            fix[f"{tag}/ref32_err/{what}"] = np.float64(err(ref, r64))
            return ref, r64

        both("const", "img")
        if tag == "skip":
            both("none", "img_none")
            both("const", "img_trunc", truncation_psi=0.7, truncation_cutoff=2)
            w = S.mapping_w(sd, cfg, z, c)
            fix[f"{tag}/w"] = w.numpy()
            fix[f"{tag}/ws_trunc"] = S.broadcast_truncate(w, S.num_ws(cfg), sd["mapping.w_avg"], 0.7, 2).numpy()
            ws_ref = G.mapping(z.float(), c.float(), truncation_psi=0.7, truncation_cutoff=2)
            assert err(ws_ref, torch.from_numpy(fix[f"{tag}/ws_trunc"])) <= 2e-6
            # gradients: the reference's fp32 autograd against the restatement's fp64 autograd
            zl = z.float().requires_grad_(True)
            params = dict(G.named_parameters())
            gr = torch.autograd.grad(G(zl, c.float(), noise_mode="const"), [zl] + list(params.values()), gy.float(), allow_unused=True)
            _, dz, dp = S.generator_grads(sd, cfg, z, c, gy)
            fix[f"{tag}/dz"] = dz.numpy()
            fix[f"{tag}/ref32_err/dz"] = np.float64(err(gr[0], dz))
            assert set(dp) == set(params), sorted(set(dp) ^ set(params))
            for (k, _), gk in zip(params.items(), gr[1:]):
                fix[f"{tag}/dp/{k}"] = dp[k].numpy()
                gk = torch.zeros_like(params[k]) if gk is None else gk
                if float(dp[k].abs().max()) > 0:
                    fix[f"{tag}/ref32_err/dp/{k}"] = np.float64(err(gk, dp[k]))
            # one moving-average update (a clone: the stored state keeps the w_avg the images were made with)
            G2 = sg2.Generator(**S.kwargs_of(cfg))
            G2.load_state_dict(sd32)
            G2.mapping(z.float(), c.float(), update_emas=True)
            exp = w.mean(dim=0) * (1 - 0.998) + sd["mapping.w_avg"] * 0.998
            assert err(G2.mapping.w_avg, exp) <= 2e-6
            fix[f"{tag}/w_avg_after"] = exp.numpy()
        # low precision: fp64 with the clamp, and the same with bf16 storage in b8 / b16
        lowp = S.generator(sd, cfg, z, c, "const", **S.LOWP)
        emu = S.generator(sd, cfg, z, c, "const", act_dtype=BF, **S.LOWP)
        fix[f"{tag}/img_lowp"] = lowp.numpy()
        fix[f"{tag}/bf16_floor"] = np.float64(err(emu, lowp))
        print(f"{tag}: ref32_err img {float(fix[f'{tag}/ref32_err/img']):.2e}, bf16_floor {float(fix[f'{tag}/bf16_floor']):.2e}")
    return fix


def check_tail_seeds():
    """bf16 runs of the fused tail may land on the other side of the leaky ReLU than fp64 on at most 0.5 % of the elements: the restatement with the device's
    rounding points (inputs and the stored core in bf16) must itself stay under that cap on the seeds tests/test_stylegan2_gpu.py uses"""
    rb = lambda t: t.to(BF).double()      # noqa: E731
    for shape in S.TAIL_SHAPES:
        for noise in S.TAIL_NOISE:
            x, w, s, nz, bias, gy = S.tail_inputs(shape, noise)
            _, pre = S.tail_ref(rb(x), rb(w), s, nz, bias)
            _, emu = S.tail_ref(rb(x), rb(w), s, nz, bias, core_dtype=BF)
            moved = int(((pre > 0) != (emu > 0)).sum())
            print(f"tail {shape} noise={noise}: {moved} of {pre.numel()} leaky-ReLU sides move under bf16 storage of the core")
            assert moved <= 0.005 * pre.numel(), (shape, noise, moved)


if __name__ == "__main__":
    check_tail_seeds()
    fix = compute()
    for key, v in fix.items():      # what fp32 holds exactly is stored as fp32; expectations stay fp64
        if v.dtype == np.float64 and "/sd/" in key:
            fix[key] = v.astype(np.float32)
    np.savez_compressed(S.GOLDEN, **fix)
    print(f"wrote {S.GOLDEN}: {len(fix)} arrays, {os.path.getsize(S.GOLDEN)} bytes")
    assert os.path.getsize(S.GOLDEN) < (1 << 20)
