"""Writes tests/golden/modconv.npz, modconv_af.npz and modconv_c.npz (one fixture in three files, modconv_ref.load_golden reads them as one): the REAL reference's modulated_conv2d, SynthesisLayer and ToRGBLayer (src/models/stylegan2.py:28-98,265-341) evaluated
in fp64 on the CPU, on seeded inputs fp32 holds exactly and the file stores as fp32 (tests/modconv_ref.py exact_inputs; styles 1 + N(0,1), some exactly 0). Per operator case
(modconv_ref.OP_CASES): op/<tag>/{x,w,s,noise,gy} and op/<tag>/{y,dx,dw,ds,dnoise}. Per layer case (modconv_ref.LAYER_CASES): layer/<tag>/sd/<key> (the
reference's state_dict, random parameters), layer/<tag>/{x,w,gy}, layer/<tag>/y, layer/<tag>/{dx,dwl} and layer/<tag>/dp/<parameter>; keys/<class> = the
reference's state_dict key list. Each case is also evaluated on the reference's other route (fused_modconv=False): the two agree to 1e-12.

    python tests/make_golden_modconv.py      (needs the reference checkout: imported through oracle/ref_import.py)

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
import modconv_ref as R      # noqa: E402



def compute():
    from oracle import ref_import as RI
    RI._prepare()
    sg2 = importlib.import_module("models.stylegan2")
    up_mod = importlib.import_module("utils.style_ops.upfirdn2d")
    fix = {}
    f = up_mod.setup_filter([1, 3, 3, 1])
    for i, (tag, (N, C, Cout, H, k, up, demod, noise, flip)) in enumerate(R.OP_CASES.items()):
        x, w, s, nz, gy = R.exact_inputs(1000 + i, N, C, Cout, H, k, up, noise)
        res = []
        for fused in (True, False):
            lv = [t.clone().requires_grad_(True) for t in (x, w, s)] + ([nz.clone().requires_grad_(True)] if nz is not None else [])
            y = sg2.modulated_conv2d(lv[0], lv[1], lv[2], noise=lv[3] if nz is not None else None, up=up, padding=k // 2, resample_filter=f,
                                     demodulate=demod, flip_weight=flip, fused_modconv=fused)
            res.append([y.detach()] + list(torch.autograd.grad(y, lv, gy)))
        for a, b in zip(*res):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max())), tag
        y, dx, dw, ds = res[0][:4]
        for name, t in (("x", x), ("w", w), ("s", s), ("gy", gy), ("y", y), ("dx", dx), ("dw", dw), ("ds", ds)):
            fix[f"op/{tag}/{name}"] = t.numpy()
        if nz is not None:
            fix[f"op/{tag}/noise"], fix[f"op/{tag}/dnoise"] = nz.numpy(), res[0][4].numpy()
    for i, (tag, (cls, kw, res_in, mode)) in enumerate(R.LAYER_CASES.items()):
        g = torch.Generator().manual_seed(2000 + i)
        layer = getattr(sg2, cls)(**kw).double()
        if hasattr(layer, "resample_filter"):
            layer.resample_filter = layer.resample_filter.float()      # the reference insists on a float32 filter constant
        for name, t in layer.state_dict().items():
            if name != "resample_filter":
                t.copy_((torch.randn(t.shape, generator=g, dtype=torch.float64) * (0.5 if name == "noise_strength" else 1.0) * 64).round() / 64)
            if name == "affine.bias":
                t.add_(1.0)
        if "noise_strength" in dict(layer.named_parameters()) and float(layer.noise_strength.detach()) == 0:
            layer.noise_strength.data.fill_(0.5)
        fix[f"keys/{cls}"] = np.array(list(layer.state_dict().keys()))
        x = ((torch.randn(R.LAYER_BATCH, kw["in_channels"], res_in, res_in, generator=g, dtype=torch.float64) * 64).round() / 64).requires_grad_(True)
        wl = ((torch.randn(R.LAYER_BATCH, R.LAYER_WDIM, generator=g, dtype=torch.float64) * 64).round() / 64).requires_grad_(True)
        y = layer(x, wl, noise_mode=mode) if cls == "SynthesisLayer" else layer(x, wl)
        gy = (torch.randn(y.shape, generator=g, dtype=torch.float64) * 64).round() / 64
        params = dict(layer.named_parameters())
        gr = torch.autograd.grad(y, [x, wl] + list(params.values()), gy, allow_unused=True)
        for name, t in layer.state_dict().items():
            fix[f"layer/{tag}/sd/{name}"] = t.detach().numpy()
        for name, t in (("x", x), ("w", wl), ("gy", gy), ("y", y), ("dx", gr[0]), ("dwl", gr[1])):
            fix[f"layer/{tag}/{name}"] = t.detach().numpy()
        for name, t in zip(params, gr[2:]):
            fix[f"layer/{tag}/dp/{name}"] = (torch.zeros_like(params[name]) if t is None else t).detach().numpy()
    return fix


if __name__ == "__main__":
    fix = compute()
    # what fp32 holds exactly is stored as fp32 (inputs, parameters); expected values stay fp64
    for key, v in fix.items():
        if v.dtype == np.float64 and np.array_equal(v.astype(np.float32).astype(np.float64), v) and key.split("/")[-1] in ("x", "w", "s", "noise", "gy") + tuple(
                k for k in ("weight", "bias", "noise_const", "noise_strength", "resample_filter", "affine.weight", "affine.bias") if "/sd/" in key):
            fix[key] = v.astype(np.float32)
    # fp64 expectations do not compress: 229 k of them are 1.8 MB, so the cases are dealt to three files, each under the 1 MiB a committed file may have
    for name in R.GOLDEN_FILES:
        part = {k: v for k, v in fix.items() if R.golden_file_of(k) == name}
        out = os.path.join(HERE, "golden", name)
        np.savez_compressed(out, **part)
        print(f"wrote {out}: {len(part)} arrays, {os.path.getsize(out)} bytes")
        assert os.path.getsize(out) < (1 << 20)
