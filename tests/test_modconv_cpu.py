"""Host-side checks of the modulated convolution (csrc/modconv.hip, style_ops/modulated_conv2d.py, backbones/stylegan2_layers.py): the plain-torch
restatement tests/modconv_ref.py reproduces the reference's fp64 outputs and gradients of tests/golden/modconv*.npz to 1e-12, the entry points are
exported and bound, sg_modconv2d_ok's truth table, every unsupported argument is refused by name before any device work, and the layers carry the
reference's state_dict keys. No GPU."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

import modconv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fix():
    return {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in R.load_golden().items()}


def _rel(a, e):
    return float((a.detach().double() - e.double()).abs().max() / max(float(e.abs().max()), 1e-300))


@pytest.mark.parametrize("tag", list(R.OP_CASES))
def test_ref_reproduces_golden_operator(fix, tag):
    N, C, Cout, H, k, up, demod, noise, flip = R.OP_CASES[tag]
    g = lambda n: fix[f"op/{tag}/{n}"].double() if f"op/{tag}/{n}" in fix else None      # noqa: E731
    assert tuple(g("x").shape) == (N, C, H, H) and tuple(g("w").shape) == (Cout, C, k, k) and (g("noise") is None) == (noise is None)
    assert bool((g("s") == 0).any()), "the styles of every case hold exact zeros"
    out = R.modconv_ref_grads(g("x"), g("w"), g("s"), g("noise"), g("gy"), up=up, demodulate=demod, flip_weight=flip, f=R.low_pass().double())
    for name, o in zip(("y", "dx", "dw", "ds", "dnoise"), out):
        if o is not None:
            assert _rel(o, g(name)) <= 1e-12, (tag, name, _rel(o, g(name)))


@pytest.mark.parametrize("tag", list(R.LAYER_CASES))
def test_ref_reproduces_golden_layer(fix, tag):
    cls, kw, res_in, mode = R.LAYER_CASES[tag]
    p = f"layer/{tag}/"
    sd = {k[len(p) + 3:]: v.double() for k, v in fix.items() if k.startswith(p + "sd/")}
    y, leaves = R.layer_ref(cls, kw, sd, fix[p + "x"].double(), fix[p + "w"].double(), mode)
    assert _rel(y, fix[p + "y"]) <= 1e-12
    names = [k for k in leaves]
    gr = torch.autograd.grad(y, [leaves[k] for k in names], fix[p + "gy"].double(), allow_unused=True)
    for k, g in zip(names, gr):
        e = fix[p + ("dx" if k == "x" else "dwl" if k == "wl" else "dp/" + k)]
        g = torch.zeros_like(e) if g is None else g
        assert float((g - e).abs().max()) <= 1e-12 * max(float(e.abs().max()), 1.0), (tag, k)


def test_entry_points_exported_and_bound(sg):
    from studiogan_amd import _lib as L
    lib = sg.lib()
    for name in ("sg_modconv2d_fwd", "sg_modconv2d_ok", "sg_modconv_launches", "sg_modconv_dcoef", "sg_modconv_reduce", "sg_modconv_reduce_slabs"):
        assert name in L.exported_symbols() and hasattr(lib, name), name
    assert lib.sg_modconv_launches() >= 0
    # the ctypes mirror has the size the C compiler gives the descriptor
    src = '#include <stdio.h>\n#include "sgamd.h"\nint main(){printf("%zu\\n", sizeof(sg_modconv_desc));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "s")], check=True)
        out = subprocess.run([os.path.join(d, "s")], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert int(out) == ctypes.sizeof(L.ModConvDesc)


def _desc(L, N, C, Cout, H, k, up, dtype=None, stride=None):
    d = L.ModConvDesc()
    c = d.conv
    c.dtype = L.F32 if dtype is None else dtype
    c.N, c.Hs, c.Ws, c.C, c.ldx, c.Cout, c.ldo = N, H, H, C, C, Cout, Cout
    c.R = c.S = k
    if up == 2:
        c.Ho = c.Wo = 2 * H + 1
        c.stride, c.pad_h, c.pad_w, c.pix_flags = 2, 0, 0, L.PIX_TRANSPOSED
    else:
        c.Ho = c.Wo = H
        c.stride, c.pad_h, c.pad_w = 1, k // 2, k // 2
    if stride is not None:
        c.stride = stride
        c.Ho = c.Wo = (H + 2 * c.pad_h - k) // stride + 1
    c.alpha = c.beta = 1.0
    return d


def test_ok_truth_table(sg):
    from studiogan_amd import _lib as L
    ok = lambda d: sg.lib().sg_modconv2d_ok(ctypes.byref(d))      # noqa: E731
    for tag, (N, C, Cout, H, k, up, *_r) in R.OP_CASES.items():
        for dtype in (L.F32, L.BF16):
            assert ok(_desc(L, N, C, Cout, H, k, up, dtype)) == 1, tag
        if up == 2:      # the data gradient of the up = 2 case: a plain stride-2 convolution from [2H + 1] back to [H]
            d = _desc(L, N, Cout, C, 2 * H + 1, 3, 1, stride=2)
            d.conv.pad_h = d.conv.pad_w = 0
            d.conv.Ho = d.conv.Wo = H
            assert ok(d) == 1, tag
    assert ok(_desc(L, 2, 8, 8, 9, 3, 1, stride=3)) == 0
    assert ok(_desc(L, 2, 8, 8, 8, 5, 1)) == 0
    assert ok(_desc(L, 2, 8, 8, 8, 3, 1, dtype=L.F64)) == 0


def test_unsupported_arguments_raise_by_name():
    from studiogan_amd.style_ops.modulated_conv2d import modulated_conv2d
    x, s = torch.zeros(2, 4, 8, 8), torch.ones(2, 4)      # CPU tensors: a refusal that came after any device work would be a different error
    w3, w1 = torch.zeros(6, 4, 3, 3), torch.zeros(6, 4, 1, 1)
    bad = {
        "down": dict(x=x, weight=w3, styles=s, padding=1, down=2),
        "up": dict(x=x, weight=w3, styles=s, padding=1, up=4),
        "weight": dict(x=x, weight=torch.zeros(6, 4, 4, 4), styles=s, padding=2),
        "kernel": dict(x=x, weight=torch.zeros(6, 4, 3, 1), styles=s, padding=1),
        "up=2": dict(x=x, weight=w1, styles=s, padding=0, up=2),
        "padding": dict(x=x, weight=w3, styles=s, padding=0),
        "float16": dict(x=x.half(), weight=w3, styles=s, padding=1),
        "float64": dict(x=x.double(), weight=w3, styles=s, padding=1),
        "noise": dict(x=x, weight=w3, styles=s, padding=1, noise=torch.zeros(2, 6, 8, 8)),
    }
    for name, kw in bad.items():
        with pytest.raises(NotImplementedError, match=name):
            modulated_conv2d(**kw)
    with pytest.raises(RuntimeError, match="GPU"):      # a supported problem on the CPU: no fallback
        modulated_conv2d(x, w3, s, padding=1)


def test_layers_carry_the_reference_state(fix):
    from studiogan_amd.backbones import stylegan2_layers as SL
    for tag, (cls, kw, res_in, mode) in R.LAYER_CASES.items():
        layer = getattr(SL, cls)(**kw)
        assert list(layer.state_dict().keys()) == list(fix["keys/" + cls]), cls
        p = f"layer/{tag}/sd/"
        layer.load_state_dict({k[len(p):]: v for k, v in fix.items() if k.startswith(p)}, strict=True)
    want = {"SynthesisLayer": {"affine.weight", "affine.bias", "weight", "bias", "noise_const", "noise_strength", "resample_filter"},
            "ToRGBLayer": {"affine.weight", "affine.bias", "weight", "bias"}}
    for cls, keys in want.items():
        assert set(fix["keys/" + cls]) == keys
    assert {"weight", "bias"} == set(SL.FullyConnectedLayer(4, 5).state_dict().keys())
