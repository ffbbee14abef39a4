"""GPU: which kernel family the convolution dispatchers hand a problem to, and whether that family is right there -- at the numeric edges of
every gate (csrc/conv*.hip `*_try`, csrc/conv_wgrad.hip wgrad_choose), with pitched operands (a channel slice of a wider tensor on every side) and
on non-square images. Every launch runs under util.engine_launches, every result is compared with CPU fp64 (autograd for the gradients); big
problems take the reference on the first and the last image only."""
import pytest
import torch

from util import check, engine_launches, launched
from test_kernels_gpu import rnd, _conv_ref

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -1232.0          # exactly representable in bf16


def _env(monkeypatch, env):
    for k in ("SG_CONV_SK", "SG_CONV_RS", "SG_CONV_RS96", "SG_CONV_RS_SH", "SG_CONV_V4", "SG_CONV_V3", "SG_CONV_V2", "SG_CONV_V2_MIN_TILES",
              "SG_WGRAD_SK", "SG_WGRAD_V3"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _wide(t, ld, coff, fill):
    """t [N, H, W, C] as the channel slice [coff, coff + C) of a new device tensor of pitch ld whose other channels hold `fill`; (wide, view)"""
    wide = torch.full(tuple(t.shape[:3]) + (ld,), fill, dtype=t.dtype, device="cuda:0")
    wide[..., coff:coff + t.shape[3]] = t.to("cuda:0")
    return wide


def _sel(N, J):
    return list(range(N)) if J <= 32768 else [0, N - 1]


def run_fwd(p, env, monkeypatch, poison=NAN):
    """One forward / data-gradient launch of problem p (a dict); returns the non-zero engine counts. Checks the result against fp64 and that no
    element of the output tensor outside the written slice changed."""
    from studiogan_amd import functional as F, _lib as L
    _env(monkeypatch, env)
    N, C, Co, H, W = p["N"], p["C"], p["Co"], p["H"], p["W"]
    R, stride = p.get("R", 3), p.get("stride", 1)
    pad = p.get("pad", R // 2)
    relu, up, pool = p.get("relu", False), p.get("up", False), p.get("pool", False)
    dt = torch.bfloat16
    x = rnd((N, C, H, W), dt, 401)
    w = rnd((Co, C, R, R), dt, 402, 0.1)
    bias = rnd((Co,), torch.float32, 403) if p.get("bias", not p.get("mask")) else None      # (a ReLU mask belongs to a data gradient: no bias)
    Ho, Wo = (H * (2 if up else 1) + 2 * pad - R) // stride + 1, (W * (2 if up else 1) + 2 * pad - R) // stride + 1
    Hy, Wy = (Ho // 2, Wo // 2) if pool else (Ho, Wo)
    res = rnd((N, Co, Hy, Wy), dt, 404) if p.get("res") else None
    msk = rnd((N, Co, Hy, Wy), dt, 405) if p.get("mask") else None
    sel = _sel(N, N * Ho * Wo)
    yref = _conv_ref(x[sel], w, stride, pad, relu, up, pool, bias, None)
    if msk is not None:
        yref = yref * (msk[sel].double() > 0)
    if res is not None:
        yref = yref + res[sel].double()
    if p.get("relu_out"):
        yref = torch.relu(yref)
    ldx, xo = C + p.get("ldx_extra", 0), p.get("x_coff", 0)
    ldo, oo = Co + p.get("ldo_extra", 0), p.get("out_coff", 0)
    xw = _wide(x.permute(0, 2, 3, 1), ldx, xo, poison)
    ow = torch.full((N, Hy, Wy, ldo), SENTINEL, dtype=dt, device="cuda:0")
    wd = w.permute(0, 2, 3, 1).contiguous().to("cuda:0")
    d = L.ConvFwdDesc()
    pf = (L.PIX_RELU if relu else 0) | (L.PIX_UPSAMPLE if up else 0)
    ef = (L.EPI_POOL if pool else 0) | (L.EPI_RELU if p.get("relu_out") else 0)
    bd = None if bias is None else bias.to("cuda:0")          # (the descriptor holds raw pointers: every operand stays referenced until the launch is done)
    F.conv2d_raw(xw, wd.data_ptr(), C, Co, R, R, stride, pad, pad, pf, ef, bias=bd, alpha=0.25 if pool else 1.0, out=ow, ldx=ldx, out_coff=oo, x_coff=xo, desc=d)
    keep = [xw, ow, wd, bd]
    if res is not None:          # residual and mask: slices of their own wide tensors, each with its own pitch; the neighbours hold the poison
        lr, ro = Co + p.get("ldr_extra", 0), p.get("res_coff", 0)
        rw = _wide(res.permute(0, 2, 3, 1), lr, ro, poison)
        d.res, d.ldr = rw.data_ptr() + 2 * ro, lr
        keep.append(rw)
    if msk is not None:
        lm, mo = Co + p.get("ldm_extra", 0), p.get("mask_coff", 0)
        mw = _wide(msk.permute(0, 2, 3, 1), lm, mo, poison)
        d.mask, d.ldm = mw.data_ptr() + 2 * mo, lm
        keep.append(mw)
    with engine_launches() as counts:
        L.call("sg_conv2d_fwd", d, L.stream())
    got = ow.float().cpu()
    name = f"{p} {env}"
    check("fwd " + name, got[sel][..., oo:oo + Co].permute(0, 3, 1, 2), yref, 4e-3)
    outside = torch.cat([got[..., :oo].reshape(-1), got[..., oo + Co:].reshape(-1)])
    assert bool((outside == SENTINEL).all()), f"{name}: {int((outside != SENTINEL).sum())} elements outside the output slice were written"
    return launched(counts)


def run_wgrad(p, env, monkeypatch, work="plan", poison=NAN):
    """One weight-gradient launch; work: 'plan' (the planned workspace), 'small' (one float short), 'none'."""
    from studiogan_amd import _lib as L
    _env(monkeypatch, env)
    N, C, Co, H, W = p["N"], p["C"], p["Co"], p["H"], p["W"]
    R = p.get("R", 3)
    pad = R // 2
    relu, up, pool = p.get("relu", False), p.get("up", False), p.get("pool", False)
    dt = torch.bfloat16
    x = rnd((N, C, H, W), dt, 411)
    w = rnd((Co, C, R, R), dt, 412, 0.1)
    wr = w.double().requires_grad_(True)
    y = _conv_ref(x, wr, 1, pad, relu, up, pool, None, None)
    gy = rnd(tuple(y.shape), dt, 413)
    y.backward(gy.double())
    ldx, xo = C + p.get("ldx_extra", 0), p.get("x_coff", 0)
    ldg, go = Co + p.get("ldg_extra", 0), p.get("dy_coff", 0)
    xw = _wide(x.permute(0, 2, 3, 1), ldx, xo, poison)
    gw = _wide(gy.permute(0, 2, 3, 1), ldg, go, poison)
    dw = torch.zeros((Co, R, R, C), dtype=torch.float32, device="cuda:0")
    d = L.ConvWgradDesc()
    d.dtype, d.N = L.BF16, N
    d.xHs, d.xWs, d.C, d.ldx = H, W, C, ldx
    d.x_flags = (L.PIX_RELU if relu else 0) | (L.PIX_UPSAMPLE if up else 0)
    d.gHs, d.gWs, d.Cout, d.ldg, d.g_flags = gy.shape[2], gy.shape[3], Co, ldg, (L.PIX_UPSAMPLE if pool else 0)
    d.Ho, d.Wo = H * (2 if up else 1), W * (2 if up else 1)
    d.R, d.S, d.stride, d.pad_h, d.pad_w = R, R, 1, pad, pad
    d.alpha = 0.25 if pool else 1.0
    d.x, d.dy, d.dw = xw.data_ptr() + 2 * xo, gw.data_ptr() + 2 * go, dw.data_ptr()
    sp, wf = L.C.c_int(0), L.C.c_longlong(0)
    L.call("sg_conv2d_wgrad_plan", d, L.C.byref(sp), L.C.byref(wf))
    buf = None
    if work != "none" and wf.value > 0:
        floats = wf.value - (1 if work == "small" else 0)
        buf = torch.empty(max(floats, 1), dtype=torch.float32, device="cuda:0")
        d.splits, d.work, d.work_floats = sp.value, buf.data_ptr(), floats
    with engine_launches() as counts:
        L.call("sg_conv2d_wgrad", d, L.stream())
    check(f"wgrad {p} {env} work={work}", dw.cpu().permute(0, 3, 1, 2), wr.grad, 2e-3)
    return launched(counts)


def P(N, C, Co, H, W=None, **kw):
    return dict(N=N, C=C, Co=Co, H=H, W=H if W is None else W, **kw)


# ---- a. gate edges: (problem, switches, expected engine), in pairs just inside / just outside each number of a gate --------------------------------
FORCE_SK, FORCE_V4, FORCE_V3, FORCE_V2 = {"SG_CONV_SK": "force"}, {"SG_CONV_V4": "force"}, {"SG_CONV_V3": "force"}, {"SG_CONV_V2": "force"}
FWD_EDGES = [
    # conv_sk: 1x1 with C <= 192, couts <= 384, J >= 16384 by default (16 images of 32 x 32 = 16384 pixels)
    ("sk C=192", P(16, 192, 96, 32, R=1), {}, "sk"),
    ("sk C=200", P(16, 200, 96, 32, R=1), {}, "gemm"),                  # (64 tiles of 96 couts: too few for conv_v2 as well)
    ("sk Cout=384", P(16, 96, 384, 32, R=1), {}, "sk"),
    ("sk Cout=392", P(16, 96, 392, 32, R=1), {}, "v2"),                 # 392 pads to four 128-wide tiles x 64 = 256 tiles
    ("sk J=16384", P(64, 96, 96, 16, R=1), {}, "sk"),
    ("sk J=16128", P(63, 96, 96, 16, R=1), {}, "gemm"),
    ("sk mask", P(16, 96, 96, 32, R=1, mask=True, bias=False), {}, "sk"),
    ("sk residual", P(16, 96, 96, 32, R=1, res=True), {}, "sk"),
    ("sk mask+residual", P(16, 96, 96, 32, R=1, mask=True, res=True, bias=False), {}, "gemm"),      # one staged operand tile: declines both
    ("sk W=12", P(2, 96, 96, 12, R=1), FORCE_SK, "gemm"),                # not a power of two
    ("sk W=1", P(512, 96, 96, 1, R=1), FORCE_SK, "gemm"),
    ("sk W=2", P(128, 96, 96, 2, R=1), FORCE_SK, "sk"),
    # conv_rs (<= 32 couts) / conv_rs96: 128-pixel rows, >= 64 strips by default (8-row images: one strip per image)
    ("rs strips=64", P(64, 96, 8, 8, 128), {}, "rs"),
    ("rs strips=63", P(63, 96, 8, 8, 128), {}, "gemm"),
    ("rs strips=64 by height", P(8, 96, 8, 64, 128), {"SG_CONV_RS_SH": "8"}, "rs"),
    ("rs strips=32 by height", P(8, 96, 8, 64, 128), {"SG_CONV_RS_SH": "16"}, "gemm"),
    ("rs96 strips=64", P(64, 96, 96, 8, 128, bias=False), {}, "rs"),
    ("rs96 strips=63", P(63, 96, 96, 8, 128, bias=False), {}, "v3"),     # 252 tiles of 96 couts: the halo kernel
    ("rs Cout=32", P(2, 96, 32, 8, 128), {"SG_CONV_RS": "force"}, "rs"),
    ("rs Cout=40", P(2, 96, 40, 8, 128), {"SG_CONV_RS": "force"}, "gemm"),
    ("rs Cout=8", P(2, 64, 8, 8, 128), {"SG_CONV_RS": "force"}, "rs"),
    ("rs Cout=4", P(2, 64, 4, 8, 128), {"SG_CONV_RS": "force"}, "gemm"),
    ("rs H=12", P(2, 96, 8, 12, 128), {"SG_CONV_RS": "force"}, "gemm"),    # strips are whole multiples of 8 rows
    ("rs out 8-byte aligned", P(2, 96, 8, 8, 128, ldo_extra=8, out_coff=4), {"SG_CONV_RS": "force"}, "rs"),
    ("16-byte stores decline 8-byte alignment", P(2, 96, 8, 8, 128, ldo_extra=8, out_coff=4), {"SG_CONV_RS": "0", "SG_CONV_V3": "force", "SG_CONV_V2": "force"}, "gemm"),
    ("rs96 pooled default", P(64, 96, 96, 8, 128, pool=True), {}, "v3"),
    ("rs96 pooled =1", P(64, 96, 96, 8, 128, pool=True), {"SG_CONV_RS96": "1"}, "rs"),
    # conv_v4: >= 768 tiles by default = couts / (32 NB) x J / 256: 96 couts, 48 images of 64 x 64 = 768 tiles, 47 = 752
    ("v4 tiles=768", P(48, 96, 96, 64, res=True), {}, "v4"),
    ("v4 tiles=752", P(47, 96, 96, 64, res=True), {}, "v3"),
    ("v4 C=384", P(2, 384, 96, 16), FORCE_V4, "v4"),
    ("v4 C=416", P(2, 416, 96, 16), FORCE_V4, "gemm"),
    ("v4 C=416 all", P(2, 416, 96, 16), {"SG_CONV_V4": "all"}, "v4"),
    ("v4 Cout=64", P(2, 64, 64, 16), FORCE_V4, "v4"),
    ("v4 Cout=96", P(2, 64, 96, 16), FORCE_V4, "v4"),
    ("v4 Cout=160", P(2, 64, 160, 16), FORCE_V4, "gemm"),
    ("v4 pool Wo=128", P(1, 32, 64, 128, pool=True), FORCE_V4, "v4"),
    ("v4 pool Wo=256", P(1, 32, 64, 256, pool=True), FORCE_V4, "v2"),       # the 256-pixel tile is not a pair of rows; 32 channels: conv_v2 (256 tiles)
    ("v4 up Wo=128", P(1, 32, 64, 64, up=True), FORCE_V4, "v4"),
    ("v4 up Wo=256", P(1, 32, 64, 128, up=True), FORCE_V4, "v2"),
    # conv_v3: >= 160 tiles by default (128 couts, 16 x 16 images: one tile each), or K >= 1152 with >= 16 tiles
    ("v3 tiles=160", P(160, 64, 128, 16), {}, "v3"),
    ("v3 tiles=159", P(159, 64, 128, 16), {}, "gemm"),
    ("v3 K=1152 tiles=16", P(16, 128, 128, 16), {}, "v3"),
    ("v3 K=1152 tiles=15", P(15, 128, 128, 16), {}, "gemm"),
    ("v3 K=864 tiles=16", P(16, 96, 128, 16), {}, "gemm"),
    ("v3 96 couts J=131072", P(512, 64, 96, 16, relu=True), {}, "v3"),        # the 512-pixel tile
    ("v3 96 couts J=130816", P(511, 64, 96, 16, relu=True), {}, "v3"),        # the 256-pixel tile
    ("v3 Cout=32", P(2, 96, 32, 32), FORCE_V3, "v3"),
    ("v3 Cout=40", P(2, 96, 40, 32), FORCE_V3, "gemm"),
    # conv_v2: >= 160 tiles by default (48 channels: no halo kernel), SG_CONV_V2_MIN_TILES moves the floor
    ("v2 tiles=160", P(160, 48, 128, 16), {}, "v2"),
    ("v2 tiles=159", P(159, 48, 128, 16), {}, "gemm"),
    ("v2 tiles=159 floor 159", P(159, 48, 128, 16), {"SG_CONV_V2_MIN_TILES": "159"}, "v2"),
    ("v2 Cout=64 padded", P(2, 48, 64, 16, ldo_extra=32, out_coff=16), FORCE_V2, "v2"),
    ("v2 Cout=40 too much padding", P(2, 48, 40, 16), FORCE_V2, "gemm"),
    ("v2 Cout=160 padded", P(2, 48, 160, 16, ldo_extra=32, out_coff=16), FORCE_V2, "v2"),
    ("v2 Cout=320 padded", P(2, 48, 320, 16, ldo_extra=32, out_coff=16), FORCE_V2, "v2"),
    ("v2 Cout=448 padded", P(2, 48, 448, 16, ldo_extra=32, out_coff=16), FORCE_V2, "v2"),
    ("v2 5x5", P(2, 16, 96, 16, R=5), FORCE_V2, "v2"),
    ("v2 7x7", P(2, 16, 96, 16, R=7), FORCE_V2, "gemm"),
    ("v2 stride 2", P(4, 64, 96, 16, stride=2), FORCE_V2, "v2"),
    ("v2 stride 2 + upsample", P(1, 64, 96, 16, stride=2, up=True), FORCE_V2, "gemm"),
]


@pytest.mark.parametrize("name,p,env,engine", FWD_EDGES, ids=[e[0].replace(" ", "_") for e in FWD_EDGES])
def test_forward_gate_edges(sg, name, p, env, engine, monkeypatch):
    assert run_fwd(p, env, monkeypatch) == {engine: 1}, name


WG_EDGES = [
    # wgrad_sk: 1x1 with row blocks of 32 input channels: 1, 2, 3 or 6 blocks (4 and 5 have no instantiation), <= 96 couts
    ("wgrad_sk C=96", P(2, 96, 96, 16, R=1), {}, "wgrad_sk"),
    ("wgrad_sk C=128", P(2, 128, 96, 16, R=1), {}, "wgrad_gemm"),
    ("wgrad_sk C=160", P(2, 160, 96, 16, R=1), {}, "wgrad_gemm"),
    ("wgrad_sk C=192", P(2, 192, 96, 16, R=1), {}, "wgrad_sk"),
    ("wgrad_sk Cout=104", P(2, 96, 104, 16, R=1), {}, "wgrad_gemm"),
    ("wgrad_sk stem W=32", P(2, 8, 96, 32), {}, "wgrad_sk"),
    ("wgrad_sk stem W=16", P(2, 8, 96, 16), {}, "wgrad_gemm"),
    # wgrad_v3: >= 16384 pixels by default (4 x 16 images: 64 pixels each), >= 4096 on 4 x 4 images in groups of four
    ("wgrad_v3 K=16384", P(256, 96, 96, 4, 16), {}, "wgrad_v3"),
    ("wgrad_v3 K=16320", P(255, 96, 96, 4, 16), {}, "wgrad_v2"),
    ("wgrad_v3 W=4 K=4096", P(256, 96, 96, 4), {}, "wgrad_v3"),
    ("wgrad_v3 W=4 K=4032", P(252, 96, 96, 4), {}, "wgrad_gemm"),
    ("wgrad_v3 W=4 N=260", P(260, 96, 96, 4), {}, "wgrad_v3"),
    ("wgrad_v3 W=4 N=258", P(258, 96, 96, 4), {}, "wgrad_v2"),
    ("wgrad_v3 W=128", P(1, 32, 64, 8, 128), {"SG_WGRAD_V3": "force"}, "wgrad_v3"),
    ("wgrad_v3 W=48", P(2, 32, 64, 16, 48), {"SG_WGRAD_V3": "force"}, "wgrad_gemm"),
    ("wgrad_v3 W=8 H=8", P(2, 32, 64, 8, 8), {"SG_WGRAD_V3": "force"}, "wgrad_v3"),
    ("wgrad_v3 W=8 H=4", P(4, 32, 64, 4, 8), {"SG_WGRAD_V3": "force"}, "wgrad_gemm"),     # a chunk is eight whole rows
    # wgrad_v2: >= 64 filter-row elements, >= 64 couts, >= 4096 pixels by default
    ("wgrad_v2 Cout=64", P(64, 16, 64, 4, 16), {}, "wgrad_v2"),
    ("wgrad_v2 Cout=56", P(64, 16, 56, 4, 16), {}, "wgrad_gemm"),
    ("wgrad_v2 I=64", P(64, 64, 128, 4, 16, R=1), {}, "wgrad_v2"),
    ("wgrad_v2 I=56", P(64, 56, 128, 4, 16, R=1), {}, "wgrad_gemm"),
    ("wgrad_v2 K=4032", P(63, 16, 64, 4, 16), {}, "wgrad_gemm"),
]


@pytest.mark.parametrize("name,p,env,engine", WG_EDGES, ids=[e[0].replace(" ", "_") for e in WG_EDGES])
def test_wgrad_gate_edges(sg, name, p, env, engine, monkeypatch):
    assert run_wgrad(p, env, monkeypatch) == {engine: 1}, name


@pytest.mark.parametrize("p,first,then", [
    (P(16, 96, 96, 16, R=1), "wgrad_sk", "wgrad_v2"),           # 4096 pixels: the tile kernel is next
    (P(2, 96, 96, 16, R=1), "wgrad_sk", "wgrad_gemm"),          # 512 pixels: the generic engine
    (P(64, 96, 96, 16), "wgrad_v3", "wgrad_v2"),
], ids=["sk-v2", "sk-gemm", "v3-v2"])
def test_wgrad_choose_steps_down_without_the_planned_workspace(sg, p, first, then, monkeypatch):
    """The streaming and the halo kernel exist in the workspace form only: with less than the planned workspace the same descriptor goes to the next engine"""
    assert run_wgrad(p, {}, monkeypatch, work="plan") == {first: 1}
    assert run_wgrad(p, {}, monkeypatch, work="small") == {then: 1}
    assert run_wgrad(p, {}, monkeypatch, work="none") == {then: 1}


# ---- b. pitched operands: x a slice of a wider tensor whose other channels hold NaN, the output a slice of a sentinel-filled tensor ------------------
PITCH = [dict(ldx_extra=32, x_coff=8, ldo_extra=64, out_coff=32, ldr_extra=16, res_coff=8, ldm_extra=24, mask_coff=16),
         dict(ldx_extra=32, x_coff=32, ldo_extra=64, out_coff=32, ldr_extra=8, res_coff=8, ldm_extra=8, mask_coff=0)]       # x_coff + C == ldx: the last row ends the allocation
FWD_PITCHED = [
    ("sk", P(2, 96, 48, 16, R=1, res=True), FORCE_SK),
    ("sk", P(5, 24, 192, 16, R=1, mask=True, bias=False), FORCE_SK),        # K = 24: zero-padded k tail
    ("sk", P(2, 8, 96, 32, mask=True, bias=False), FORCE_SK),               # the stem: 8 channels of a wider image
    ("sk", P(2, 96, 16, 16, R=1, pool=True), FORCE_SK),
    ("rs", P(2, 96, 8, 16, 128), {"SG_CONV_RS": "force"}),
    ("rs", P(2, 64, 24, 8, 128, relu=True), {"SG_CONV_RS": "force"}),
    ("rs", P(2, 96, 96, 16, 128, relu=True), {"SG_CONV_RS96": "force"}),
    ("rs", P(2, 96, 96, 16, 128, pool=True), {"SG_CONV_RS96": "force"}),
    ("v4", P(2, 96, 96, 16, res=True, mask=True), FORCE_V4),
    ("v4", P(2, 64, 128, 8, up=True, pool=True, res=True), FORCE_V4),
    ("v3", P(2, 96, 96, 16, res=True, mask=True), {"SG_CONV_V4": "0", "SG_CONV_V3": "force"}),
    ("v3", P(2, 160, 128, 16, pool=True, res=True), {"SG_CONV_V4": "0", "SG_CONV_V3": "force"}),
    ("v3", P(2, 96, 8, 32), {"SG_CONV_V4": "0", "SG_CONV_V3": "force"}),         # 8 couts on the 32-wide tile
    ("v3", P(2, 64, 16, 32, relu=True), {"SG_CONV_V4": "0", "SG_CONV_V3": "force"}),
    ("v2", P(2, 72, 64, 16, res=True, mask=True), FORCE_V2),                     # 64 couts on the 96-wide tile
    ("v2", P(2, 48, 160, 16, R=1, res=True), {"SG_CONV_V2": "force", "SG_CONV_SK": "0"}),
    ("v2", P(2, 40, 320, 16, relu=True), FORCE_V2),
    ("gemm", P(2, 72, 96, 12, res=True, mask=True), {"SG_CONV_V2": "0"}),
    ("gemm", P(1, 24, 16, 9, 7), {"SG_CONV_V2": "0"}),
]


@pytest.mark.parametrize("pitch", [0, 1])
@pytest.mark.parametrize("idx", range(len(FWD_PITCHED)), ids=["%s-%d" % (e[0], i) for i, e in enumerate(FWD_PITCHED)])
def test_forward_pitched_operands(sg, idx, pitch, monkeypatch):
    engine, p, env = FWD_PITCHED[idx]
    q = dict(p, **PITCH[pitch])
    assert run_fwd(q, env, monkeypatch) == {engine: 1}


WG_PITCHED = [
    ("wgrad_sk", P(2, 96, 48, 16, R=1, relu=True), {}),
    ("wgrad_sk", P(2, 24, 96, 16, R=1), {}),                       # zero-filled channel tail of the row block
    ("wgrad_sk", P(2, 8, 96, 32), {}),
    ("wgrad_sk", P(2, 96, 8, 32), {}),
    ("wgrad_v3", P(2, 96, 96, 32, relu=True), {"SG_WGRAD_V3": "force"}),
    ("wgrad_v3", P(4, 64, 64, 8, up=True, pool=True), {"SG_WGRAD_V3": "force"}),
    ("wgrad_v3", P(8, 96, 96, 4), {"SG_WGRAD_V3": "force"}),
    ("wgrad_v2", P(2, 64, 96, 16, relu=True), FORCE_V2),
    ("wgrad_v2", P(3, 72, 200, 8), FORCE_V2),
    ("wgrad_gemm", P(3, 72, 200, 8), {"SG_CONV_V2": "0"}),
]


@pytest.mark.parametrize("pitch", [0, 1])
@pytest.mark.parametrize("engine,p,env", WG_PITCHED, ids=["%s-%d" % (e[0], i) for i, e in enumerate(WG_PITCHED)])
def test_wgrad_pitched_operands(sg, engine, p, env, pitch, monkeypatch):
    q = dict(p, ldx_extra=32, x_coff=(8, 32)[pitch], ldg_extra=(64, 32)[pitch], dy_coff=32)      # (pitch 1: both slices end their tensors)
    assert run_wgrad(q, env, monkeypatch) == {engine: 1}


# ---- c. non-square images, both orders ------------------------------------------------------------------------------------------------
NONSQUARE_ENV = [("sk", 1, FORCE_SK), ("v4", 3, FORCE_V4), ("v3", 3, {"SG_CONV_V4": "0", "SG_CONV_V3": "force"}), ("v2", 3, {"SG_CONV_V4": "0", "SG_CONV_V3": "0", "SG_CONV_V2": "force"})]


@pytest.mark.parametrize("hw", [(8, 32), (32, 8)], ids=["8x32", "32x8"])
@pytest.mark.parametrize("variant", ["plain", "up", "pool"])
@pytest.mark.parametrize("engine,R,env", NONSQUARE_ENV, ids=[e[0] for e in NONSQUARE_ENV])
def test_forward_and_data_gradient_nonsquare(sg, engine, R, env, variant, hw, monkeypatch):
    H, W = hw
    p = P(3, 96, 96, H, W, R=R, relu=True, up=variant == "up", pool=variant == "pool", res=True)
    assert run_fwd(p, env, monkeypatch) == {engine: 1}
    # the launch its data gradient makes: the pooled gradient broadcast on load / the upsampling summed on store, the ReLU mask in the epilogue
    g = P(3, 96, 96, H * (2 if variant == "up" else 1) // (2 if variant == "pool" else 1), W * (2 if variant == "up" else 1) // (2 if variant == "pool" else 1),
          R=R, up=variant == "pool", pool=variant == "up", mask=True, bias=False)
    assert run_fwd(g, env, monkeypatch) == {engine: 1}


@pytest.mark.parametrize("hw", [(8, 32), (32, 8)], ids=["8x32", "32x8"])
@pytest.mark.parametrize("variant", ["plain", "up", "pool"])
@pytest.mark.parametrize("engine,R,env", [("wgrad_sk", 1, {}), ("wgrad_v3", 3, {"SG_WGRAD_V3": "force"}), ("wgrad_v2", 3, FORCE_V2)], ids=["wgrad_sk", "wgrad_v3", "wgrad_v2"])
def test_wgrad_nonsquare(sg, engine, R, env, variant, hw, monkeypatch):
    H, W = hw
    p = P(4, 64, 96, H, W, R=R, relu=True, up=variant == "up", pool=variant == "pool")
    assert run_wgrad(p, env, monkeypatch) == {engine: 1}


def test_wgrad_sk_stem_nonsquare(sg, monkeypatch):
    for (H, W) in ((8, 32), (16, 64)):
        assert run_wgrad(P(2, 8, 96, H, W), {}, monkeypatch) == {"wgrad_sk": 1}
        assert run_wgrad(P(2, 96, 8, H, W), {}, monkeypatch) == {"wgrad_sk": 1}
