"""Sign planes (include/sgamd.h sg_conv_fwd_desc: the ReLU mask of a bf16 activation as one bit per element), checked the same way on the GPU
(tests/test_sign_plane_gpu.py) and on the kernel interpreter (tests/test_sign_plane_cpu.py). Everything here is EXACT: a plane is compared bit for bit
with the packed `y > 0` of the tensor the same launch returned, a launch that reads a plane is compared bit for bit with the launch that reads the
activation. The only tolerance is at block level, on the gradients that are accumulated with float atomics (biases, the attention gain): 1e-5 relative.

Shapes are the smallest each engine's gate admits (tests/test_conv_dispatch_gpu.py FWD_EDGES): three images of 16 x 16 (768 pixels = three 256-pixel tiles,
the quad kernel's 192 low-resolution positions are 1.5 tiles of 128), 192 output channels (two cout tiles, so the second one writes / reads at word
offset 3), 64 output channels on conv_v2 (a 96-wide tile whose last 16-byte chunks do not exist) and on conv_v4, pitched operands, a plane pitch one
word larger than ceil(C / 32)."""
import contextlib
import ctypes
import os

import torch

SENT = 0x5A5A5A5A                      # plane sentinel (int32)
OUT_SENT = -1232.0                     # output sentinel, exactly representable in bf16
ENGINE_NAMES = ("other", "sk", "rs", "v4", "v3", "v2", "gemm", "v4_skip", "q", "q_skip")
_SWITCHES = ("SG_CONV_SK", "SG_CONV_RS", "SG_CONV_RS96", "SG_CONV_V4", "SG_CONV_V3", "SG_CONV_V2", "SG_CONV_V2_MIN_TILES", "SG_CONV_Q", "SG_CONV_Q_BJ",
             "SG_SIGN_PLANE", "SG_QUAD", "SG_SKIP_FUSION")
ENV = {
    "v4": {"SG_CONV_V4": "force"},
    "v3": {"SG_CONV_V4": "0", "SG_CONV_V3": "force"},
    "v2": {"SG_CONV_V4": "0", "SG_CONV_V3": "0", "SG_CONV_V2": "force"},
    "gemm": {"SG_CONV_SK": "0", "SG_CONV_RS": "0", "SG_CONV_V4": "0", "SG_CONV_V3": "0", "SG_CONV_V2": "0"},
    "sk": {"SG_CONV_SK": "force"},
}


@contextlib.contextmanager
def env(values):
    saved = {k: os.environ.get(k) for k in _SWITCHES}
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


@contextlib.contextmanager
def engines(dev):
    """engine name -> launches inside the block (the library's launch profiler, as util.engine_launches, but also for the interpreter's CPU tensors)"""
    from studiogan_amd import _lib as L
    counts = {}
    L.call("sg_prof_enable", 1)
    try:
        yield counts
        _sync(dev)
        n = 15
        t = (ctypes.c_double * (n * 5))()
        L.call("sg_prof_collect_tags", t, n)
        for i, name in enumerate(ENGINE_NAMES):
            if int(t[i * 5]):
                counts[name] = int(t[i * 5])
    finally:
        _sync(dev)
        L.call("sg_prof_collect", (ctypes.c_double * 9)(), 3)
        L.call("sg_prof_enable", 0)


def plane_counts():
    from studiogan_amd import functional as F
    return F.sign_plane_counts()


def rnd_bf16(shape, seed, scale=1.0, dev=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def mask_values(shape, seed, dev):
    """a bf16 tensor drawn from {-1, -0.0, +0.0, the smallest positive subnormal, 1}: two of the five are positive, exact zeros of both signs are present"""
    g = torch.Generator().manual_seed(seed)
    table = torch.tensor([0xBF80, 0x8000, 0x0000, 0x0001, 0x3F80], dtype=torch.int32)
    raw = table[torch.randint(0, 5, shape, generator=g)].to(torch.int16)
    return raw.view(torch.bfloat16).to(dev)


def pack_plane(t):
    """reference plane of t [..., C] (bf16): int32 [..., ceil(C / 32)], bit c & 31 of word c >> 5 = t[..., c] > 0"""
    C = t.shape[-1]
    nw = (C + 31) // 32
    pos = (t.float().cpu() > 0).to(torch.int64)
    pad = torch.zeros(tuple(t.shape[:-1]) + (nw * 32,), dtype=torch.int64)
    pad[..., :C] = pos
    w = (pad.view(tuple(t.shape[:-1]) + (nw, 32)) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def bits_equal(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    if a.dtype == torch.bfloat16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.shape == b.shape and torch.equal(a, b)


def _wide(t, ld, fill):
    """t [N, H, W, C] as the first C channels of a tensor of pitch ld"""
    w = torch.full(tuple(t.shape[:3]) + (ld,), fill, dtype=t.dtype, device=t.device)
    w[..., :t.shape[3]] = t
    return w


def _sent_plane(N, H, W, ldw, dev):
    """a plane for N images with one image more behind it, all sentinel"""
    return torch.full((N + 1, H, W, ldw), SENT, dtype=torch.int32, device=dev)


# ---- 1. producers -------------------------------------------------------------------------------------------------------------------------
# (engine, C, Cout, pool, skip channels, ReLU on the result). N = 3, 16 x 16 inputs.
PRODUCERS = [
    ("v4", 64, 192, False, 0, False),
    ("v4", 32, 64, True, 0, True),
    ("v4_skip", 64, 192, False, 32, False),
    ("v4_skip", 32, 96, True, 32, False),
    ("v3", 64, 192, False, 0, True),
    ("v3", 96, 96, True, 0, False),
    ("v2", 64, 192, False, 0, False),
    ("v2", 48, 64, False, 0, True),           # 64 couts in a 96-wide tile: the third word does not exist
    ("q", 64, 192, True, 0, False),
    ("q", 32, 64, True, 0, False),
    ("q_skip", 32, 192, True, 32, False),
    ("q_skip", 64, 96, True, 32, False),
    # the streaming kernel: "sk3" = the RGB stem (3x3 over 8 padded channels), "sk1" = the 1x1 form; 192 couts = two accumulator passes of 96, 40 couts = a
    # second word of which only 8 bits exist
    ("sk3", 8, 96, False, 0, False),
    ("sk3", 8, 64, False, 0, True),
    ("sk1", 96, 192, False, 0, False),
    ("sk1", 64, 96, True, 0, True),
    ("sk1", 32, 40, False, 0, False),
]


def producer_case(case, dev):
    from studiogan_amd import functional as F, _lib as L
    eng, C, Co, pool, C2, relu_out = case
    R = 1 if eng == "sk1" else 3
    tag = "sk" if eng in ("sk1", "sk3") else eng
    N, H = 3, 16
    Hy = H // 2 if pool else H
    nw = (Co + 31) // 32
    ldo, ldw = Co + 8, nw + 1
    x = rnd_bf16((N, H, H, C), 11, dev=dev)
    bias = torch.linspace(-0.5, 0.5, Co).to(dev)
    x2 = rnd_bf16((N, H, H, C2), 12, dev=dev) if C2 else None
    w2 = rnd_bf16((Co, C2), 13, 0.1, dev) if C2 else None
    bias2 = torch.linspace(0.25, -0.25, Co).to(dev) if C2 else None
    ef = (L.EPI_POOL if pool else 0) | (L.EPI_RELU if relu_out else 0)
    quad = eng in ("q", "q_skip")
    w = rnd_bf16((Co, 16 if quad else R * R, C), 14, 0.1, dev)
    keep = [x, bias, x2, w2, bias2, w]

    def launch(plane):
        out = torch.full((N + 1, Hy, Hy, ldo), OUT_SENT, dtype=torch.bfloat16, device=dev)
        if quad:
            d = L.ConvQDesc()
            d.dtype, d.form, d.N, d.Hl, d.Wl, d.C, d.ldx, d.Cout = L.BF16, L.Q_POOL, N, H // 2, H // 2, C, C, Co
            d.pix_flags, d.epi_flags, d.alpha, d.beta = L.PIX_RELU, (L.EPI_RELU if relu_out else 0), 1.0, 1.0
            d.x, d.wq, d.bias, d.out, d.ldo = x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), ldo
            if C2:
                d.x2, d.w2q, d.bias2, d.C2, d.ldx2 = x2.data_ptr(), w2.data_ptr(), bias2.data_ptr(), C2, C2
            name = "sg_conv2d_q"
            main = d
        else:
            d = L.ConvSkipDesc() if C2 else L.ConvFwdDesc()
            main = d.main if C2 else d
            F.conv2d_raw(x, w.data_ptr(), C, Co, R, R, 1, R // 2, R // 2, L.PIX_RELU, ef, bias=bias, alpha=0.25 if pool else 1.0, out=out, desc=main)
            if C2:
                d.x2, d.w2, d.bias2, d.C2, d.ldx2, d.x2_up = x2.data_ptr(), w2.data_ptr(), bias2.data_ptr(), C2, C2, 0
            name = "sg_conv2d_fwd_skip" if C2 else "sg_conv2d_fwd"
        if plane is not None:
            main.sign_out, main.lds = plane.data_ptr(), ldw
            main.epi_flags |= L.EPI_PLANES
        with engines(dev) as counts:
            L.call(name, d, L.stream())
        assert counts == {tag: 1}, f"{case}: expected one {tag} launch, the profiler saw {counts}"
        return out

    with env(ENV.get(tag, {})):
        y0 = launch(None)
        plane = _sent_plane(N, Hy, Hy, ldw, dev)
        before = plane_counts()
        y1 = launch(plane)
        after = plane_counts()
    assert after[0] == before[0] + 1, f"{case}: the library did not count a plane-writing launch"
    assert bits_equal(y1, y0), f"{case}: the output changed with sign_out"
    assert bool((y1[N:] == OUT_SENT).all()) and bool((y1[:N, ..., Co:] == OUT_SENT).all()), f"{case}: output written outside its rows"
    y = y1[:N, ..., :Co]
    if relu_out:
        assert bool((y == 0).any())
    assert bits_equal(plane[:N, ..., :nw], pack_plane(y)), f"{case}: plane != packed (y > 0)"        # (tail bits of the last word are zero in the reference)
    assert bool((plane[N:] == SENT).all()) and bool((plane[:N, ..., nw:] == SENT).all()), f"{case}: plane words outside the written rows changed"
    del keep


# the engines without a plane pass (the generic GEMM, the row-streaming kernels) do not write planes: the launch must say so, and the carrier stays empty
NON_PRODUCERS = [("gemm", 64, 96, 3), ("gemm", 96, 96, 1), ("v3", 96, 32, 3)]      # (conv_v3's 32-cout tile is compiled without the plane code)


def non_producer_case(case, dev):
    from studiogan_amd import functional as F, _lib as L
    eng, C, Co, R = case
    N, H = 4, 8
    x = rnd_bf16((N, H, H, C), 21, dev=dev)
    w = rnd_bf16((Co, R * R, C), 22, 0.1, dev)
    with env(ENV[eng]):
        carrier = F.SignPlane()
        y0 = F.conv2d_raw(x, w.data_ptr(), C, Co, R, R, 1, R // 2, R // 2)
        before = plane_counts()
        with engines(dev) as counts:
            y1 = F.conv2d_raw(x, w.data_ptr(), C, Co, R, R, 1, R // 2, R // 2, out_plane=carrier)
        after = plane_counts()
    assert counts == {eng: 1}, f"{case}: {counts}"
    assert after[0] == before[0] and carrier.bits is None, f"{case}: an engine without the tile epilogue claims to have written a plane"
    assert bits_equal(y1, y0)


# ---- 2. consumers -------------------------------------------------------------------------------------------------------------------------
# (engine, C of dy, C of the masked result, with residual)
CONSUMERS = [(e, c, co, r) for (e, c, co) in (("q", 64, 192), ("q", 32, 64), ("v4", 64, 192), ("v4", 32, 96), ("v3", 64, 192), ("v3", 96, 96), ("v2", 64, 192), ("v2", 48, 64))
             for r in (False, True)]
IGNORERS = [("gemm", 64, 96, False), ("gemm", 64, 96, True), ("sk", 96, 96, False)]


def consumer_case(case, dev):
    """out(mask = a DECOY that lets everything pass, mask_bits = plane of the true mask) == out(mask = the true mask): the engine read the plane, not the tensor.
    An engine that ignores planes is handed the true mask with its plane and must give what it gives without the plane."""
    from studiogan_amd import functional as F, _lib as L
    eng, C, Co, with_res = case
    reads_plane = eng in ("q", "v4", "v3", "v2")
    N, H = (3, 16) if reads_plane else (4, 8)
    quad = eng == "q"
    R = 1 if eng == "sk" else 3
    Hi = H // 2 if quad else H                     # the quad kernel's UP form: dy on the low-resolution grid, mask / residual / result on the fine one
    nw = (Co + 31) // 32
    ldm, ldr, ldo, ldw = Co + 8, Co + 16, Co + 8, nw + 1
    dy = rnd_bf16((N, Hi, Hi, C), 31, dev=dev)
    w = rnd_bf16((Co, 16 if quad else R * R, C), 32, 0.1, dev)
    true = mask_values((N, H, H, Co), 33, dev)
    assert bool((true.float() == 0).any()) and bool((true.view(torch.int16) == 1).any())
    truew = _wide(true, ldm, float("nan"))
    decoy = torch.full_like(truew, 1.0)
    bits = torch.full((N, H, H, ldw), SENT, dtype=torch.int32, device=dev)
    bits[..., :nw] = pack_plane(true).to(dev)
    res = _wide(rnd_bf16((N, H, H, Co), 34, dev=dev), ldr, float("nan")) if with_res else None

    def launch(mask, plane):
        out = torch.full((N, H, H, ldo), OUT_SENT, dtype=torch.bfloat16, device=dev)
        if quad:
            d = L.ConvQDesc()
            d.dtype, d.form, d.N, d.Hl, d.Wl, d.C, d.ldx, d.Cout = L.BF16, L.Q_UP, N, Hi, Hi, C, C, Co
            d.pix_flags, d.epi_flags, d.alpha, d.beta = 0, 0, 1.0, 1.0
            d.x, d.wq, d.out, d.ldo = dy.data_ptr(), w.data_ptr(), out.data_ptr(), ldo
            name = "sg_conv2d_q"
        else:
            d = L.ConvFwdDesc()
            F.conv2d_raw(dy, w.data_ptr(), C, Co, R, R, 1, R // 2, R // 2, 0, 0, out=out, desc=d)
            name = "sg_conv2d_fwd"
        d.mask, d.ldm = mask.data_ptr(), ldm
        if res is not None:
            d.res, d.ldr = res.data_ptr(), ldr
        if plane is not None:
            d.mask_bits, d.ldmb = plane.data_ptr(), ldw
            d.epi_flags |= L.EPI_PLANES
        before = plane_counts()
        with engines(dev) as counts:
            L.call(name, d, L.stream())
        after = plane_counts()
        assert counts == {eng: 1}, f"{case}: expected one {eng} launch, the profiler saw {counts}"
        return out, (after[1] - before[1], after[2] - before[2])

    with env(ENV.get(eng, {})):
        ref, c_ref = launch(truew, None)
        got, c_got = launch(decoy if reads_plane else truew, bits)
    assert c_ref == (0, 1), f"{case}: counters of the activation launch {c_ref}"
    assert c_got == ((1, 0) if reads_plane else (0, 1)), f"{case}: counters of the plane launch {c_got}"
    if not with_res:          # (the mask did something: zeros where it is off, values where it is on)
        assert bool((ref[..., :Co].float() == 0).any()) and bool((ref[..., :Co].float() != 0).any())
    assert bits_equal(got, ref), f"{case}: the result with mask_bits differs from the result with mask"


# ---- 3. block level -----------------------------------------------------------------------------------------------------------------------
def block_case(dev):
    """A BigGAN discriminator at 32 x 32, width 96, bf16: DiscOptBlock, self-attention, a down-sampling DiscBlock and two identity-skip DiscBlocks, forward and
    backward, SG_SIGN_PLANE on against off. With conv_v2 / conv_v4 forced (the engines the full-size layers get) the masked data gradients are, in backward order:
      block 4, 3 (identity skip): conv2d2 masks with h (conv_v4 wrote its plane) -> plane; conv2d1 masks with the block input. Block 3's input is the pooled tail of
        block 2 (quad kernel + fused skip, wrote a plane) -> plane; block 4's input comes out of AddRelu, no convolution -> activation.
      block 2 (behind the attention block): conv2d2 masks with h -> plane; the 1x1 skip and conv2d1 mask with the attention block's output -> activation, twice.
      block 1 (DiscOptBlock): conv2d2 masks with h, written by conv_v2 here -> plane.
    = 5 planes and 3 activations with the switch on, 8 activations with it off."""
    from studiogan_amd import ops
    from studiogan_amd.backbones import big_resnet as bb

    class _MODEL:
        info_type = "N/A"

    res = {}
    for on in ("1", "0"):
        with env({"SG_CONV_V4": "force", "SG_CONV_V2": "force", "SG_SIGN_PLANE": on}):
            torch.manual_seed(5)
            MOD = ops.Modules(apply_g_sn=True, apply_d_sn=True, g_cond_mtd="cBN", backbone="big_resnet")
            D = bb.Discriminator(32, 48, True, True, [1], "PD", "W/O", "N/A", False, 10, "ortho", "N/A", True, MOD, _MODEL).to(dev)
            D.train()
            acts = []
            ops.BLOCK_HOOKS[0] = True
            D.__dict__["_sg_teacher"] = lambda bi, a: (acts.append(a), a.retain_grad(), a)[2]
            try:
                g = torch.Generator().manual_seed(6)
                img = torch.randn((3, 3, 32, 32), generator=g).to(dev)      # (no gradient: the discriminator update's path, block 1 runs its fused tail)
                lab = torch.tensor([1, 4, 7], device=dev)
                before = plane_counts()
                out = D(img, lab)
                logits = out["adv_output"] if isinstance(out, dict) else out
                logits.float().sum().backward()
                _sync(dev)
                after = plane_counts()
            finally:
                ops.BLOCK_HOOKS[0] = False
                D.__dict__.pop("_sg_teacher", None)
            grads = {k: p.grad.detach().clone() for k, p in D.named_parameters() if p.grad is not None}
            res[on] = dict(acts=[a.detach().clone() for a in acts], dacts=[a.grad.detach().clone() for a in acts], grads=grads,
                           logits=logits.detach().clone(), counts=tuple(a - b for a, b in zip(after, before)))
    a, b = res["1"], res["0"]
    print("sign-plane launches (written, read, activation) on:", a["counts"], "off:", b["counts"])
    assert b["counts"][0] == 0 and b["counts"][1] == 0, b["counts"]
    assert a["counts"][1] + a["counts"][2] == b["counts"][2], (a["counts"], b["counts"])
    assert a["counts"][1:] == (5, 3), a["counts"]
    assert len(a["acts"]) == 5 and bits_equal(a["logits"], b["logits"])
    for i, (p, q) in enumerate(zip(a["acts"] + a["dacts"], b["acts"] + b["dacts"])):
        assert bits_equal(p, q), f"activation / data gradient {i} differs between SG_SIGN_PLANE=1 and 0"
    assert a["grads"].keys() == b["grads"].keys() and any("conv2d1.weight" in k for k in a["grads"])
    for k in a["grads"]:
        # sums accumulated with float atomics, in whatever order the workgroups arrive: the bias gradients (sg_colsum / the weight-gradient kernels' side sums) and the
        # attention block's scalar output gain `sigma` (sg_dot) -- equal operands, 1e-5 relative; every other parameter gradient is bit-identical
        if k.endswith(".bias") or k.endswith(".sigma"):
            assert torch.allclose(a["grads"][k], b["grads"][k], rtol=0, atol=1e-5 * float(b["grads"][k].abs().max()) + 1e-30), k
        else:
            assert bits_equal(a["grads"][k], b["grads"][k]), k
