"""Checks of the eight elementwise entry points that have a scalar and a 16-byte instantiation of ONE kernel body (csrc/elementwise.hip: sg_avgpool2_fwd / _bwd,
sg_maxpool2_fwd / _bwd, sg_relu_mask, sg_slice_up_fwd / _bwd, sg_copy_channels), written once for both places they run: the GPU (tests/test_ew_gpu.py) and the kernel
sources on the CPU interpreter (tests/test_ew_cpu.py under hipemu.fullemu.Installed).

Bound: none. These operations are copies, selects, maxima and one fixed-order fp32 sum of four rounded once, so the torch restatement on the CPU is exact and every
comparison is torch.equal on the bytes of the WHOLE buffer an output lives in: the region the operation owns against the restatement, everything around it (and, in a
pitched output, the columns behind C) against the sentinel the buffer was filled with.

Which instantiation ran is read from sg_ew_vec_launches(): a bf16 vector-path case moves it by exactly one, a scalar-path case and every fp32 case not at all. Every
vector-path case runs a second time with its first input 8 bytes past a 16-byte boundary, which takes the scalar instantiation, and the two outputs must be the same
bytes."""
import torch

SENT = 0xA5          # the byte every buffer is filled with before a kernel writes into it
PAD = 64             # sentinel bytes in front of and behind every region
IT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
DTYPES = (torch.float32, torch.bfloat16)
POOL = dict(N=2, H=4, W=6)            # non-square: an H / W swap shows; two samples: the batch term shows
SLICE = dict(N=2, Hs=2, Ws=3)


# ---- bits ----------------------------------------------------------------------------------------------------------------------------------------------------------
def bits_of(v, dtype):
    """fp32 values -> the stored representation (one rounding to dtype), as integers"""
    return v.to(dtype).view(IT[dtype])


def vals(bits, dtype):
    return bits.view(dtype).float()


def patterns(pats, dtype):
    return torch.tensor(pats, dtype=torch.int64).to(IT[dtype])


def grad_specials(dtype, snan=True):
    """what a gradient that is only moved must keep: a quiet NaN with a payload, a signalling NaN (a float round trip through f2bf would set its quiet bit), -0,
    +inf, -inf"""
    p = [0x7fc1, 0x8000, 0x7f80, 0xff80] + ([0x7f81] if snan else [])
    return patterns(p if dtype == torch.bfloat16 else [0x7fc00001, 0x80000000, 0x7f800000, 0xff800000] + ([0x7f800001] if snan else []), dtype)


def randn_bits(shape, dtype, seed):
    return bits_of(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)), dtype)


def grad_bits(shape, dtype, seed, snan=True):
    """random normal with eight copies of every special value at seeded places -> (bits, the flat places: place j holds special j % count)"""
    b = randn_bits(shape, dtype, seed)
    sp = grad_specials(dtype, snan).repeat(8)
    assert sp.numel() <= b.numel() // 2
    at = torch.randperm(b.numel(), generator=torch.Generator().manual_seed(seed + 1))[:sp.numel()]
    b.view(-1)[at] = sp
    return b, at


def sentinel(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * IT[dtype].itemsize,), SENT, dtype=torch.uint8).view(IT[dtype]).reshape(shape)


class Buf:
    """a region with the integer content `bits` inside a larger buffer of sentinel bytes on `dev`, `shift` bytes past a 16-byte boundary"""

    def __init__(self, dev, bits, shift=0):
        raw = bits.contiguous().view(-1).view(torch.uint8)
        self.lo, self.hi = PAD + shift, PAD + shift + raw.numel()
        self.host = torch.full((self.hi + PAD,), SENT, dtype=torch.uint8)
        self.host[self.lo:self.hi] = raw
        self.dev = self.host.clone().to(dev)
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self):
        from studiogan_amd import _lib as L
        return L.ptr(self.dev) + self.lo

    def expect(self, bits):
        """the whole buffer as it has to look afterwards: `bits` in the region, the sentinel around it"""
        e = torch.full_like(self.host, SENT)
        e[self.lo:self.hi] = bits.contiguous().view(-1).view(torch.uint8)
        assert e.numel() == self.host.numel()
        return e

    def region(self):
        return self.dev[self.lo:self.hi].cpu()


def _call(name, *args):
    """-> by how much sg_ew_vec_launches() moved (None on a library from before the counter)"""
    from studiogan_amd import _lib as L
    lib = L.lib()
    count = getattr(lib, "sg_ew_vec_launches", None)
    n0 = count() if count else None
    L.call(name, *args, L.stream())
    return None if n0 is None else count() - n0


def _finish(moved, **outs):
    """outs: name -> (Buf, expected bits of its region). Asserts every buffer byte for byte -> (moved, {name: region bytes})"""
    res = {}
    for name, (buf, exp) in outs.items():
        got, want = buf.dev.cpu(), buf.expect(exp)
        assert torch.equal(got[buf.lo:buf.hi], want[buf.lo:buf.hi]), f"{name}: {int((got != want)[buf.lo:buf.hi].sum())} bytes of the result differ from the restatement"
        assert torch.equal(got, want), f"{name}: bytes outside the region were written"
        res[name] = buf.region()
    return moved, res


def _dt(dtype):
    from studiogan_amd import _lib as L
    return L.dt(dtype)


def _windows(v, N, H, W):
    """[N*H*W, C] -> the four pixels of every 2x2 window in row-major window order, each [N, H/2, W/2, C]"""
    v = v.reshape(N, H, W, -1)
    return [v[:, a::2, b::2] for a in (0, 1) for b in (0, 1)]


def _unpool(t):
    """[N, H2, W2, C] -> [N, 2 H2, 2 W2, C], every value at the four pixels of its window"""
    return t.repeat_interleave(2, 1).repeat_interleave(2, 2)


def _pos(N, H, W):
    """[N, H, W, 1]: a pixel's place in its window, 2 (h & 1) + (w & 1)"""
    return (2 * (torch.arange(H) % 2)[:, None] + (torch.arange(W) % 2)[None, :]).expand(N, H, W)[..., None]


# ---- the operations: inputs, launch, exact restatement ---------------------------------------------------------------------------------------------------------------
def avgpool2_fwd(dev, dtype, sh, C, snan=True):
    N, H, W = POOL["N"], POOL["H"], POOL["W"]
    xb = randn_bits((N * H * W, C), dtype, 11)
    x, y = Buf(dev, xb, sh.get("in", 0)), Buf(dev, sentinel((N * H * W // 4, C), dtype), sh.get("out", 0))
    moved = _call("sg_avgpool2_fwd", _dt(dtype), x.ptr(), y.ptr(), N, H, W, C)
    a, b, c, d = _windows(vals(xb, dtype), N, H, W)
    return _finish(moved, y=(y, bits_of(0.25 * (((a + b) + c) + d), dtype)))


def avgpool2_bwd(dev, dtype, sh, C, snan=True):
    N, H, W = POOL["N"], POOL["H"], POOL["W"]
    gb = randn_bits((N, H // 2, W // 2, C), dtype, 12)
    dy, dx = Buf(dev, gb, sh.get("in", 0)), Buf(dev, sentinel((N * H * W, C), dtype), sh.get("out", 0))
    moved = _call("sg_avgpool2_bwd", _dt(dtype), dy.ptr(), dx.ptr(), N, H, W, C)
    return _finish(moved, dx=(dx, _unpool(bits_of(0.25 * vals(gb, dtype), dtype))))


def maxpool2_fwd(dev, dtype, sh, C, ldx, ldy, no_idx=False, snan=True):
    N, H, W = POOL["N"], POOL["H"], POOL["W"]
    xv = torch.randint(-1, 2, (N * H * W, ldx), generator=torch.Generator().manual_seed(13)).float()
    x = Buf(dev, bits_of(xv, dtype), sh.get("in", 0))
    yexp, iexp = sentinel((N * H * W // 4, ldy), dtype), torch.full((N * H * W // 4, C), SENT, dtype=torch.uint8)
    y, idx = Buf(dev, yexp, sh.get("out", 0)), Buf(dev, iexp, sh.get("idx", 0))
    moved = _call("sg_maxpool2_fwd", _dt(dtype), x.ptr(), ldx, y.ptr(), ldy, None if no_idx else idx.ptr(), N, H, W, C)
    v = _windows(xv[:, :C], N, H, W)
    m, a = v[0], torch.zeros_like(v[0], dtype=torch.uint8)
    for k in (1, 2, 3):                                  # the first maximum in row-major window order wins: a later pixel takes over only when strictly larger
        up = v[k] > m
        m, a = torch.where(up, v[k], m), torch.where(up, torch.full_like(a, k), a)
    ties = (torch.stack(v) == m).sum(0) > 1
    assert float(ties.float().mean()) >= 1 / 3, "too few windows tie for the maximum: the tie rule would go unseen"
    yexp, iexp = yexp.clone(), iexp.clone()
    yexp[:, :C] = bits_of(m, dtype).reshape(-1, C)
    if not no_idx:
        iexp[:] = a.reshape(-1, C)
    return _finish(moved, y=(y, yexp), idx=(idx, iexp))


def maxpool2_bwd(dev, dtype, sh, C, ldx, ldy, snan=True):
    N, H, W = POOL["N"], POOL["H"], POOL["W"]
    gb = randn_bits((N * H * W // 4, ldy), dtype, 14)
    gb[:, :C] = grad_bits((N * H * W // 4, C), dtype, 14, snan)[0]      # (every element of dy is kept at exactly one pixel of its window)
    ib = torch.randint(0, 4, (N, H // 2, W // 2, C), generator=torch.Generator().manual_seed(15)).to(torch.uint8)
    dy, idx = Buf(dev, gb, sh.get("in", 0)), Buf(dev, ib, sh.get("idx", 0))
    exp = sentinel((N * H * W, ldx), dtype)
    dx = Buf(dev, exp, sh.get("out", 0))
    moved = _call("sg_maxpool2_bwd", _dt(dtype), dy.ptr(), ldy, idx.ptr(), dx.ptr(), ldx, N, H, W, C)
    g = _unpool(gb[:, :C].reshape(N, H // 2, W // 2, C))
    exp = exp.clone()
    exp[:, :C] = torch.where(_unpool(ib) == _pos(N, H, W), g, torch.zeros_like(g)).reshape(-1, C)      # on the stored bits: no float in between
    for p in grad_specials(dtype, snan):
        assert bool((exp[:, :C] == p).any()), "a special value of dy reaches no kept place"
    return _finish(moved, dx=(dx, exp))


def relu_mask(dev, dtype, sh, n, snan=True):
    gb, at = grad_bits((n,), dtype, 16, snan)
    xb = randn_bits((n,), dtype, 17)
    sp = patterns([0x0000, 0x8000, 0x7fc0, 0x0001] if dtype == torch.bfloat16 else [0x00000000, 0x80000000, 0x7fc00000, 0x00000001], dtype)      # +0, -0, NaN, the smallest positive subnormal
    xb[torch.randperm(n, generator=torch.Generator().manual_seed(18))[:8 * sp.numel()]] = sp.repeat(8)
    odd = (torch.arange(at.numel()) // grad_specials(dtype, snan).numel()) % 2 == 1      # copies 1, 3, 5, 7 of every special are dropped, the others kept
    xb[at[odd]], xb[at[~odd]] = bits_of(torch.tensor(-1.0), dtype), bits_of(torch.tensor(1.0), dtype)
    keep = vals(xb, dtype) > 0
    for p, k in zip(sp, (False, False, False, True)):
        assert bool((xb == p).any()) and bool((keep[xb == p] == k).all()), "x > 0 is false for +0, -0 and NaN, true for a subnormal"
    assert bool((vals(xb, dtype) < 0).any())
    dy, x, dx = Buf(dev, gb, sh.get("in", 0)), Buf(dev, xb), Buf(dev, sentinel((n,), dtype), sh.get("out", 0))
    moved = _call("sg_relu_mask", _dt(dtype), dy.ptr(), x.ptr(), dx.ptr(), n)
    exp = torch.where(keep, gb, torch.zeros_like(gb))
    for p in grad_specials(dtype, snan):
        assert bool((exp == p).any()) and bool((gb[~keep] == p).any()), "a special value of dy is never kept / never dropped"
    return _finish(moved, dx=(dx, exp))


def slice_up_fwd(dev, dtype, sh, C, ldx, up, snan=True):
    N, Hs, Ws = SLICE["N"], SLICE["Hs"], SLICE["Ws"]
    xb = randn_bits((N, Hs, Ws, ldx), dtype, 19)
    x, y = Buf(dev, xb, sh.get("in", 0)), Buf(dev, sentinel((N * Hs * up * Ws * up, C), dtype), sh.get("out", 0))
    moved = _call("sg_slice_up_fwd", _dt(dtype), x.ptr(), y.ptr(), N, Hs, Ws, ldx, C, up)
    return _finish(moved, y=(y, xb[..., :C].repeat_interleave(up, 1).repeat_interleave(up, 2)))


def slice_up_bwd(dev, dtype, sh, C, ldx, up, snan=True):
    N, Hs, Ws = SLICE["N"], SLICE["Hs"], SLICE["Ws"]
    gb = randn_bits((N, Hs * up, Ws * up, C), dtype, 20)
    dy, dx = Buf(dev, gb, sh.get("in", 0)), Buf(dev, sentinel((N * Hs * Ws, ldx), dtype), sh.get("out", 0))
    moved = _call("sg_slice_up_bwd", _dt(dtype), dy.ptr(), dx.ptr(), N, Hs, Ws, ldx, C, up)
    g = vals(gb, dtype)
    acc = torch.zeros(N, Hs, Ws, C)
    for a in range(up):                                  # a outer, b inner, in fp32, one rounding at the end
        for b in range(up):
            acc = acc + g[:, a::up, b::up]
    exp = torch.zeros(N, Hs, Ws, ldx, dtype=IT[dtype])    # the channels the slice dropped, [C, ldx): exactly zero
    exp[..., :C] = bits_of(acc, dtype)
    return _finish(moved, dx=(dx, exp))


def copy_channels(dev, dtype, sh, C, lds, ldd, snan=True):
    rows = 7
    info = torch.iinfo(IT[dtype])
    sb = torch.randint(info.min, info.max + 1, (rows, lds), generator=torch.Generator().manual_seed(21)).to(IT[dtype])      # random bits
    exp = sentinel((rows, ldd), dtype)
    src, dst = Buf(dev, sb, sh.get("in", 0)), Buf(dev, exp, sh.get("out", 0))
    moved = _call("sg_copy_channels", _dt(dtype), src.ptr(), lds, dst.ptr(), ldd, rows, C)
    exp = exp.clone()
    exp[:, :C] = sb[:, :C]                               # the destination's columns at and beyond C keep the sentinel
    return _finish(moved, dst=(dst, exp))


# ---- the case table: (operation, arguments, byte shifts of its pointers, whether bf16 takes the 16-byte instantiation) --------------------------------------------
def _cases():
    out = []
    for op in (avgpool2_fwd, avgpool2_bwd):
        out += [(op, dict(C=8), {}, True), (op, dict(C=24), {}, True), (op, dict(C=12), {}, False), (op, dict(C=24), {"out": 8}, False)]
    for op in (maxpool2_fwd, maxpool2_bwd):
        for C in (8, 24):
            for dx, dy in ((0, 0), (8, 16)):
                out.append((op, dict(C=C, ldx=C + dx, ldy=C + dy), {}, True))
                if op is maxpool2_fwd:
                    out.append((op, dict(C=C, ldx=C + dx, ldy=C + dy, no_idx=True), {}, True))
        out += [(op, dict(C=12, ldx=12, ldy=12), {}, False), (op, dict(C=8, ldx=12, ldy=8), {}, False), (op, dict(C=8, ldx=8, ldy=12), {}, False),
                (op, dict(C=8, ldx=8, ldy=8), {"idx": 4}, False)]
    out += [(relu_mask, dict(n=8 * 37), {}, True), (relu_mask, dict(n=8 * 37 + 3), {}, False), (relu_mask, dict(n=8 * 37), {"out": 8}, False)]
    for op in (slice_up_fwd, slice_up_bwd):
        for up in (1, 2):
            out += [(op, dict(C=C, ldx=ldx, up=up), {}, vec) for C, ldx, vec in ((8, 8, True), (8, 24, True), (24, 40, True), (12, 16, False), (8, 12, False))]
    out += [(copy_channels, dict(C=C, lds=lds, ldd=ldd), {}, vec) for C, lds, ldd, vec in ((8, 8, 24, True), (24, 40, 24, True), (8, 12, 24, False), (12, 16, 16, False))]
    return out


CASES = _cases()


def case_id(case):
    op, spec, sh, vec = case
    return " ".join([op.__name__] + [f"{k}={v}" for k, v in spec.items()] + [f"{k}+{v}B" for k, v in sh.items()] + ["vec" if vec else "scalar"])


def run_case(case, dev, dtype):
    """one row of the table in one dtype: the restatement byte for byte, the sentinel untouched, the counter; a vector-path row a second time on the scalar
    instantiation (first input 8 bytes off), same bytes"""
    op, spec, sh, vec = case
    moved, res = op(dev, dtype, sh, **spec)
    assert moved == (1 if vec and dtype == torch.bfloat16 else 0), f"sg_ew_vec_launches moved by {moved}"
    if vec:
        moved2, res2 = op(dev, dtype, {"in": 8}, **spec)
        assert moved2 == 0, f"the misaligned run moved sg_ew_vec_launches by {moved2}"
        for k in res:
            assert torch.equal(res[k], res2[k]), f"{k}: the two instantiations wrote different bytes"
