"""Shared checks of the "bf16x6" fp32 mode (csrc/gemm_core.h SPLIT == 6: every fp32 operand element as three bf16 terms whose sum is the element exactly, six
bf16 MFMAs per 16-wide k-tile). One body for the GPU (tests/test_f32x6_gpu.py) and for the CPU interpreter (tests/test_f32x6_cpu.py): `d` is the device the
tensors live on, `sync` what makes a launch's result readable. Every runner returns errors and leaves the assertions on bounds to its caller; what it asserts
itself is which arithmetic ran (sg_f32_split_launches) and that the process-wide switch is back at "exact"."""
import torch
import torch.nn.functional as TF

from test_kernels_gpu import rnd, nhwc, nchw


def split3(x):
    """the kernel's split restated in torch: each term the round-to-nearest-even bf16 of the fp32 remainder before it"""
    h = x.to(torch.bfloat16).float()
    r = x - h
    m = r.to(torch.bfloat16).float()
    lo = (r - m).to(torch.bfloat16).float()
    return h, m, lo


def full_significand(shape, seed, emin, emax):
    """seeded fp32 values with |x| in [2^emin, 2^emax), random sign, all 24 significand bits in use (the lowest one is set)"""
    g = torch.Generator().manual_seed(seed)
    mant = (torch.randint(1 << 23, 1 << 24, shape, generator=g) | 1).float()
    e = torch.randint(emin, emax, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return torch.ldexp(sign * mant, e - 23)


class split_launches:
    """the block's launches: `want` of them on the split path of `mode` (None: not checked), none on the other split mode's; the switch reads 0 afterwards"""

    def __init__(self, L, mode, want=1):
        self.L, self.mode, self.want = L, mode, want

    def counts(self):
        lib = self.L.lib()
        return int(lib.sg_f32_split_launches(3)), int(lib.sg_f32_split_launches(6))

    def __enter__(self):
        self.before = self.counts()
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        d3, d6 = (a - b for a, b in zip(self.counts(), self.before))
        assert self.L.lib().sg_get_f32_mode() == 0
        if self.want is not None:
            want = {"exact": (0, 0), "bf16x3": (self.want, 0), "bf16x6": (0, self.want)}[self.mode]
            assert (d3, d6) == want, f"mode {self.mode}: split launches (bf16x3, bf16x6) = {(d3, d6)}, expected {want}"
        return False


def max_err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def l2_err(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


def conv_fwd(d, case, mode, sync, metric=max_err):
    """fp32 forward convolution (bias + ReLU epilogue) in `mode` against F.conv2d in fp64, on the inputs of test_kernels_gpu.f32_split_case"""
    from studiogan_amd import functional as F, _lib as L
    N, Cin, Cout, H, W, R, S, stride, (ph, pw) = case
    x = rnd((N, Cin, H, W), torch.float32, 21)
    w = rnd((Cout, Cin, R, S), torch.float32, 22, 0.2)
    bias = rnd((Cout,), torch.float32, 23)
    yref = torch.relu(TF.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=(ph, pw)))
    w_fwd = w.permute(0, 2, 3, 1).contiguous().to(d)
    xd, bd = nhwc(x).to(d), bias.to(d)
    with split_launches(L, mode), F.f32_mode(mode):
        y = F.conv2d_raw(xd, w_fwd.data_ptr(), Cin, Cout, R, S, stride, ph, pw, 0, L.EPI_RELU, bias=bd)
    sync()
    return metric(nchw(y.cpu()), yref)


def wgrad_plan(d, x, dy, Cin, Cout, R, S, Ho, Wo, stride, ph, pw):
    """(splits, work_floats) sg_conv2d_wgrad_plan gives for the launch F.conv2d_wgrad_raw makes of these operands"""
    from studiogan_amd import _lib as L
    ds = L.ConvWgradDesc()
    ds.dtype, ds.N = L.F32, x.shape[0]
    ds.xHs, ds.xWs, ds.C, ds.ldx = x.shape[1], x.shape[2], Cin, x.shape[3]
    ds.gHs, ds.gWs, ds.Cout, ds.ldg = dy.shape[1], dy.shape[2], Cout, dy.shape[3]
    ds.Ho, ds.Wo, ds.R, ds.S, ds.stride, ds.pad_h, ds.pad_w = Ho, Wo, R, S, stride, ph, pw
    ds.alpha = 1.0
    ds.x, ds.dy = x.data_ptr(), dy.data_ptr()
    sp, wf = L.C.c_int(0), L.C.c_longlong(0)
    L.call("sg_conv2d_wgrad_plan", ds, L.C.byref(sp), L.C.byref(wf))
    return sp.value, wf.value


def wgrad_tile(I, J):
    """ASSUMED tile of the generic engine for a weight gradient of I = R*S*Cin rows and J = Cout columns: a copy of csrc/conv_wgrad.hip wgrad_plan's rule, not
    something read back from the library -- the C ABI reports a plan's split count, not its tile. It says which template instance a case is MEANT to reach; if
    the rule in C changes, this copy has to follow."""
    if I <= 32:
        return (32, 256)
    if J <= 32:
        return (256, 32)
    if J % 128 != 0 and (J % 96 == 0 or 64 < J < 128):
        return (256, 96)
    return (128, 128)


def conv_wgrad(d, case, mode, sync, metric=max_err):
    """fp32 weight gradient in `mode` against autograd in fp64 (inputs of test_kernels_gpu.f32_split_wgrad_case). Returns (error, splits of the plan)."""
    from studiogan_amd import functional as F, _lib as L
    N, Cin, Cout, H, W, R, S, stride, (ph, pw) = case
    x = rnd((N, Cin, H, W), torch.float32, 31)
    w = rnd((Cout, Cin, R, S), torch.float32, 32, 0.2).double().requires_grad_(True)
    y = TF.conv2d(x.double(), w, None, stride=stride, padding=(ph, pw))
    gy = rnd(tuple(y.shape), torch.float32, 33)
    y.backward(gy.double())
    xd, gyd = nhwc(x).to(d), nhwc(gy).to(d)
    Ho, Wo = y.shape[2], y.shape[3]
    splits, work = wgrad_plan(d, xd, gyd, Cin, Cout, R, S, Ho, Wo, stride, ph, pw)
    assert work == (splits * Cout * R * S * Cin if splits > 1 else 0)
    dw = torch.zeros((Cout, R, S, Cin), dtype=torch.float32, device=d)
    with split_launches(L, mode), F.f32_mode(mode):
        F.conv2d_wgrad_raw(xd, gyd, dw.data_ptr(), Cin, Cout, R, S, Ho, Wo, stride, ph, pw)
    sync()
    return metric(dw.cpu().permute(0, 3, 1, 2), w.grad), splits


def gemm_vector_ok(form, rows, K):
    """does an operand of gemm() below take the all-vector loaders (csrc/gemm.hip gemm_t)? Its pitch and batch stride are multiples of 4 whenever this holds."""
    return (K if form == 0 else rows) % 4 == 0


def gemm(d, I, J, K, pf, qf, mode, sync, batch=1, bias=False, res_beta=None, alpha=1.0, alpha_ptr=None, splits=1, misalign=False):
    """OUT[b][j][i] = beta * res + alpha * alpha_ptr * sum_k P(i,k) Q(j,k) + bias[i] through sg_gemm in `mode`: relative L2 error against fp64.
    misalign: P starts 4 bytes past a 16-byte boundary (the all-vector path declines it: exact MFMA whatever the mode)."""
    from studiogan_amd import functional as F, _lib as L
    P = rnd((batch, I, K) if pf == 0 else (batch, K, I), torch.float32, 41)
    Q = rnd((batch, J, K) if qf == 0 else (batch, K, J), torch.float32, 42)
    b = rnd((I,), torch.float32, 43) if bias else None
    r = rnd((batch, J, I), torch.float32, 44) if res_beta is not None else None
    ap = torch.tensor([alpha_ptr], dtype=torch.float32) if alpha_ptr is not None else None
    Pm = P.double() if pf == 0 else P.double().transpose(1, 2)
    Qm = Q.double() if qf == 0 else Q.double().transpose(1, 2)
    a = torch.tensor(alpha, dtype=torch.float32)
    if ap is not None:
        a = a * ap[0]                                   # the kernel's own fp32 product of the two scales
    ref = torch.einsum("bik,bjk->bji", Pm, Qm) * a.double()
    if bias:
        ref = ref + b.double()
    if r is not None:
        ref = ref + float(torch.tensor(res_beta, dtype=torch.float32)) * r.double()
    if misalign:
        buf = torch.zeros(P.numel() + 4, dtype=torch.float32, device=d)
        buf[1:1 + P.numel()] = P.reshape(-1).to(d)
        p_arg = buf.data_ptr() + 4
        assert p_arg % 16 == 4
    else:
        buf = P.to(d)
        p_arg = buf.data_ptr()
    Qd = Q.to(d)
    out = torch.zeros((batch, J, I), dtype=torch.float32, device=d)
    bd, rd, apd = (None if t is None else t.to(d) for t in (b, r, ap))
    on_split = mode == "bf16x6" and not misalign and gemm_vector_ok(pf, I, K) and gemm_vector_ok(qf, J, K)
    flags = L.EPI_OUT_F32 | (L.EPI_ATOMIC if splits > 1 else 0)
    with split_launches(L, mode if on_split else "exact"), F.f32_mode(mode):
        F.gemm_raw(L.F32, p_arg, pf, P.shape[2], Qd.data_ptr(), qf, Q.shape[2], out.data_ptr(), I, I, J, K, batch=batch, p_bs=P.shape[1] * P.shape[2],
                   q_bs=Q.shape[1] * Q.shape[2], out_bs=J * I, bias=None if bd is None else bd.data_ptr(), res=None if rd is None else rd.data_ptr(),
                   res_bs=J * I, ldr=I if rd is not None else 0, beta=1.0 if res_beta is None else res_beta, alpha=alpha, alpha_ptr=apd,
                   epi_flags=flags, splits=splits)
    sync()
    return l2_err(out.cpu(), ref)
