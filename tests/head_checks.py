"""Checks of the small reductions that turn discriminator outputs into a scalar loss and its first gradient (csrc/heads.hip, csrc/ext/losses.hip, the
"discriminator head", "adversarial losses", "WGAN-GP pieces" and "LeCam" sections of csrc/elementwise.hip, sg_softmax_rows_bwd2 of csrc/ext/second_order.hip),
written once for both places they run: the GPU (tests/test_head_kernels_gpu.py) and the kernel sources on the CPU interpreter (tests/test_head_kernels_cpu.py
under hipemu.fullemu.Installed). One table of cases (CASES), one runner per entry point; a runner takes a torch.device and its case's shape / kind and returns
(launch, check): launch() runs the kernels once into guarded buffers and returns what they wrote, check(outputs) holds it against the restatement.

Reference: a plain torch restatement of the operation in fp64, autograd for every gradient the kernel returns analytically. Inputs are drawn in fp32 and
widened, so both sides see the same numbers; float arguments (eps, temperature, m_p, the LeCam anchors) are the fp32 values the C ABI receives.

Bound: every comparison is err = max|a - b| / max|b| against the fp64 restatement, held to 4 x the err of THE SAME restatement evaluated by torch in fp32 on
the CPU (computed here, per comparison), with a floor of 1e-6 (about 16 fp32 ulp: __expf and reciprocal-multiply forms that differ from torch's by a few ulp
per element, a tree reduction against a strided one over at most 1024 terms) and a cap of 1e-5 (what test_head_losses_embedding already holds these kernels
to). A scalar loss is judged relative to the mean over rows of the absolute per-row terms instead of to the loss itself (a Wasserstein loss cancels to ~0);
where that mean is exactly 0 (a batch that sits on its kinks) the loss must be exactly 0. A row_loss output is a vector like any other: max|b|.
Three results are 0 by algebra, where the fp64 restatement returns only its own rounding of 0 and neither scale means anything. Each is named in its runner:
normalize's dx at cols == 1 (y = +-1; judged by the addends that cancel, |inv * dy|); the D2D-CE row_loss and loss of a batch with a single class
(pos + log(exp(-pos) + 0); judged by |pos| + |log(...)|); and the contrastive dS / dp of such a batch in both kinds with the 2C row_loss and loss
(log(1 + 0 / num)), where the kernels sum nothing, so exact zeros are required and the restatement is not asked. bf16 entries are
compared with the restatement of the bf16-rounded inputs; an output STORED as bf16 gets one bf16 rounding (2^-8 relative) on top of its bound.

Exact, not bounded: zero rows and zero subgradients (wherever the fp64 restatement of a gradient is exactly 0 the kernel's must be exactly 0: the inputs sit
on grids so the kinks r == 1, f == -1, real == ema_fake, s_ij == 0, p == m_p, equal column means and tied maxima occur exactly, in fp32 and fp64 alike),
gather / scatter, interp at alpha 0 / 1, and where NaN goes. Every restatement also returns its sign / mask / arg-max decisions, and the fp32 and the fp64
evaluation must agree on all of them, so no element ever has to be left out for sitting near a kink.

Guards: every output lives in an ew_checks.Buf with 64 sentinel bytes in front and behind, untouched afterwards. Determinism: the kernels claim a fixed
reduction order, so every case launches twice and the two results must be the same bits. One line per comparison is printed: err, the fp32 restatement's
err, the bound."""
import zlib

import torch
import torch.nn.functional as TF

import ew_checks as EC

FLOOR, CAP = 1e-6, 1e-5
BF16_STORE = 2.0 ** -8
WRAP = 4096 * 256 + 3                 # = 7 * 149797: one element more than the capped grids (4096 blocks of 256) cover in a pass, so the grid-stride loop wraps
WRAP_ROWS, WRAP_COLS = 7, 149797
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16

# ABI name -> (index of its kind / dtype / accumulate argument, the values the table has to reach), or None
ENTRY_POINTS = {
    "sg_row_normalize_fwd": None, "sg_row_normalize_bwd": None, "sg_row_dot": None, "sg_row_scale": (5, {0, 1}), "sg_softmax_rows_bwd2": None,
    "sg_class_loss": (0, {0, 1}), "sg_contrastive_loss": (0, {0, 1}), "sg_gather_cols": None, "sg_scatter_cols": None,
    "sg_loss_d": (0, {0, 1, 2}), "sg_loss_g": (0, {0, 1, 2}), "sg_loss_ls_d": None, "sg_loss_ls_g": None, "sg_lecam": None, "sg_fm_loss": None,
    "sg_exp_fwd": None, "sg_exp_bwd": None, "sg_normal_nll": None, "sg_gp_fwd": (0, {0, 1, 2}), "sg_gp_bwd": (0, {0, 1, 2}), "sg_interp_rows": None,
    "sg_relu_sum_hw_fwd": (0, {0, 1}), "sg_relu_sum_hw_bwd": (0, {0, 1}), "sg_masked_sum_hw": (0, {0, 1}), "sg_pd_head_fwd": None,
}


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------------------------------
def _L():
    from studiogan_amd import _lib
    return _lib


def _call(name, *args):
    L = _L()
    L.call(name, *args, L.stream())


def _p(t):
    return _L().ptr(t)


def _f32(v):
    """the value a float argument has once the C ABI has taken it"""
    return float(torch.tensor(v, dtype=F32))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _grid(shape, g, lim=48):
    """logits on a 1/8 grid in [-lim/8, lim/8]"""
    return torch.randint(-lim, lim + 1, shape, generator=g).float() / 8


class Out:
    """an output region of `shape` inside sentinel bytes on `dev`; `init`: the values it holds before the launch (default: the sentinel)"""

    def __init__(self, dev, shape, dtype=F32, init=None):
        self.shape, self.dtype = tuple(shape), dtype
        self.buf = EC.Buf(dev, EC.sentinel(self.shape, dtype) if init is None else EC.bits_of(init.reshape(self.shape), dtype))

    def ptr(self):
        return self.buf.ptr()

    def read(self):
        b = self.buf
        raw = b.dev.cpu()
        assert bool((raw[:b.lo] == EC.SENT).all()) and bool((raw[b.hi:] == EC.SENT).all()), "bytes outside the output were written"
        return raw[b.lo:b.hi].clone().view(self.dtype).reshape(self.shape)


def untouched(t):
    """True where an fp32 output still holds the sentinel"""
    return t.contiguous().view(torch.int32) == EC.sentinel((1,), F32)[0]


def twice(launch):
    a, b = launch(), launch()
    for k in a:
        assert torch.equal(a[k].view(EC.IT[a[k].dtype]), b[k].view(EC.IT[b[k].dtype])), f"{k}: two launches on the same input wrote different bits"
    return a


def same(tag, got, want):
    """equal values, NaN in the same places (+0 and -0 are one value)"""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    ok = got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    print(f"  {tag}: exact, {'equal' if ok else 'DIFFERS'}")
    assert ok, f"{tag}: not exactly the restatement ({int((~torch.isfinite(got)).sum())} non-finite values of {got.numel()})"


def close(tag, got, r64, r32, scale=None, extra=0.0):
    if r64.numel() == 0:
        return
    got, r64, r32 = got.double().reshape(-1), r64.double().reshape(-1), r32.double().reshape(-1)
    assert got.shape == r64.shape, f"{tag}: shape"
    den = float(r64.abs().max()) if scale is None else float(scale)
    if den == 0.0:
        return same(tag, got, r64)
    err, err32 = float((got - r64).abs().max()) / den, float((r32 - r64).abs().max()) / den
    bound = min(max(4 * err32, FLOOR), CAP) + extra
    print(f"  {tag}: err {err:.3e} fp32-restatement err {err32:.3e} bound {bound:.3e}")
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite values"
    assert err <= bound, f"{tag}: err {err:.3e} above {bound:.3e} (fp32 restatement: {err32:.3e})"
    if scale is None:
        assert bool((got[r64 == 0] == 0).all()), f"{tag}: non-zero where the restatement is exactly zero"


def verify(got, ref, exact=(), extra=None):
    """got: name -> tensor; ref(dtype) -> the same names (+ "_scale": name -> the scale a scalar loss is judged by, "_dec": name -> a decision tensor)"""
    r64, r32 = ref(F64), ref(F32)
    d64, d32 = r64.pop("_dec", {}), r32.pop("_dec", {})
    for k in d64:
        assert torch.equal(d64[k], d32[k]), f"the fp32 and the fp64 restatement disagree on the decision '{k}'"
    scale = r64.pop("_scale", {})
    r32.pop("_scale", None)
    assert set(got) == set(r64), (sorted(got), sorted(r64))
    for k in got:
        if k in exact:
            same(k, got[k], r64[k])
        else:
            close(k, got[k], r64[k], r32[k], scale.get(k), (extra or {}).get(k, 0.0))


def _split(d, name, mask, a, b):
    v = d.pop(name)
    d[f"{name} [{a}]"], d[f"{name} [{b}]"] = v[~mask], v[mask]


# ---- csrc/heads.hip: rows of [rows, cols], one wave per row ------------------------------------------------------------------------------------------------------------
def row_normalize(dev, rows, cols, eps):
    """sg_row_normalize_fwd + _bwd: torch.nn.functional.normalize(dim=1) and autograd through it. rows >= 3: row 1 is all zero and row 2 has norm 1e-14, both below
    eps: the clamped branch (y = x / eps, dx = dy / eps) that the sign of inv encodes; they are compared apart from the free rows, which 1 / eps would dwarf"""
    g = _gen("row_normalize", rows, cols)
    x, dy = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    cl = torch.zeros(rows, dtype=torch.bool)
    if rows >= 3:
        x[1] = 0
        x[2] = x[2] / x[2].norm() * 1e-14
        cl[1] = cl[2] = True
    e = _f32(eps)
    xd, dyd = x.to(dev), dy.to(dev)

    def launch():
        y, inv, dx = Out(dev, (rows, cols)), Out(dev, (rows,)), Out(dev, (rows, cols))
        _call("sg_row_normalize_fwd", _p(xd), y.ptr(), inv.ptr(), rows, cols, e)
        _call("sg_row_normalize_bwd", y.ptr(), inv.ptr(), _p(dyd), dx.ptr(), rows, cols)
        return dict(y=y.read(), inv=inv.read(), dx=dx.read())

    def ref(dt):
        xx = x.to(dt).requires_grad_()
        y = TF.normalize(xx, dim=1, eps=e)
        y.backward(dy.to(dt))
        nrm = xx.detach().norm(dim=1)
        small = nrm < e
        assert torch.equal(small, cl)
        r = dict(y=y.detach(), inv=torch.where(small, -1.0, 1.0).to(dt) / nrm.clamp_min(e), dx=xx.grad, _dec=dict(clamped=small))
        for k in ("y", "inv", "dx"):
            _split(r, k, cl, "free", "clamped")
        if cols == 1 and not bool(cl.all()):             # y = +-1: dx = inv * (dy - y <y, dy>) is identically 0 and the restatement returns its own rounding, so the
            r["_scale"] = {"dx [free]": float((dy.to(dt)[~cl, 0] / nrm[~cl]).abs().max())}      # error is taken relative to the two addends that cancel, |inv * dy|
        return r

    def check(o):
        o = dict(o)
        for k in ("y", "inv", "dx"):
            _split(o, k, cl, "free", "clamped")
        verify(o, ref)
    return launch, check


def row_dot(dev, rows, cols):
    g = _gen("row_dot", rows, cols)
    a, b = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    ad, bd = a.to(dev), b.to(dev)

    def launch():
        p = Out(dev, (rows,))
        _call("sg_row_dot", _p(ad), _p(bd), p.ptr(), rows, cols)
        return dict(p=p.read())
    return launch, lambda o: verify(o, lambda dt: dict(p=(a.to(dt) * b.to(dt)).sum(1)))


def row_scale(dev, rows, cols, acc):
    """out = (acc ? out : 0) + g[r] * x"""
    gen = _gen("row_scale", rows, cols)
    g, x, o0 = torch.randn(rows, generator=gen), torch.randn(rows, cols, generator=gen), torch.randn(rows, cols, generator=gen)
    gd, xd = g.to(dev), x.to(dev)

    def launch():
        out = Out(dev, (rows, cols), init=o0 if acc else None)
        _call("sg_row_scale", _p(gd), _p(xd), out.ptr(), rows, cols, acc)
        return dict(out=out.read())
    return launch, lambda o: verify(o, lambda dt: dict(out=(o0.to(dt) if acc else 0) + g.to(dt)[:, None] * x.to(dt)))


def softmax_rows_bwd2(dev, rows, cols):
    """the derivative of sg_softmax_rows_bwd's dS = P * (dP - <P, dP>) with respect to P, contracted with u: autograd of exactly that"""
    g = _gen("softmax_rows_bwd2", rows, cols)
    P, dP, u = torch.softmax(torch.randn(rows, cols, generator=g), 1), torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    Pd, dPd, ud = P.to(dev), dP.to(dev), u.to(dev)

    def launch():
        gP = Out(dev, (rows, cols))
        _call("sg_softmax_rows_bwd2", _p(Pd), _p(dPd), _p(ud), gP.ptr(), rows, cols)
        return dict(gP=gP.read())

    def ref(dt):
        p, d = P.to(dt).requires_grad_(), dP.to(dt)
        dS = p * (d - (p * d).sum(1, keepdim=True))
        (dS * u.to(dt)).sum().backward()
        return dict(gP=p.grad)
    return launch, lambda o: verify(o, ref)


def _class_launch(dev, kind, z, label):
    rows, cols = z.shape
    zd, ld = z.to(dev), label.to(dev)

    def launch():
        rl, loss, dz = Out(dev, (rows,)), Out(dev, (1,)), Out(dev, (rows, cols))
        _call("sg_class_loss", kind, _p(zd), _p(ld), rows, cols, rl.ptr(), loss.ptr(), dz.ptr())
        return dict(row_loss=rl.read(), loss=loss.read(), dz=dz.read())
    return launch


def _class_ref(kind, z, label, good, dt):
    """rows in `good` only, still divided by ALL rows (what the kernels' 1 / rows does to the rows a poisoned batch leaves intact)"""
    rows = z.shape[0]
    zz = z.to(dt).requires_grad_()
    zg, lg = zz[good], label[good]
    zt = zg.gather(1, lg[:, None])[:, 0]
    if kind == 0:
        lse = torch.logsumexp(zg, 1)
        rl, dec = lse - zt, {}
    else:                                                # Crammer-Singer: torch.max over the row without its label column returns the LOWEST index among equals,
        m, arg = zg.masked_fill(TF.one_hot(lg, z.shape[1]).bool(), float("-inf")).max(1)      # and its backward puts the gradient on that index
        rl = torch.relu(1 + m - zt)
        dec = dict(hinge_on=(1 + m - zt).detach() > 0, arg=arg)
    loss = rl.sum() / rows
    loss.backward()
    return dict(row_loss=rl.detach(), loss=loss.detach().reshape(1), dz=zz.grad[good], _dec=dec, _scale=dict(loss=float(rl.detach().abs().sum()) / rows))


CS_MODES = ("label first", "label last", "label on the maximum", "hinge exactly 0")


def _cs_inputs(rows, cols, phase):
    """integer logits in [-3, 3]: from 63 columns on several wrong classes tie for the maximum, in different lanes and (cols > 64) in the same lane. Row r takes mode
    (r + phase) % 4: the label at column 0, at the last column, on the row's overall arg-max (so the wrong maximum is the runner-up), and a row whose label's logit
    is exactly 1 above the wrong maximum (hinge 0, zero subgradient)"""
    g = _gen("crammer_singer", rows, cols)
    z = torch.randint(-3, 4, (rows, cols), generator=g).float()
    label = torch.zeros(rows, dtype=torch.int64)
    for r in range(rows):
        mode = (r + phase) % 4
        label[r] = (0, cols - 1, int(z[r].argmax()), (r * 7 + 3) % cols)[mode]
        if mode == 3:
            t = int(label[r])
            z[r, t] = torch.cat([z[r, :t], z[r, t + 1:]]).max() + 1
    if cols >= 63:
        zm = z.masked_fill(TF.one_hot(label, cols).bool(), float("-inf"))
        assert bool(((zm == zm.max(1, keepdim=True).values).sum(1) > 1).any()), "no row ties for the wrong maximum: the tie rule would go unseen"
    return z, label


def class_loss(dev, kind, rows, cols, big=False):
    """sg_class_loss: cross entropy (kind 0; big: logits of size +-80, the max subtraction) and Crammer-Singer (kind 1)"""
    parts = []
    if kind == 0:
        g = _gen("xent", rows, cols, big)
        z = torch.randn(rows, cols, generator=g) * 3
        if big:
            z = z + 80 * (torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1)
        label = torch.randint(0, cols, (rows,), generator=g)
        label[0], label[rows - 1] = cols - 1, 0
        parts.append((z, label))
    else:
        parts += [_cs_inputs(rows, cols, ph) for ph in (range(4) if rows < 4 else (0,))]      # fewer than four rows: once per phase, so every row mode is seen
    launches = [_class_launch(dev, kind, z, l) for z, l in parts]

    def launch():
        return {f"{k}{i}": v for i, la in enumerate(launches) for k, v in la().items()}

    def check(o):
        for i, (z, l) in enumerate(parts):
            if kind == 1 and len(parts) > 1:
                print(f"  -- row 0: {CS_MODES[i % 4]}")
            verify({k: o[f"{k}{i}"] for k in ("row_loss", "loss", "dz")}, lambda dt: _class_ref(kind, z, l, torch.ones(rows, dtype=torch.bool), dt))
    return launch, check


def class_loss_bad_label(dev, kind, rows, cols):
    """labels -1 and `cols` (an ADC label against a C-wide head): the loss and those rows of row_loss / dz are NaN, nothing is read out of bounds, and every other
    row is what the remaining rows give under the same 1 / rows"""
    g = _gen("bad_label", kind, rows, cols)
    z = torch.randn(rows, cols, generator=g) * 3 if kind == 0 else torch.randint(-3, 4, (rows, cols), generator=g).float()
    label = torch.randint(0, cols, (rows,), generator=g)
    label[0], label[rows - 1] = -1, cols
    good = (label >= 0) & (label < cols)
    assert bool(good.any())
    launch = _class_launch(dev, kind, z, label)

    def check(o):
        for k, v in (("loss", o["loss"]), ("row_loss [bad labels]", o["row_loss"][~good]), ("dz [bad labels]", o["dz"][~good])):
            same(k, v, torch.full_like(v, float("nan")))
        verify({"row_loss": o["row_loss"][good], "dz": o["dz"][good]},
               lambda dt: {k: v for k, v in _class_ref(kind, z, label, good, dt).items() if k in ("row_loss", "dz", "_dec", "_scale")})
    return launch, check


def contrastive(dev, kind, B, classes, T, m_p=0.98, zeros=False):
    """sg_contrastive_loss: kind 0 the conditional contrastive loss (2C), kind 1 data-to-data cross entropy (D2D-CE), restated from the reference's
    utils/losses.py:50-165 -- diagonal removed, same-label mask, detached row maximum. classes: labels drawn from 2 or 3 classes, "B" = all different (no
    positives), "one" = all the same (kind 1: q == 0). S and p are cosines; p[0] == m_p exactly and p[1] = 1 lies above it; zeros: a quarter of S is exactly 0,
    which with m_p == 1 makes s_ij == 0 exactly (the ReLU's zero subgradient)"""
    g = _gen("contrastive", kind, B, classes)
    E, Q = TF.normalize(torch.randn(B, 4, generator=g), dim=1), TF.normalize(torch.randn(B, 4, generator=g), dim=1)
    S, p = (E @ E.t()).clamp(-1, 1), (E * Q).sum(1).clamp(-1, 1)
    T, m_p = _f32(T), _f32(m_p)
    eye = torch.eye(B, dtype=torch.bool)
    if zeros:
        S[(torch.rand(B, B, generator=g) < 0.25) | eye] = 0.0
        assert m_p == 1.0
    p[0] = m_p
    if B > 2:
        p[1] = 1.0
    label = {"one": torch.zeros(B, dtype=torch.int64), "B": torch.randperm(B, generator=g)}.get(classes)
    if label is None:
        label = torch.randint(0, classes, (B,), generator=g)
    Sd, pd, ld = S.to(dev), p.to(dev), label.to(dev)
    samec = label[:, None] == label[None, :]
    one_class = bool(samec.all())

    def launch():
        rl, loss, dS, dp = Out(dev, (B,)), Out(dev, (1,)), Out(dev, (B, B)), Out(dev, (B,))
        _call("sg_contrastive_loss", kind, _p(Sd), _p(pd), _p(ld), B, T, m_p, rl.ptr(), loss.ptr(), dS.ptr(), dp.ptr())
        return dict(row_loss=rl.read(), loss=loss.read(), dS=dS.read(), dp=dp.read())

    def ref(dt):
        SS, pp = S.to(dt).requires_grad_(), p.to(dt).requires_grad_()
        if kind == 0:
            e = torch.exp(SS / T).masked_fill(eye, 0.0)
            a = torch.exp(pp / T)
            num, den = a + (e * samec).sum(1), a + e.sum(1)
            rl, add, dec = -torch.log(num / den), None, {}
        else:
            s = (SS + m_p - 1) / T
            mx = s.masked_fill(eye, float("-inf")).max(1, keepdim=True).values.detach()
            q = (torch.exp(torch.relu(s) - mx) * (~samec & ~eye)).sum(1)
            u = (m_p - pp) / T
            pos = torch.relu(u)
            rep = torch.log(torch.exp(-pos) + q)
            rl, add, dec = pos + rep, pos.abs() + rep.abs(), dict(s_on=s.detach() > 0, s_zero=s.detach() == 0, pull_on=u.detach() > 0)
            if zeros:
                assert bool((dec["s_zero"] & ~eye).any())
            assert bool((u.detach() == 0)[0]) and (B == 2 or m_p == 1.0 or bool(u.detach()[1] < 0))
        loss = rl.mean()
        loss.backward()
        r = dict(row_loss=rl.detach(), loss=loss.detach().reshape(1), dS=SS.grad, dp=pp.grad, _dec=dec, _scale=dict(loss=float(rl.detach().abs().mean())))
        if one_class:
            del r["dS"], r["dp"]
            if kind == 0:
                del r["row_loss"], r["loss"]
            else:                                        # pos + log(exp(-pos) + 0) is 0 by algebra and the restatement returns its own rounding of it: the only
                r["_scale"] = dict(loss=float(add.detach().mean()), row_loss=float(add.detach().max()))      # losses judged by the addends that cancel
        return r

    def check(o):
        o = dict(o)
        if one_class:                                    # no negatives: the loss does not depend on S or p. The kernels give exact zeros (the sum over the
            same("dS [one class]", o.pop("dS"), torch.zeros(B, B))      # negatives is an empty sum in both kinds); the restatement gives its own rounding of 0
            same("dp [one class]", o.pop("dp"), torch.zeros(B))         # there, so it is not asked
            if kind == 0:                                # log(1 + 0 / num): the loss is exactly 0 as well
                same("row_loss [one class]", o.pop("row_loss"), torch.zeros(B))
                same("loss [one class]", o.pop("loss"), torch.zeros(1))
        verify(o, ref)
    return launch, check


def gather_cols(dev, rows, cols, bad):
    """out[r] = z[r][label[r]]; a label outside [0, cols) gives NaN (pinned: what the code does today)"""
    g = _gen("gather", rows, cols)
    z, label = torch.randn(rows, cols, generator=g), torch.randint(0, cols, (rows,), generator=g)
    if bad:
        label[0], label[rows - 1] = cols, -1
    zd, ld = z.to(dev), label.to(dev)

    def launch():
        out = Out(dev, (rows,))
        _call("sg_gather_cols", _p(zd), _p(ld), rows, cols, out.ptr())
        return dict(out=out.read())

    def ref(dt):
        ok = (label >= 0) & (label < cols)
        v = z.to(dt).gather(1, label.clamp(0, cols - 1)[:, None])[:, 0]
        return dict(out=torch.where(ok, v, torch.full_like(v, float("nan"))))
    return launch, lambda o: verify(o, ref, exact=("out",))


def scatter_cols(dev, rows, cols, bad):
    """dz[r][c] = (c == label[r]) * g[r]; a label outside [0, cols) leaves its row all zero (pinned: what the code does today)"""
    gen = _gen("scatter", rows, cols)
    g, label = torch.randn(rows, generator=gen), torch.randint(0, cols, (rows,), generator=gen)
    if bad:
        label[0], label[rows - 1] = cols, -1
    gd, ld = g.to(dev), label.to(dev)

    def launch():
        dz = Out(dev, (rows, cols))
        _call("sg_scatter_cols", _p(gd), _p(ld), rows, cols, dz.ptr())
        return dict(dz=dz.read())
    return launch, lambda o: verify(o, lambda dt: dict(dz=(torch.arange(cols)[None, :] == label[:, None]).to(dt) * g.to(dt)[:, None]), exact=("dz",))


# ---- adversarial losses, LeCam: one 256-thread block per call ---------------------------------------------------------------------------------------------------------
BEYOND = (20.0, 20.125, -20.125, 25.0, -25.0, 30.0, -30.0, -20.0)      # either side of softplusf's switch at 20, and the saturated sigmoid


def _logits(name, kind, B):
    """real / fake logits on the 1/8 grid in [-6, 6] with the hinge kinks r == 1 and f == -1 at element 0; vanilla (kind 2) from 19 on also beyond +-20"""
    g = _gen(name, kind, B)
    r, f = _grid((B,), g), _grid((B,), g)
    r[0], f[0] = 1.0, -1.0
    if kind == 2 and B >= 19:
        r[2:2 + len(BEYOND)] = torch.tensor(BEYOND)
        f[3:3 + len(BEYOND)] = torch.tensor(BEYOND)
    return r, f


def _pair_loss(dev, abi, lead, B, r, f, rows):
    """a loss over real and fake logits: launch of `abi`(*lead, real, fake, B, ...) and its restatement from rows(r, f) -> (row terms, decisions)"""
    rd, fd = r.to(dev), f.to(dev)

    def launch():
        loss, dr, df = Out(dev, (1,)), Out(dev, (B,)), Out(dev, (B,))
        _call(abi, *lead[0], _p(rd), _p(fd), B, *lead[1], loss.ptr(), dr.ptr(), df.ptr())
        return dict(loss=loss.read(), d_real=dr.read(), d_fake=df.read())

    def ref(dt):
        rr, ff = r.to(dt).requires_grad_(), f.to(dt).requires_grad_()
        term, dec = rows(rr, ff)
        loss = term.mean()
        loss.backward()
        return dict(loss=loss.detach().reshape(1), d_real=rr.grad, d_fake=ff.grad, _scale=dict(loss=float(term.detach().abs().mean())), _dec=dec)
    return launch, lambda o: verify(o, ref)


def loss_d(dev, kind, B):
    """sg_loss_d: 0 hinge, 1 Wasserstein, 2 vanilla = softplus(-r) + softplus(f)"""
    r, f = _logits("loss_d", kind, B)

    def rows(rr, ff):
        if kind == 0:
            t = torch.relu(1 - rr) + torch.relu(1 + ff)
            return t, dict(real_on=(1 - rr).detach() > 0, fake_on=(1 + ff).detach() > 0)
        if kind == 1:
            return ff - rr, {}
        t = TF.softplus(-rr) + TF.softplus(ff)
        return t, {}
    return _pair_loss(dev, "sg_loss_d", ((kind,), ()), B, r, f, rows)


def loss_g(dev, kind, B):
    """sg_loss_g: 0 / 1 -mean(f), 2 softplus(-f)"""
    _, f = _logits("loss_g", kind, B)
    fd = f.to(dev)

    def launch():
        loss, df = Out(dev, (1,)), Out(dev, (B,))
        _call("sg_loss_g", kind, _p(fd), B, loss.ptr(), df.ptr())
        return dict(loss=loss.read(), d_fake=df.read())

    def ref(dt):
        ff = f.to(dt).requires_grad_()
        t = TF.softplus(-ff) if kind == 2 else -ff
        t.mean().backward()
        return dict(loss=t.mean().detach().reshape(1), d_fake=ff.grad, _scale=dict(loss=float(t.detach().abs().mean())))
    return launch, lambda o: verify(o, ref)


def loss_ls_d(dev, B):
    r, f = _logits("loss_ls_d", 0, B)

    def rows(rr, ff):
        t = 0.5 * (rr - 1) ** 2 + 0.5 * ff ** 2
        return t, {}
    return _pair_loss(dev, "sg_loss_ls_d", ((), ()), B, r, f, rows)


def loss_ls_g(dev, B):
    _, f = _logits("loss_ls_g", 0, B)
    f[0] = 1.0
    fd = f.to(dev)

    def launch():
        loss, df = Out(dev, (1,)), Out(dev, (B,))
        _call("sg_loss_ls_g", _p(fd), B, loss.ptr(), df.ptr())
        return dict(loss=loss.read(), d_fake=df.read())

    def ref(dt):
        ff = f.to(dt).requires_grad_()
        t = 0.5 * (ff - 1) ** 2
        t.mean().backward()
        return dict(loss=t.mean().detach().reshape(1), d_fake=ff.grad, _scale=dict(loss=float(t.detach().mean())))
    return launch, lambda o: verify(o, ref)


def lecam(dev, B):
    """mean relu(real - ema_fake)^2 + mean relu(ema_real - fake)^2; the anchors sit on the grid, and element 0 sits exactly on both kinks"""
    ema_real, ema_fake = 0.5, -0.25
    r, f = _logits("lecam", 0, B)
    r[0], f[0] = ema_fake, ema_real

    def rows(rr, ff):
        t = torch.relu(rr - ema_fake) ** 2 + torch.relu(ema_real - ff) ** 2
        return t, dict(real_on=(rr - ema_fake).detach() > 0, fake_on=(ema_real - ff).detach() > 0)
    return _pair_loss(dev, "sg_lecam", ((), (ema_real, ema_fake)), B, r, f, rows)


# ---- csrc/ext/losses.hip ----------------------------------------------------------------------------------------------------------------------------------------------
def fm_loss(dev, B, C):
    """feature matching: mean_c |mean_b fake - mean_b real|. Column C // 2 holds the same grid values in both (rotated by one sample): equal means, sign 0, zero
    gradient"""
    g = _gen("fm", B, C)
    real, fake = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    c0 = C // 2
    fake[:, c0] = _grid((B,), g)
    real[:, c0] = fake[:, c0].roll(1)
    rd, fd = real.to(dev), fake.to(dev)
    parts = (C + 255) // 256

    def launch():
        work, loss, df = Out(dev, (parts,)), Out(dev, (1,)), Out(dev, (B, C))
        _call("sg_fm_loss", _p(rd), _p(fd), B, C, work.ptr(), loss.ptr(), df.ptr())
        work.read()
        return dict(loss=loss.read(), d_fake=df.read())

    def ref(dt):
        rr, ff = real.to(dt), fake.to(dt).requires_grad_()
        diff = ff.mean(0) - rr.mean(0)
        loss = diff.abs().mean()
        loss.backward()
        assert float(diff.detach()[c0]) == 0.0 and bool((ff.grad[:, c0] == 0).all())
        return dict(loss=loss.detach().reshape(1), d_fake=ff.grad, _scale=dict(loss=float(loss.detach())),
                    _dec=dict(sign=torch.sign(diff.detach())))

    def check(o):
        assert _L().lib().sg_fm_work_floats(C) == parts
        verify(o, ref)
    return launch, check


LOG_VAR = (-9.210340371976182, 2.302585092994046)       # variances from 1e-4 to 10


def exp_fwd_bwd(dev, n):
    """sg_exp_fwd + sg_exp_bwd (InfoGAN's variance head): y = exp(x), dx = dy * y"""
    g = _gen("exp", n)
    x = LOG_VAR[0] + (LOG_VAR[1] - LOG_VAR[0]) * torch.rand(n, generator=g)
    dy = torch.randn(n, generator=g)
    xd, dyd = x.to(dev), dy.to(dev)

    def launch():
        y, dx = Out(dev, (n,)), Out(dev, (n,))
        _call("sg_exp_fwd", _p(xd), y.ptr(), n)
        _call("sg_exp_bwd", _p(dyd), y.ptr(), dx.ptr(), n)
        return dict(y=y.read(), dx=dx.read())

    def ref(dt):
        xx = x.to(dt).requires_grad_()
        y = torch.exp(xx)
        y.backward(dy.to(dt))
        return dict(y=y.detach(), dx=xx.grad)
    return launch, lambda o: verify(o, ref)


def normal_nll(dev, B, K):
    """-mean_b sum_k [ -0.5 log(2 pi var + 1e-6) - (x - mu)^2 / (2 var + 1e-6) ], variances log-uniform in [1e-4, 10] with both ends present"""
    g = _gen("nll", B, K)
    x, mu = torch.randn(B, K, generator=g), torch.randn(B, K, generator=g)
    var = torch.exp(LOG_VAR[0] + (LOG_VAR[1] - LOG_VAR[0]) * torch.rand(B, K, generator=g))
    var[0, 0], var[B - 1, K - 1] = 1e-4, 10.0
    xd, md, vd = x.to(dev), mu.to(dev), var.to(dev)

    def launch():
        loss, dmu, dvar = Out(dev, (1,)), Out(dev, (B, K)), Out(dev, (B, K))
        _call("sg_normal_nll", _p(xd), _p(md), _p(vd), B, K, loss.ptr(), dmu.ptr(), dvar.ptr())
        return dict(loss=loss.read(), dmu=dmu.read(), dvar=dvar.read())

    def ref(dt):
        m, v = mu.to(dt).requires_grad_(), var.to(dt).requires_grad_()
        a, b = 0.5 * torch.log(v * 6.283185307179586 + 1e-6), (x.to(dt) - m) ** 2 / (v * 2 + 1e-6)
        loss = (a + b).sum(1).mean()
        loss.backward()
        return dict(loss=loss.detach().reshape(1), dmu=m.grad, dvar=v.grad, _scale=dict(loss=float((a + b).detach().sum(1).abs().mean())))
    return launch, lambda o: verify(o, ref)


# ---- WGAN-GP pieces ---------------------------------------------------------------------------------------------------------------------------------------------------
def grad_penalty(dev, kind, B, n):
    """sg_gp_fwd + sg_gp_bwd: 0 mean (|g_b| - 1)^2 (WGAN-GP / DRA), 1 0.5 mean |g_b|^2 (R1), 2 max |g_b|^2 (maxGP). B >= 3: row 1 is all zero (kind 0: the norm's
    zero subgradient, exact zeros as torch gives), rows 0 and 2 are the same row times 4, so they tie for the maximum and the FIRST is the arg-max"""
    g = _gen("gp", B, n)
    x = torch.randn(B, n, generator=g)
    if B >= 3:
        x[0] = x[0] * 4
        x[1], x[2] = 0, x[0]
    go = torch.tensor([0.75])
    xd, god = x.to(dev), go.to(dev)

    def launch():
        norms, loss, d = Out(dev, (B + 1,)), Out(dev, (1,)), Out(dev, (B, n))
        _call("sg_gp_fwd", kind, _p(xd), B, n, norms.ptr(), loss.ptr())
        _call("sg_gp_bwd", kind, _p(xd), norms.ptr(), _p(god), d.ptr(), B, n)
        nr = norms.read()
        return dict(norms=nr[:B], slot=nr[B:], loss=loss.read(), dgrads=d.read())

    def ref(dt):
        xx = x.to(dt).requires_grad_()
        nrm = xx.norm(2, dim=1)
        dec = {}
        if kind == 0:
            loss = ((nrm - 1) ** 2).mean()
        elif kind == 1:
            loss = 0.5 * (nrm ** 2).mean()
        else:
            loss, arg = torch.max(nrm ** 2, dim=0)           # the lowest index among equals, and the gradient goes there
            dec = dict(arg=arg)
            assert B < 3 or int(arg) == 0
        (loss * go.to(dt)[0]).backward()
        if B >= 3:
            assert bool((xx.grad[1] == 0).all())
        return dict(norms=nrm.detach(), loss=loss.detach().reshape(1), dgrads=xx.grad, _scale=dict(loss=float(loss.detach())), _dec=dec)

    def check(o):
        o = dict(o)
        slot = o.pop("slot")
        if kind == 2:
            same("norms[B] (the arg-max row)", slot, torch.zeros(1))
        else:
            assert bool(untouched(slot).all()), "norms[B] was written by a kind that has no arg-max"
        if B >= 3:
            same("dgrads [zero row]", o["dgrads"][1], torch.zeros(n))
        verify(o, ref)
    return launch, check


def interp_rows(dev, B, n):
    """alpha[b] * real[b] + (1 - alpha[b]) * fake[b]; alpha exactly 0 in row 0 and exactly 1 in the last row (B == 1: 1)"""
    g = _gen("interp", B, n)
    real, fake, alpha = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g), torch.rand(B, generator=g)
    alpha[0], alpha[B - 1] = 0.0, 1.0
    rd, fd, ad = real.to(dev), fake.to(dev), alpha.to(dev)

    def launch():
        out = Out(dev, (B, n))
        _call("sg_interp_rows", _p(rd), _p(fd), _p(ad), out.ptr(), B, n)
        return dict(out=out.read())

    def check(o):
        if B > 1:
            same("out [alpha == 0]", o["out"][0], fake[0])
        same("out [alpha == 1]", o["out"][B - 1], real[B - 1])
        verify(o, lambda dt: dict(out=alpha.to(dt)[:, None] * real.to(dt) + (1 - alpha.to(dt))[:, None] * fake.to(dt)))
    return launch, check


# ---- discriminator head -----------------------------------------------------------------------------------------------------------------------------------------------
def _acts(name, dtype, B, HW, C):
    """activations rounded to `dtype` with +0.0 and -0.0 among them (x > 0 is false for both)"""
    g = _gen(name, B, HW, C)
    x = torch.randn(B, HW, C, generator=g)
    x.view(-1)[1::5] = 0.0
    x.view(-1)[2::7] = -0.0
    x = x.to(dtype)
    assert B * HW * C < 3 or bool((x.view(-1)[2::7].float().view(torch.int32) < 0).all())
    return g, x


def relu_sum_hw(dev, dtype, B, HW, C):
    """sg_relu_sum_hw_fwd + _bwd: h = sum_hw relu(x) in fp32; dx = (x > 0) * dh stored as `dtype`"""
    g, x = _acts("relu_sum", dtype, B, HW, C)
    dh = torch.randn(B, C, generator=g)
    xd, dhd, code = x.to(dev), dh.to(dev), _L().dt(dtype)

    def launch():
        h, dx = Out(dev, (B, C)), Out(dev, (B, HW, C), dtype)
        _call("sg_relu_sum_hw_fwd", code, _p(xd), h.ptr(), B, HW, C)
        _call("sg_relu_sum_hw_bwd", code, _p(xd), _p(dhd), dx.ptr(), B, HW, C)
        return dict(h=h.read(), dx=dx.read())

    def ref(dt):
        xx = x.to(dt).requires_grad_()
        h = torch.relu(xx).sum(1)
        h.backward(dh.to(dt))
        return dict(h=h.detach(), dx=xx.grad, _dec=dict(on=xx.detach() > 0))
    return launch, lambda o: verify(o, ref, extra=dict(dx=BF16_STORE if dtype == BF16 else 0.0))


def masked_sum_hw(dev, dtype, B, HW, C):
    """out = sum_hw t * (x > 0), fp32"""
    g, x = _acts("masked_sum", dtype, B, HW, C)
    t = torch.randn(B, HW, C, generator=g).to(dtype)
    xd, td, code = x.to(dev), t.to(dev), _L().dt(dtype)

    def launch():
        out = Out(dev, (B, C))
        _call("sg_masked_sum_hw", code, _p(td), _p(xd), out.ptr(), B, HW, C)
        return dict(out=out.read())
    return launch, lambda o: verify(o, lambda dt: dict(out=(t.to(dt) * (x.to(dt) > 0)).sum(1)))


def pd_head_fwd(dev, C, emb, b1):
    """adv[b] = <h[b], w1 + emb[b]> + b1 (projection discriminator); emb and b1 are optional"""
    B = 3
    g = _gen("pd_head", C)
    h, w1, e, b = torch.randn(B, C, generator=g), torch.randn(C, generator=g), torch.randn(B, C, generator=g), torch.randn(1, generator=g)
    hd, wd, ed, bd = h.to(dev), w1.to(dev), e.to(dev), b.to(dev)

    def launch():
        adv = Out(dev, (B,))
        _call("sg_pd_head_fwd", _p(hd), _p(wd), _p(bd) if b1 else None, _p(ed) if emb else None, adv.ptr(), B, C)
        return dict(adv=adv.read())

    def ref(dt):
        w = w1.to(dt)[None, :] + (e.to(dt) if emb else 0)
        return dict(adv=(h.to(dt) * w).sum(1) + (b.to(dt) if b1 else 0))
    return launch, lambda o: verify(o, ref)


# ---- the case table: (runner, its arguments) ------------------------------------------------------------------------------------------------------------------------------
ROWS, COLS = (1, 3, 5, 9), (1, 63, 64, 65, 200, 1024)
BATCH = (1, 19, 255, 256, 257, 600)


def _cases():
    out = []
    for r in ROWS:
        for c in COLS:
            out += [(row_normalize, dict(rows=r, cols=c, eps=e)) for e in (1e-12, 1e-8)]
            out += [(row_dot, dict(rows=r, cols=c)), (softmax_rows_bwd2, dict(rows=r, cols=c))]
            out += [(row_scale, dict(rows=r, cols=c, acc=a)) for a in (0, 1)]
    # the four cases of WRAP elements (row_scale twice, scatter_cols, exp_fwd_bwd): capped grids wrap. Well under a second each on the interpreter too
    out += [(row_scale, dict(rows=WRAP_ROWS, cols=WRAP_COLS, acc=a)) for a in (0, 1)]
    for kind in (0, 1):
        out += [(class_loss, dict(kind=kind, rows=r, cols=c)) for r in (1, 3, 5, 9, 257) for c in (2, 63, 64, 65, 130, 1000)]
        out += [(class_loss_bad_label, dict(kind=kind, rows=r, cols=c)) for r, c in ((3, 2), (5, 65), (9, 1000), (257, 130))]
    out += [(class_loss, dict(kind=0, rows=5, cols=c, big=True)) for c in (2, 65, 1000)]
    for kind in (0, 1):
        for B in (2, 5, 64, 65, 130, 256):
            out += [(contrastive, dict(kind=kind, B=B, classes=cl, T=T)) for cl in (2, 3, "B", "one") for T in (1.0, 0.5, 0.07)]
    out += [(contrastive, dict(kind=1, B=B, classes=2, T=0.5, m_p=1.0, zeros=True)) for B in (2, 5, 64, 65, 130, 256)]
    for op in (gather_cols, scatter_cols):
        out += [(op, dict(rows=r, cols=c, bad=b)) for r in (1, 255, 257) for c in (1, 10, 1000) for b in (False, True)]
    out.append((scatter_cols, dict(rows=WRAP_COLS, cols=WRAP_ROWS, bad=False)))
    for B in BATCH:
        out += [(op, dict(kind=k, B=B)) for op in (loss_d, loss_g) for k in (0, 1, 2)]
        out += [(op, dict(B=B)) for op in (loss_ls_d, loss_ls_g, lecam)]
    out += [(fm_loss, dict(B=B, C=C)) for B, C in ((1, 1), (7, 255), (8, 256), (5, 257), (3, 700))]
    out += [(exp_fwd_bwd, dict(n=n)) for n in (1, 255, 257, WRAP)]
    out += [(normal_nll, dict(B=B, K=K)) for B, K in ((3, 1), (64, 4), (129, 2), (300, 3))]
    for B, n in ((1, 1), (3, 255), (3, 257), (5, 3072), (300, 10)):
        out += [(grad_penalty, dict(kind=k, B=B, n=n)) for k in (0, 1, 2)]
        out.append((interp_rows, dict(B=B, n=n)))
    for dtype in (F32, BF16):
        for shape in ((1, 1, 1), (3, 16, 20), (2, 16, 300)):
            out += [(op, dict(dtype=dtype, B=shape[0], HW=shape[1], C=shape[2])) for op in (relu_sum_hw, masked_sum_hw)]
    out += [(pd_head_fwd, dict(C=C, emb=e, b1=b)) for C in (1, 255, 257, 1536) for e in (False, True) for b in (False, True)]
    return out


CASES = _cases()


def case_id(case):
    op, spec = case
    return " ".join([op.__name__] + [f"{k}={str(v).replace('torch.', '')}" for k, v in spec.items()])


def case_launch(case, dev):
    """the case's launch() alone (the table test of tests/test_head_kernels_cpu.py records what it calls)"""
    op, spec = case
    return op(dev, **spec)[0]


def run_case(case, dev):
    op, spec = case
    print(f"\n{case_id(case)}")
    launch, check = op(dev, **spec)
    check(twice(launch))
