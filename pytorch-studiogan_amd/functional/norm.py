"""(conditional) batch norm, synchronised across ranks (csrc/norm.hip, comm.hip, p2p.hip; reference src/utils/ops.py:14-28,227-228)."""
from ._base import *  # noqa: F401,F403  (shared helpers, switches, raw launch wrappers, torch / _lib / comm)

# ---------------------------------------------------------------------------------------------------------
# (conditional) batch norm
# ---------------------------------------------------------------------------------------------------------
class BNCfg:
    __slots__ = ("batch_stats", "track", "eps", "momentum", "relu", "group", "packed")

    def __init__(self, batch_stats, track, eps, momentum, relu, group=None, packed=False):
        self.batch_stats, self.track, self.eps, self.momentum, self.relu, self.group = batch_stats, track, eps, momentum, relu, group
        self.packed = packed      # `gain` is the packed per-sample [N][gain(C) | bias(C)] tensor of a conditional batch norm (CbnAffineFn), `bias` is None


def _world(group):
    if group is not None and dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group if group is not True else None)
    return 1


def _allreduce_sum(t, group):
    """sum over the data-parallel ranks: the C ABI's RCCL entry point when a native communicator serves the group (comm.enable),
    torch.distributed otherwise."""
    nc = _comm.native_for(group)
    pp = _comm.p2p_for(group) if (t.dtype == torch.float64 and t.numel() <= _comm.P2PMailbox.MAX_DOUBLES) else None
    with _comm.exposed():          # on the compute stream: the whole collective is exposed (bench.py exposed_comm_ms_per_step)
        if pp is not None:         # peer-store mailboxes: one launch, one xGMI round trip (csrc/p2p.hip)
            pp.allreduce_f64_(t)
        elif nc is not None:
            nc.allreduce_(t)
        else:
            dist.all_reduce(t, group=None if group is True else group)


class BNFn(torch.autograd.Function):
    """y = relu?( (x - mean) * invstd * gain + bias ) with batch or running statistics.

    gain/bias: None, per-channel [C] (nn.BatchNorm2d affine) or per-sample [N,C] (ConditionalBatchNorm2d: gain already
    holds 1 + W_g y). Sync-BN = one all-reduce of the fp64 partial sums between the two kernels
    (reference src/utils/ops.py:14-28,227-228; src/models/model.py:161-165)."""

    @staticmethod
    def forward(ctx, x, gain, bias, running_mean, running_var, cfg, *opt):
        x = _c(x)
        _tick()
        fused = _take_stats(x) if cfg.batch_stats else None      # statistics the producing convolution took in its epilogue
        ctx.link = opt[0] if opt else None      # optional 7th argument: a GradLink (see ConvSkipFn)
        ctx.nopt = len(opt)
        N, H, W, Cc = x.shape
        HW = H * W
        dev = x.device
        mean = torch.empty(Cc, dtype=torch.float32, device=dev)
        invstd = torch.empty(Cc, dtype=torch.float32, device=dev)
        count = float(N * HW)
        if cfg.batch_stats:
            ws = _world(cfg.group)
            rm = running_mean if cfg.track else None
            rv = running_var if cfg.track else None
            nc = _comm.native_for(cfg.group) if ws > 1 else None
            pp = _comm.p2p_for(cfg.group) if (ws > 1 and 2 * Cc <= _comm.P2PMailbox.MAX_DOUBLES) else None
            if pp is not None:
                # sync-BN with the exchange FUSED INTO the finalize kernel: this rank's partial sums go straight into every peer's HBM (csrc/p2p.hip), the same
                # launch waits for the peers' and writes mean / invstd / running statistics of the global batch
                partial = zeros_small(2 * Cc, torch.float64, dev)
                if fused is not None:
                    L.call("sg_bn_stats_from_tiles", fused[0].data_ptr(), fused[1], Cc, L.ptr(partial), L.stream())
                else:
                    L.call("sg_bn_partial_stats", L.dt(x), L.ptr(x), Cc, N * HW, Cc, L.ptr(partial), L.stream())
                count *= ws
                with _comm.exposed():
                    L.call("sg_bn_finalize_p2p", pp.handle, L.ptr(partial), count, Cc, cfg.eps, cfg.momentum, L.ptr(mean), L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.stream())
            elif fused is not None:
                partial = zeros_small(2 * Cc, torch.float64, dev)
                L.call("sg_bn_stats_from_tiles", fused[0].data_ptr(), fused[1], Cc, L.ptr(partial), L.stream())
                if ws > 1:
                    _allreduce_sum(partial, cfg.group)
                    count *= ws
                L.call("sg_bn_finalize", L.ptr(partial), count, Cc, cfg.eps, cfg.momentum, L.ptr(mean), L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.stream())
            elif nc is not None:
                # sync-BN statistics in ONE C-ABI call: partial sums -> RCCL all-reduce -> mean / invstd / running stats, same stream
                partial = torch.empty(2 * Cc, dtype=torch.float64, device=dev)
                L.call("sg_bn_stats_sync", L.dt(x), L.ptr(x), Cc, N * HW, Cc, L.ptr(partial), nc.handle, cfg.eps, cfg.momentum, L.ptr(mean),
                       L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.stream())
                count *= ws
            else:
                partial = zeros_small(2 * Cc, torch.float64, dev)
                L.call("sg_bn_partial_stats", L.dt(x), L.ptr(x), Cc, N * HW, Cc, L.ptr(partial), L.stream())
                if ws > 1:
                    dist.all_reduce(partial, group=None if cfg.group is True else cfg.group)
                    count *= ws
                L.call("sg_bn_finalize", L.ptr(partial), count, Cc, cfg.eps, cfg.momentum, L.ptr(mean), L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.stream())
        else:
            L.call("sg_bn_from_running", L.ptr(running_mean), L.ptr(running_var), Cc, cfg.eps, L.ptr(mean), L.ptr(invstd), L.stream())
        gsn = 0
        bias_ptr_off = 0
        if cfg.packed:
            gain = _c(gain.float())
            assert bias is None and gain.dim() == 2 and gain.shape[1] == 2 * Cc
            gsn, bias_ptr_off = 2 * Cc, 4 * Cc
        elif gain is not None:
            gain = _c(gain.float())
            gsn = Cc if gain.dim() == 2 else 0
        if bias is not None:
            bias = _c(bias.float())
            assert (Cc if bias.dim() == 2 else 0) == gsn or gain is None
            if gain is None:
                gsn = Cc if bias.dim() == 2 else 0
        y = torch.empty_like(x)
        bptr = (L.ptr(gain) + bias_ptr_off) if cfg.packed else L.ptr(bias)
        L.call("sg_bn_apply", L.dt(x), L.ptr(x), L.ptr(y), N, HW, Cc, L.ptr(mean), L.ptr(invstd), L.ptr(gain), bptr, gsn, 1 if cfg.relu else 0, L.stream())
        ctx.save_for_backward(x, gain, bias, mean, invstd)
        ctx.cfg, ctx.gsn, ctx.count = cfg, gsn, count
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gain, bias, mean, invstd = ctx.saved_tensors
        cfg, gsn = ctx.cfg, ctx.gsn
        if torch.is_grad_enabled():
            if gsn:
                # per-sample rows (conditional batch norm): dx AND the row gradients as one differentiable operator (latent optimisation through a
                # class-conditional generator). No GradLink is armed in a create_graph pass (ConvSkipFn / SliceUpFn return their gradients themselves).
                if cfg.packed:
                    rows = gain
                else:      # separate per-sample gain / bias tensors: packed here, so that the operator below has ONE layout
                    Cc = x.shape[3]
                    z = torch.zeros((x.shape[0], Cc), dtype=torch.float32, device=x.device)
                    rows = torch.cat([gain if gain is not None else z + 1.0, bias if bias is not None else z], dim=1)
                dx, drows = CBNBwdFn.apply(dy, x, rows, mean, invstd, cfg, ctx.count)
                if not ctx.needs_input_grad[0]:
                    dx = None
                if cfg.packed:
                    return (dx, drows if ctx.needs_input_grad[1] else None, None, None, None, None) + (None,) * ctx.nopt
                Cc = x.shape[3]
                return (dx, drows[:, :Cc] if (gain is not None and ctx.needs_input_grad[1]) else None,
                        drows[:, Cc:] if (bias is not None and ctx.needs_input_grad[2]) else None, None, None, None) + (None,) * ctx.nopt
            if _param_grad_wanted(gain, bias):
                raise NotImplementedError("create_graph=True through a per-channel affine BN is supported for its input gradient only (WGAN-GP path); "
                                          "per-sample rows (conditional batch norm) have the full second-order pass")
            dx = BNBwdFn.apply(dy, x, gain, bias, mean, invstd, cfg, ctx.count) if ctx.needs_input_grad[0] else None
            return (dx, None, None, None, None, None) + (None,) * ctx.nopt
        dy = _c(dy)
        N, H, W, Cc = x.shape
        HW = H * W
        dev = x.device
        skip_dx = ctx.link.take() if ctx.link is not None else None     # the skip path's gradient w.r.t. this same input (GradLink)
        if skip_dx is not None and not ctx.needs_input_grad[0]:
            raise RuntimeError("GradLink: a skip gradient was handed over but this batch norm's input needs no gradient")
        sums = zeros_small((N, Cc, 2), torch.float32, dev)
        bptr = (L.ptr(gain) + 4 * Cc) if cfg.packed else L.ptr(bias)       # packed cBN rows: [gain(C) | bias(C)], pitch gsn = 2 C
        L.call("sg_bn_bwd_reduce", L.dt(x), L.ptr(x), L.ptr(dy), N, HW, Cc, L.ptr(mean), L.ptr(invstd), L.ptr(gain), bptr, gsn,
               1 if cfg.relu else 0, L.ptr(sums), L.stream())
        chan = torch.empty(2 * Cc, dtype=torch.float64, device=dev)
        dgain = zeros_like_small(gain) if (gain is not None and ctx.needs_input_grad[1]) else None
        dbias = zeros_like_small(bias) if (bias is not None and ctx.needs_input_grad[2]) else None
        dbptr = ((L.ptr(dgain) + 4 * Cc) if dgain is not None else None) if cfg.packed else L.ptr(dbias)
        L.call("sg_bn_bwd_finalize", L.ptr(sums), N, Cc, L.ptr(gain), gsn, L.ptr(dgain), dbptr, L.ptr(chan), L.stream())
        dx = None
        if ctx.needs_input_grad[0]:
            if cfg.batch_stats and _world(cfg.group) > 1:
                _allreduce_sum(chan, cfg.group)
            dx = torch.empty_like(x)
            L.call("sg_bn_bwd_apply_res", L.dt(x), L.ptr(x), L.ptr(dy), L.ptr(dx), N, HW, Cc, L.ptr(mean), L.ptr(invstd), L.ptr(gain), bptr,
                   gsn, 1 if cfg.relu else 0, L.ptr(chan), ctx.count, 1 if cfg.batch_stats else 0, L.ptr(_c(skip_dx) if skip_dx is not None else None), L.stream())
        return (dx, dgain, dbias, None, None, None) + (None,) * ctx.nopt


class BNBwdFn(torch.autograd.Function):
    """BN's data gradient dx(dy, x, gain) as a differentiable op (statistics are functions of x): the second-order pass
    of the gradient penalty through a discriminator that uses batch norm (WGAN-GP.yaml: no SN => BN in D). Formulas and
    kernels: csrc/norm.hip "second-order backward"."""

    @staticmethod
    def forward(ctx, dy, x, gain, bias, mean, invstd, cfg, count):
        dy = _c(dy)
        N, H, W, Cc = x.shape
        dev = x.device
        sums = zeros_small((N, Cc, 2), torch.float32, dev)
        L.call("sg_bn_bwd_reduce", L.dt(x), L.ptr(x), L.ptr(dy), N, H * W, Cc, L.ptr(mean), L.ptr(invstd), L.ptr(gain), L.ptr(bias), 0,
               1 if cfg.relu else 0, L.ptr(sums), L.stream())
        chan = torch.empty(2 * Cc, dtype=torch.float64, device=dev)
        L.call("sg_bn_bwd_finalize", L.ptr(sums), N, Cc, L.ptr(gain), 0, None, None, L.ptr(chan), L.stream())
        if cfg.batch_stats and _world(cfg.group) > 1:
            _allreduce_sum(chan, cfg.group)
        dx = torch.empty_like(x)
        L.call("sg_bn_bwd_apply", L.dt(x), L.ptr(x), L.ptr(dy), L.ptr(dx), N, H * W, Cc, L.ptr(mean), L.ptr(invstd), L.ptr(gain), L.ptr(bias),
               0, 1 if cfg.relu else 0, L.ptr(chan), count, 1 if cfg.batch_stats else 0, L.stream())
        ctx.save_for_backward(dy, x, gain, bias, mean, invstd)
        ctx.cfg, ctx.count = cfg, count
        return dx

    @staticmethod
    def backward(ctx, u):
        dy, x, gain, bias, mean, invstd = ctx.saved_tensors
        cfg = ctx.cfg
        u = _c(u)
        N, H, W, Cc = x.shape
        dev = x.device
        relu = 1 if cfg.relu else 0
        sums = zeros_small((N, Cc, 5), torch.float32, dev)
        L.call("sg_bn_bwd2_reduce", L.dt(x), L.ptr(x), L.ptr(dy), L.ptr(u), N, H * W, Cc, L.ptr(mean), L.ptr(invstd), L.ptr(gain), L.ptr(bias), relu,
               L.ptr(sums), L.stream())
        chan_local = torch.empty(5 * Cc, dtype=torch.float64, device=dev)
        L.call("sg_bn_bwd2_finalize", L.ptr(sums), N, Cc, L.ptr(chan_local), L.stream())
        chan = chan_local
        if cfg.batch_stats and _world(cfg.group) > 1:
            chan = chan_local.clone()
            _allreduce_sum(chan, cfg.group)
        use_batch = 1 if cfg.batch_stats else 0
        g_dy = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        g_x = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        if g_dy is not None or g_x is not None:
            L.call("sg_bn_bwd2_apply", L.dt(x), L.ptr(x), L.ptr(dy), L.ptr(u), L.ptr(g_dy), L.ptr(g_x), N, H * W, Cc, L.ptr(mean), L.ptr(invstd),
                   L.ptr(gain), L.ptr(bias), relu, L.ptr(chan), ctx.count, use_batch, L.stream())
        dgain = None
        if gain is not None and ctx.needs_input_grad[2]:
            dgain = zeros_like_small(gain)
            L.call("sg_bn_bwd2_dgain", L.ptr(chan_local), L.ptr(chan), ctx.count, L.ptr(invstd), Cc, use_batch, L.ptr(dgain), L.stream())
        return g_dy, g_x, dgain, None, None, None, None, None


class CBNBwdFn(torch.autograd.Function):
    """The backward of a batch norm with PER-SAMPLE affine rows (conditional batch norm; rows = packed [N][gain(C) | bias(C)]) as a differentiable operator:
    (dy, x, rows) -> (dx, drows), statistics being functions of x. Its own backward takes the cotangents of dx and of the row gradients and returns the gradients
    w.r.t. dy, x and the gain rows (the bias rows enter through the ReLU mask only): LOGAN's latent optimisation through a class-conditional generator (reference
    src/utils/losses.py:278-298). Formulas and kernels: csrc/norm.hip "second-order backward with per-sample affine rows"."""

    @staticmethod
    def forward(ctx, dy, x, rows, mean, invstd, cfg, count):
        if _world(cfg.group) > 1:
            raise NotImplementedError("CBNBwdFn: create_graph=True through a SYNCHRONISED conditional batch norm (world size > 1) is not implemented -- the per-channel "
                                      "pass's all-reduce of the fp64 channel terms would carry over, but no multi-rank LOGAN run exists to check it against")
        dy, rows = _c(dy), _c(rows.float())
        N, H, W, Cc = x.shape
        HW = H * W
        dev = x.device
        assert rows.shape == (N, 2 * Cc)
        relu = 1 if cfg.relu else 0
        gptr, bptr = L.ptr(rows), L.ptr(rows) + 4 * Cc
        sums = zeros_small((N, Cc, 2), torch.float32, dev)
        L.call("sg_bn_bwd_reduce", L.dt(x), L.ptr(x), L.ptr(dy), N, HW, Cc, L.ptr(mean), L.ptr(invstd), gptr, bptr, 2 * Cc, relu, L.ptr(sums), L.stream())
        chan = torch.empty(2 * Cc, dtype=torch.float64, device=dev)
        drows = torch.zeros_like(rows)          # (an output of this operator: a tensor of its own, not a piece of the shared zero block)
        L.call("sg_bn_bwd_finalize", L.ptr(sums), N, Cc, gptr, 2 * Cc, L.ptr(drows), L.ptr(drows) + 4 * Cc, L.ptr(chan), L.stream())
        dx = torch.empty_like(x)
        L.call("sg_bn_bwd_apply", L.dt(x), L.ptr(x), L.ptr(dy), L.ptr(dx), N, HW, Cc, L.ptr(mean), L.ptr(invstd), gptr, bptr, 2 * Cc, relu, L.ptr(chan), count,
               1 if cfg.batch_stats else 0, L.stream())
        ctx.save_for_backward(dy, x, rows, mean, invstd)
        ctx.cfg, ctx.count = cfg, count
        ctx.set_materialize_grads(False)
        return dx, drows

    @staticmethod
    def backward(ctx, u, ab):
        _first_order_only("CBNBwdFn")        # (third order: not a path of the reference)
        dy, x, rows, mean, invstd = ctx.saved_tensors
        cfg = ctx.cfg
        N, H, W, Cc = x.shape
        HW = H * W
        dev = x.device
        if u is None and ab is None:
            return (None,) * 7
        u = _c(u) if u is not None else torch.zeros_like(x)
        ab = _c(ab.float()) if ab is not None else None
        relu, use_batch = 1 if cfg.relu else 0, 1 if cfg.batch_stats else 0
        gptr, bptr = L.ptr(rows), L.ptr(rows) + 4 * Cc
        aptr = L.ptr(ab) if ab is not None else None
        bcot = (L.ptr(ab) + 4 * Cc) if ab is not None else None
        sums = zeros_small((N, Cc, 5), torch.float32, dev)
        L.call("sg_cbn_bwd2_reduce", L.dt(x), L.ptr(x), L.ptr(dy), L.ptr(u), N, HW, Cc, L.ptr(mean), L.ptr(invstd), gptr, bptr, 2 * Cc, relu, L.ptr(sums), L.stream())
        chan = torch.empty(7 * Cc, dtype=torch.float64, device=dev)
        L.call("sg_cbn_bwd2_finalize", L.ptr(sums), N, Cc, gptr, aptr, 2 * Cc, L.ptr(chan), L.stream())
        g_dy = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        g_x = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        if g_dy is not None or g_x is not None:
            L.call("sg_cbn_bwd2_apply", L.dt(x), L.ptr(x), L.ptr(dy), L.ptr(u), L.ptr(g_dy), L.ptr(g_x), N, HW, Cc, L.ptr(mean), L.ptr(invstd), gptr, bptr, aptr, bcot,
                   2 * Cc, relu, L.ptr(chan), ctx.count, use_batch, L.stream())
        g_rows = None
        if ctx.needs_input_grad[2]:
            g_rows = zeros_like_small(rows)          # (the bias half stays zero)
            L.call("sg_cbn_bwd2_dgain", L.ptr(sums), L.ptr(chan), ctx.count, L.ptr(invstd), N, Cc, 2 * Cc, use_batch, L.ptr(g_rows), L.stream())
        return g_dy, g_x, g_rows, None, None, None, None


__all__ = ['BNBwdFn', 'BNCfg', 'BNFn', 'CBNBwdFn', '_allreduce_sum', '_world']
