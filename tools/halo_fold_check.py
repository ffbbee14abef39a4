"""Outputs of the halo and quad forward / data-gradient kernels (conv_v3.h, conv_v4.h, conv_q.h) across two builds of the library, bit for bit.

    SG_LIBSGAMD=<other build> python tools/halo_fold_check.py --save ref.pt
    python tools/halo_fold_check.py --against ref.pt

Runs the small case tables of tests/test_conv_v2_gpu.py (V3_CASES with SG_CONV_V4=0 SG_CONV_V3=force and V4_CASES with SG_CONV_V4=all, forward and data
gradient; SKIP_CASES; MASKRES_CASES) and of tests/test_quad_gpu.py (FWD_CASES for each of SG_CONV_Q_BJ / SG_CONV_Q_DB = 256 / 128 / 256db; SKIP_CASES; the four
launches of test_conv_epilogue_bn_statistics with their per-tile statistics rows). Each case's key carries the kernel family that the launch profiler saw take it;
--against asserts torch.equal on every output."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402


def run():
    from studiogan_amd import functional as F, _lib as L
    import test_conv_v2_gpu as TC
    import test_quad_gpu as TQ
    from test_kernels_gpu import rnd, nhwc
    from util import engine_launches, launched
    d, dt, outs, env = torch.device("cuda:0"), torch.bfloat16, {}, os.environ
    dev = lambda t: None if t is None else t.to(d)

    def put(key, launch):          # the key carries the kernel family that took the launch: two builds that dispatch differently do not compare
        with engine_launches() as counts:
            ts = launch()
        outs[f"{key} [{' + '.join(launched(counts)) or 'untagged'}]"] = tuple(t.cpu() for t in (ts if isinstance(ts, tuple) else (ts,)))
    # (data gradient: the cases whose transposed problem the tests send through the kernel)
    for tag, cases, v4, dgrad in (("v3", TC.V3_CASES, "0", lambda ci, co: ci % 96 == 0 or ci % 128 == 0), ("v4", TC.V4_CASES, "all", lambda ci, co: co % 32 == 0 and (ci % 96 == 0 or ci % 64 == 0))):
        env["SG_CONV_V4"], env["SG_CONV_V3"], env["SG_CONV_V2"] = v4, "force", "force"
        for case in cases:
            N, Cin, Cout, H, relu, up, pool = case
            Ho = H * (2 if up else 1)
            Hy = Ho // 2 if pool else Ho
            x, w, bias, res = rnd((N, Cin, H, H), dt, 91), rnd((Cout, Cin, 3, 3), dt, 92, 0.1), rnd((Cout,), torch.float32, 93), rnd((N, Cout, Hy, Hy), dt, 94)
            xd, al = nhwc(x).to(d), 0.25 if pool else 1.0
            wd, wdg = w.permute(0, 2, 3, 1).contiguous().to(d), w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(d)
            put(f"{tag} fwd {case}", lambda: F.conv2d_raw(xd, wd.data_ptr(), Cin, Cout, 3, 3, 1, 1, 1, (L.PIX_RELU if relu else 0) | (L.PIX_UPSAMPLE if up else 0),
                                                          L.EPI_POOL if pool else 0, bias=bias.to(d), res=nhwc(res).to(d), alpha=al))
            if not dgrad(Cin, Cout):
                continue
            gy = rnd((N, Cout, Hy, Hy), dt, 95)
            put(f"{tag} dgrad {case}", lambda: F.conv2d_raw(nhwc(gy).to(d), wdg.data_ptr(), Cout, Cin, 3, 3, 1, 1, 1, L.PIX_UPSAMPLE if pool else 0,
                                                            L.EPI_POOL if up else 0, mask=xd if relu else None, alpha=al))
    for k in ("SG_CONV_V4", "SG_CONV_V3", "SG_CONV_V2"):
        env.pop(k)
    for case in TC.SKIP_CASES:
        N, C, Cout, C2, H, relu, pool, up2 = case
        H2 = H // 2 if up2 else H
        h, x, w, w0 = rnd((N, C, H, H), dt, 41), rnd((N, C2, H2, H2), dt, 42), rnd((Cout, C, 3, 3), dt, 43, 0.1), rnd((Cout, C2, 1, 1), dt, 44, 0.1)
        wd, w0d = w.permute(0, 2, 3, 1).contiguous().to(d), w0.permute(0, 2, 3, 1).contiguous().to(d)
        b, b0 = rnd((Cout,), torch.float32, 45).to(d), rnd((Cout,), torch.float32, 46).to(d)
        put(f"v4 skip {case}", lambda: F.conv2d_skip_raw(nhwc(h).to(d), wd.data_ptr(), C, Cout, nhwc(x).to(d), w0d.data_ptr(), C2, up2, L.PIX_RELU if relu else 0,
                                                         L.EPI_POOL if pool else 0, bias=b, bias2=b0, alpha=0.25 if pool else 1.0))
    for case in TC.MASKRES_CASES:
        N, Cin, Cout, H, R, up, pool, cenv = case
        env.update(cenv)
        Hy = H * (2 if up else 1) // (2 if pool else 1)
        x, w, m, res = rnd((N, Cin, H, H), dt, 51), rnd((Cout, Cin, R, R), dt, 52, 0.1), rnd((N, Cout, Hy, Hy), dt, 53), rnd((N, Cout, Hy, Hy), dt, 54)
        wd = w.permute(0, 2, 3, 1).contiguous().to(d)
        put(f"mask + residual {case[:7]}", lambda: F.conv2d_raw(nhwc(x).to(d), wd.data_ptr(), Cin, Cout, R, R, 1, R // 2, R // 2, L.PIX_UPSAMPLE if up else 0,
                                                                L.EPI_POOL if pool else 0, mask=nhwc(m).to(d), res=nhwc(res).to(d), alpha=0.25 if pool else 1.0))
        for k in cenv:
            env.pop(k)

    def quad(bj):
        env["SG_CONV_Q_BJ"], env["SG_CONV_Q_DB"] = bj[:3], "1" if bj.endswith("db") else "0"
    for bj in ("256", "128", "256db"):
        quad(bj)
        for case in TQ.FWD_CASES:
            form, N, Hl, Wl, C, Cout, relu_in, with_bias, with_mask, with_res, relu_out = case
            Hx, Wx, Hy, Wy = (2 * Hl, 2 * Wl, Hl, Wl) if form == 0 else (Hl, Wl, 2 * Hl, 2 * Wl)
            x, w9 = rnd((N, Hx, Wx, C), dt, 311), rnd((Cout, 3, 3, C), dt, 312, 0.1).to(d)
            wq = torch.empty(Cout, 16, C, dtype=dt, device=d)
            F.quad_pack_raw(w9.data_ptr(), wq, form, Cout, C)
            bias, res, mask = (dev(rnd(sh, ty, seed) if on else None) for sh, ty, seed, on in (((Cout,), torch.float32, 313, with_bias), ((N, Hy, Wy, Cout), dt, 315, with_res),
                                                                                                 ((N, Hy, Wy, Cout), dt, 314, with_mask)))
            put(f"q bj={bj} {case}", lambda: F.conv2d_q_raw(x.to(d), wq.data_ptr(), form, C, Cout, L.PIX_RELU if relu_in else 0, L.EPI_RELU if relu_out else 0, bias=bias, res=res, mask=mask))
    for case in TQ.SKIP_CASES:
        N, Hl, Wl, C, Cout, C2, relu, bj = case
        quad(bj)
        h, x, w9, w0 = rnd((N, 2 * Hl, 2 * Wl, C), dt, 341), rnd((N, 2 * Hl, 2 * Wl, C2), dt, 342), rnd((Cout, 3, 3, C), dt, 343, 0.1).to(d), rnd((Cout, C2), dt, 344, 0.2).to(d)
        wq = torch.empty(Cout, 16, C, dtype=dt, device=d)
        F.quad_pack_raw(w9.data_ptr(), wq, 0, Cout, C)
        w0q = (w0.float() * 0.25).to(dt)
        w0q = w0q.repeat(1, 4).contiguous() if C2 == 8 else w0q
        b2, b0 = rnd((Cout,), torch.float32, 345).to(d), rnd((Cout,), torch.float32, 346).to(d)
        put(f"q skip {case}", lambda: F.conv2d_q_raw(h.to(d), wq.data_ptr(), L.Q_POOL, C, Cout, L.PIX_RELU if relu else 0, 0, bias=b2, x2=x.to(d), w2q_ptr=w0q.data_ptr(),
                                                     bias2=b0, x2_norelu=C2 == 8))
    env.pop("SG_CONV_Q_DB")
    N, Hl, Wl, C, Cout = 3, 8, 16, 64, 96          # (test_conv_epilogue_bn_statistics)
    w9, bias = rnd((Cout, 3, 3, C), dt, 501, 0.1).to(d), rnd((Cout,), torch.float32, 502).to(d)
    for kind in ("quad_up", "quad_up_128", "quad_pool", "v4_skip"):
        F._STATS_OFFER[0] = None
        if kind.startswith("quad"):
            form = L.Q_UP if "up" in kind else L.Q_POOL
            env["SG_CONV_Q_BJ"] = "128" if kind.endswith("128") else "256"
            x = rnd((N, Hl, Wl, C) if form == L.Q_UP else (N, 2 * Hl, 2 * Wl, C), dt, 503)
            wq = torch.empty(Cout, 16, C, dtype=dt, device=d)
            F.quad_pack_raw(w9.data_ptr(), wq, form, Cout, C)
            y = F.conv2d_q_raw(x.to(d), wq.data_ptr(), form, C, Cout, 0, 0, bias=bias, stats=True)
        else:
            w0 = rnd((Cout, 32), dt, 505, 0.2).to(d)
            y = F.conv2d_skip_raw(rnd((N, 2 * Hl, 2 * Wl, C), dt, 503).to(d), w9.data_ptr(), C, Cout, rnd((N, Hl, Wl, 32), dt, 504).to(d), w0.data_ptr(), 32, True, 0, 0, bias=bias, bias2=bias, stats=True)
        assert F._STATS_OFFER[0] is not None, f"no statistics were offered: {kind}"
        outs[f"statistics {kind}"] = (y.cpu(), F._STATS_OFFER[0][3].cpu())
    env.pop("SG_CONV_Q_BJ")
    return outs


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--save")
    g.add_argument("--against")
    a = ap.parse_args()
    import studiogan_amd
    print("library:", studiogan_amd.LIB_PATH)
    outs = run()
    assert all(t is not None for ts in outs.values() for t in ts), "a kernel refused an eligible problem"
    if a.save:
        torch.save(outs, a.save)
        print(f"saved {len(outs)} cases to {a.save}")
    else:
        ref = torch.load(a.against)
        assert ref.keys() == outs.keys(), "the two runs cover different cases"
        bad = 0
        for k, ts in outs.items():
            assert all(t.float().abs().max() > 0 for t in ts), f"all-zero output: {k}"
            eq = len(ts) == len(ref[k]) and all(torch.equal(t, r) for t, r in zip(ts, ref[k]))
            bad += not eq
            print(f"{k:100s} {'equal' if eq else 'DIFFERS'}" + (" (output and statistics rows)" if len(ts) > 1 else ""))
        assert bad == 0, f"{bad} of {len(outs)} cases differ from {a.against}"
        print(f"all {len(outs)} cases bit-identical to {a.against}")
