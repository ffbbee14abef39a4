"""Outputs of the halo and quad weight-gradient kernels across two builds of the library, bit for bit.

    SG_LIBSGAMD=<other build> python tools/wgrad_fold_check.py --save ref.pt
    python tools/wgrad_fold_check.py --against ref.pt

Runs WV3_CASES (tests/test_conv_v2_gpu.py) and WG_CASES (tests/test_quad_gpu.py) through conv2d_wgrad_raw / conv2d_q_wgrad_raw with SG_WGRAD_V3=force,
both values of SG_WGRAD_V3_LEAN / SG_WGRAD_Q_LEAN and splits 0 and 3; --against asserts torch.equal on every dW and every bias gradient."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402


def run():
    from studiogan_amd import functional as F, _lib as L
    from test_conv_v2_gpu import WV3_CASES
    from test_quad_gpu import WG_CASES
    from test_kernels_gpu import rnd
    d, dt, outs = torch.device("cuda:0"), torch.bfloat16, {}
    os.environ["SG_WGRAD_V3"] = "force"
    for lean in ("0", "1"):
        os.environ["SG_WGRAD_V3_LEAN"] = os.environ["SG_WGRAD_Q_LEAN"] = lean
        for splits in (0, 3):
            for case in WV3_CASES:
                N, Cin, Cout, H, relu, up, pool = case
                Ho = H * (2 if up else 1)
                hg = Ho // 2 if pool else Ho
                x, gy = rnd((N, H, H, Cin), dt, 81).to(d), rnd((N, hg, hg, Cout), dt, 82).to(d)
                dw = torch.zeros((Cout, 3, 3, Cin), dtype=torch.float32, device=d)
                db = torch.zeros((Cout,), dtype=torch.float32, device=d)
                assert F.conv2d_wgrad_raw(x, gy, dw.data_ptr(), Cin, Cout, 3, 3, Ho, Ho, 1, 1, 1, (L.PIX_RELU if relu else 0) | (L.PIX_UPSAMPLE if up else 0),
                                          L.PIX_UPSAMPLE if pool else 0, alpha=0.5, dbias=db, splits=splits), f"bias gradient not fused: {case}"
                outs[f"v3 lean={lean} splits={splits} {case}"] = (dw.cpu(), db.cpu())
            for case in WG_CASES:
                form, N, Hl, Wl, C, Cout, relu, _ = case
                Hx, Wx = (2 * Hl, 2 * Wl) if form == 0 else (Hl, Wl)
                Hg, Wg = (Hl, Wl) if form == 0 else (2 * Hl, 2 * Wl)
                x, dy = rnd((N, Hx, Wx, C), dt, 341).to(d), rnd((N, Hg, Wg, Cout), dt, 342).to(d)
                dw = torch.zeros(Cout, 9, C, dtype=torch.float32, device=d)
                db = torch.zeros(Cout, dtype=torch.float32, device=d)
                assert F.conv2d_q_wgrad_raw(x, dy, dw.data_ptr(), form, C, Cout, L.PIX_RELU if relu else 0, alpha=0.5, dbias=db, splits=splits), case
                torch.cuda.synchronize()
                outs[f"q lean={lean} splits={splits} {case}"] = (dw.cpu(), db.cpu())
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
    if a.save:
        torch.save(outs, a.save)
        print(f"saved {len(outs)} cases (dW and db each) to {a.save}")
    else:
        ref = torch.load(a.against)
        assert ref.keys() == outs.keys(), "the two runs cover different cases"
        bad = 0
        for k, (dw, db) in outs.items():
            e = (torch.equal(dw, ref[k][0]), torch.equal(db, ref[k][1]))
            assert dw.abs().max() > 0 and db.abs().max() > 0, f"all-zero output: {k}"
            bad += e != (True, True)
            print(f"{k:70s} dW {'equal' if e[0] else 'DIFFERS'}  db {'equal' if e[1] else 'DIFFERS'}")
        assert bad == 0, f"{bad} of {len(outs)} cases differ from {a.against}"
        print(f"all {len(outs)} cases bit-identical (dW and bias gradient) to {a.against}")
