"""Outputs of the spectral-norm entry points (csrc/sn.hip: sg_sn_forward / sg_sn_backward) across two builds of the library, bit for bit.

    SG_LIBSGAMD=<library built from the parent commit> python tools/sn_fold_check.py --save ref.pt
    python tools/sn_fold_check.py --against ref.pt

Four tables in fp32 and bf16: tests/sn_checks.py LAYERS (every row also checks itself against fp64 as in the test), WIDE_LAYERS (the table that takes the fallback
pack kernel k_sn_pack), this tool's TALL_LAYERS (linear layers of 1100 to 24576 rows) and the 70-layer table of forward_table, in one call and split at 37. After every call each layer's buffers are kept WHOLE, padding and
pre-filled sentinel bytes included: u, v, sigma, both snapshots, w_fwd, w_dgrad, w_f32, dw, and the `work` scratch. sn.hip has no atomics and sums in fixed orders,
so --against asserts torch.equal on the stored bits of every one of them. One difference is permitted, --parent-leaves-wide-padding: on WIDE_LAYERS a parent build
whose k_sn_pack leaves the padding channels of w_fwd unwritten is compared on the real channels (and on the bytes behind the image) only; the number of elements
that excludes is printed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

BUFS = ("u_d", "v_d", "sigma_d", "us_d", "vs_d", "fwd_d", "dg_d", "f32_d", "dw_d",      # sn_checks.run's names ...
        "u", "v", "sigma", "us", "vs", "fwd", "dg")                                      # ... and forward_table's
# tall linear layers: k_sn_u's row walks (norm, u, u_snap) with 2 to 24 elements per thread and up to three trips, more chances than LAYERS' two for a last-place
# change of the norm to reach u and sigma
TALL_LAYERS = [("linear", r, 4, 1, {}) for r in (1100, 1536, 2048, 3000, 4097, 6000, 8193, 12000, 16385, 24576)]
SHAPES70 = [(16 + 8 * (i % 3), 8 + 8 * (i % 2), 3 if i % 5 else 1) for i in range(70)]   # tests/test_sn_gpu.py


def collect(dev, tolerate):
    import sn_checks as SC
    from studiogan_amd import _lib as L
    outs, pads = {}, {}
    for dtype, dn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        def tap(table):
            def f(stage, recs, work):
                torch.cuda.synchronize()
                outs[f"{table} {dn} {stage} work"] = work.cpu()
                for i, r in enumerate(recs):
                    for k in BUFS:
                        if r.get(k) is not None:
                            outs[f"{table} {dn} {stage} layer {i} {k}"] = r[k].detach().cpu()
                    if table == "WIDE_LAYERS" and r.get("fwd_d") is not None and r["cin_pad"] > r["cin"]:
                        pads[f"{table} {dn} {stage} layer {i} fwd_d"] = (max(r["rows"], r["rows_pad"]), r["RS"], r["cin"], r["cin_pad"])
            return f
        for table, layers in (("LAYERS", SC.LAYERS), ("WIDE_LAYERS", SC.WIDE_LAYERS), ("TALL_LAYERS", TALL_LAYERS)):
            rows = SC.run(dev, dtype, L, L.call, L.ptr, L.stream, layers=layers, tap=tap(table))
            bad = [(n, e, t) for n, e, t in rows if not e <= t]
            # (a build that leaves the padding unwritten fails the forward-image rows of the padded layers, and only those)
            assert not bad or (tolerate and table == "WIDE_LAYERS" and all(n.endswith("cin_pad w_fwd image") for n, _, _ in bad)), bad
            print(f"{table} {dn}: {len(rows)} rows against fp64, {len(bad)} outside their tolerance {[n for n, _, _ in bad]}")
        SC.forward_table(dev, dtype, L, L.call, L.ptr, L.stream, SHAPES70, seed=5, tap=tap("70 layers, one call"))
        SC.forward_table(dev, dtype, L, L.call, L.ptr, L.stream, SHAPES70, seed=5, split_at=37, tap=tap("70 layers, two calls"))
    return outs, pads


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--save")
    g.add_argument("--against")
    ap.add_argument("--parent-leaves-wide-padding", action="store_true")
    a = ap.parse_args()
    import studiogan_amd
    print("library:", studiogan_amd.LIB_PATH)
    outs, pads = collect(torch.device("cuda:0"), bool(a.save and a.parent_leaves_wide_padding))
    n_el = sum(t.numel() for t in outs.values())
    if a.save:
        torch.save(outs, a.save)
        print(f"saved {len(outs)} buffers, {n_el} elements, to {a.save}")
    else:
        ref = torch.load(a.against)
        assert ref.keys() == outs.keys(), f"the two runs cover different buffers: {sorted(set(ref) ^ set(outs))[:6]}"
        bad, excluded = [], 0
        for k, t in outs.items():
            x, y = bits(t), bits(ref[k])
            assert x.dtype == y.dtype and x.shape == y.shape, k
            if a.parent_leaves_wide_padding and k in pads:
                ro, RS, cin, cp = pads[k]
                keep = torch.ones(x.numel(), dtype=torch.bool)
                keep[:ro * RS * cp].view(ro, RS, cp)[:, :, cin:] = False
                excluded += int((~keep).sum())
                assert bool((t[~keep] == 0).all()), f"{k}: padding channels not zero in this build"
                x, y = x[keep], y[keep]
            if not torch.equal(x, y):
                bad.append(k)
                print("DIFFERS", k)
        assert not bad, f"{len(bad)} of {len(outs)} buffers differ from {a.against}"
        print(f"all {len(outs)} buffers, {n_el} elements, bit-identical to {a.against}" +
              (f" ({excluded} padding-channel elements of w_fwd on WIDE_LAYERS left out: zero here, unwritten there)" if a.parent_leaves_wide_padding else ""))
