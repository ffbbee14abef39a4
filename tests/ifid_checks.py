"""Checks of csrc/frechet_small.hip and of metrics.intra_class_frechet against the fp64 oracle (tests/ifid_ref.py), written once for two runners:
tests/test_ifid_gpu.py (the GPU, the issue's shapes) and tests/test_ifid_cpu.py (the CPU interpreter of tests/hipemu, tiny shapes). Every output buffer is
carved out of a larger allocation filled with a sentinel, every input matrix out of one filled with NaN: a read or a write outside a matrix shows.

Bounds (fp64 unit roundoff u = 1.1e-16):
  mean         a sum of n <= 130 fp32 values in fp64: n u max|x| = 1.4e-14 max|x|                                   -> 1e-13 max|x|
  trace        a sum of positive terms, each with a few u of relative error, in another order than numpy's: (n + C / 256 + 8) u -> 1e-12 relative
  cross-Gram   a dot product over C <= 100 terms of centred values: C u |a_i| |b_j| = 1.1e-14 |a_i| |b_j|            -> 1e-13 max|a_i| max|b_j|
  nuclear norm 1e-12 relative against the SVD (set by the issue; the measure is below 1e-12 and the sum of the singular values is second-order accurate in it)
  distances    1e-9 relative against the oracle (the bound the square device route holds against its golden), and against the reference
               |got - ref| <= 2 |ref - oracle| + 1e-9 |ref| with both terms from the fixture (set by the issue)."""
import os

import numpy as np
import torch

import ifid_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.25e77
GUARD = 37      # elements on either side of a carved buffer (odd: the carved buffer is 8-byte aligned and no more)


def carve(n, dtype, dev, fill=SENTINEL):
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return big, big[GUARD:GUARD + n]


def guards_intact(big, n, fill=SENTINEL):
    f = torch.tensor(fill, dtype=big.dtype)
    return bool((big[:GUARD].cpu() == f).all()) and bool((big[GUARD + n:].cpu() == f).all())


def make_sets(sizes, C, seed, shift=0.0, scale=1.0):
    """class-sorted fp32 rows [sum sizes][C] and the int64 offsets"""
    rs = np.random.RandomState(seed)
    f = np.concatenate([R.relu_features(rs, n, C, shift + 0.05 * k, scale) for k, n in enumerate(sizes)])
    seg = np.zeros(len(sizes) + 1, dtype=np.int64)
    seg[1:] = np.cumsum(sizes)
    return f, seg


def seg_moments(L, f_dev, seg, C, dev):
    K = len(seg) - 1
    big_mu, mu = carve(K * C, torch.float64, dev)
    big_tr, tr = carve(K, torch.float64, dev)
    L.call("sg_seg_moments", L.ptr(f_dev), seg.ctypes.data, K, C, L.ptr(mu), L.ptr(tr), L.stream())
    assert guards_intact(big_mu, K * C) and guards_intact(big_tr, K), "sg_seg_moments wrote outside mu / tr"
    return mu.cpu().numpy().reshape(K, C), tr.cpu().numpy()


def moments_case(L, dev, C, sizes):
    f, seg = make_sets(sizes, C, seed=100 + C)
    mu, tr = seg_moments(L, torch.from_numpy(f).to(dev), seg, C, dev)
    for k in range(len(sizes)):
        x = f[seg[k]:seg[k + 1]]
        mu_ref, tr_ref = R.moments(x)
        e_mu, e_tr = np.abs(mu[k] - mu_ref).max() / np.abs(x).max(), abs(tr[k] - tr_ref) / tr_ref
        print(f"moments C={C} n={sizes[k]}: mean {e_mu:.2e} of max|x|, trace {e_tr:.2e} relative")
        assert e_mu <= 1e-13 and e_tr <= 1e-12, (C, sizes[k], e_mu, e_tr)


def cross_gram_case(L, dev, C, sizes_a, sizes_b):
    fa, sega = make_sets(sizes_a, C, seed=200 + C)
    fb, segb = make_sets(sizes_b, C, seed=300 + C, shift=0.2, scale=1.3)
    K = len(sizes_a)
    da, db = torch.from_numpy(fa).to(dev), torch.from_numpy(fb).to(dev)
    mua, _ = seg_moments(L, da, sega, C, dev)
    mub, _ = seg_moments(L, db, segb, C, dev)
    r, c = np.minimum(sizes_a, sizes_b), np.maximum(sizes_a, sizes_b)
    moff = np.zeros(K, dtype=np.int64)
    for k in range(1, K):
        moff[k] = moff[k - 1] + r[k - 1] * c[k - 1] + 5      # 5 sentinel elements between two matrices
    total = int(moff[-1] + r[-1] * c[-1])
    big, M = carve(total, torch.float64, dev)
    dmu = torch.from_numpy(np.stack([mua, mub])).to(dev).contiguous()
    L.call("sg_seg_cross_gram", L.ptr(da), sega.ctypes.data, L.ptr(dmu[0]), L.ptr(db), segb.ctypes.data, L.ptr(dmu[1]), K, C, L.ptr(M), moff.ctypes.data, L.stream())
    assert guards_intact(big, total), "sg_seg_cross_gram wrote outside M"
    h = M.cpu().numpy()
    for k in range(K):
        xa, xb = fa[sega[k]:sega[k + 1]], fb[segb[k]:segb[k + 1]]
        ref = R.cross_gram(xa, xb)
        assert ref.shape == (r[k], c[k])
        got = h[moff[k]:moff[k] + r[k] * c[k]].reshape(r[k], c[k])
        scale = np.linalg.norm(R.centred(xa)[1], axis=1).max() * np.linalg.norm(R.centred(xb)[1], axis=1).max()
        e = np.abs(got - ref).max() / scale
        print(f"cross-Gram C={C} ({sizes_a[k]}, {sizes_b[k]}): {e:.2e} of max|a_i| max|b_j|")
        assert e <= 1e-13, (C, sizes_a[k], sizes_b[k], e)
        if k + 1 < K:
            assert (h[moff[k] + r[k] * c[k]:moff[k + 1]] == SENTINEL).all(), "sg_seg_cross_gram wrote between two matrices"


def sample_matrices(shapes, C=64, seed=7):
    rs = np.random.RandomState(seed)
    return [R.cross_gram(R.relu_features(rs, r, C), R.relu_features(rs, c, C, 0.2, 1.3)) for r, c in shapes]


def nuclear_norm_launch(L, dev, mats, max_sweeps=40, tol=1e-12):
    """ONE sg_seg_nuclear_norm launch over `mats` (fp64 numpy matrices) laid out with NaN gaps; returns (nuc, offd, sweeps)"""
    K = len(mats)
    moff = np.zeros(K, dtype=np.int64)
    for k in range(1, K):
        moff[k] = moff[k - 1] + mats[k - 1].size + 3
    total = int(moff[-1] + mats[-1].size)
    host = np.full(total + 2 * GUARD, np.nan)
    for k, m in enumerate(mats):
        host[GUARD + moff[k]:GUARD + moff[k] + m.size] = m.reshape(-1)
    big = torch.from_numpy(host).to(dev)
    rows = np.array([m.shape[0] for m in mats], dtype=np.int32)
    cols = np.array([m.shape[1] for m in mats], dtype=np.int32)
    big_n, nuc = carve(K, torch.float64, dev)
    big_o, offd = carve(K, torch.float64, dev)
    big_s, sweeps = carve(K, torch.int32, dev, fill=-12345)
    L.call("sg_seg_nuclear_norm", L.ptr(big[GUARD:]), moff.ctypes.data, rows.ctypes.data, cols.ctypes.data, K, max_sweeps, float(tol),
           L.ptr(nuc), L.ptr(offd), L.ptr(sweeps), L.stream())
    assert guards_intact(big_n, K) and guards_intact(big_o, K) and guards_intact(big_s, K, -12345), "sg_seg_nuclear_norm wrote outside its outputs"
    assert np.array_equal(big.cpu().numpy().view(np.int64), host.view(np.int64)), "sg_seg_nuclear_norm changed M"
    return nuc.cpu().numpy(), offd.cpu().numpy(), sweeps.cpu().numpy()


def nuclear_case(L, dev, shapes):
    mats = sample_matrices(shapes)
    nuc, offd, sweeps = nuclear_norm_launch(L, dev, mats)
    for k, m in enumerate(mats):
        ref = R.nuclear_norm(m)
        e = abs(nuc[k] - ref) / ref
        print(f"nuclear norm {m.shape}: {e:.2e} relative, measure {offd[k]:.2e}, {sweeps[k]} sweeps")
        assert e <= 1e-12 and 1 <= sweeps[k] <= 40 and 0.0 <= offd[k] < 1e-12, (m.shape, e, offd[k], sweeps[k])
    return sweeps


def zero_row_case(L, dev):
    """rows of zero norm (an all-zero matrix; a zero row next to others; exactly dependent rows that a rotation turns into one): no NaN anywhere"""
    rs = np.random.RandomState(3)
    a = rs.randn(3, 5)
    a[1] = 0.0
    b = rs.randn(4, 6)
    b[3] = b[0]
    # two samples per class: the centred rows are x and -x, M = [[d, -d], [-d, d]] exactly. One rotation leaves a row that is rounding noise AND an exact
    # multiple of the other (with fused multiply-adds it is not 0): it must count as a zero row, not hold the scale-free measure at 1 for ever
    twos = [np.array([[d, -d], [-d, d]]) for d in (0.3, 3.14159e-3, 7.7, 1.2345e-9)]
    outer = np.outer([1.0, -0.5, 0.25], [3.0, -1.0, 2.0, 0.7])      # rank 1: every row a multiple of the first
    mats = [np.zeros((2, 2)), a, b, rs.randn(1, 4)] + twos + [outer]
    nuc, offd, sweeps = nuclear_norm_launch(L, dev, mats)
    print("rows of zero norm / dependent rows: sweeps", sweeps, "measures", offd)
    assert np.isfinite(nuc).all() and np.isfinite(offd).all(), (nuc, offd)
    assert nuc[0] == 0.0 and offd[0] == 0.0 and sweeps[0] == 1
    for k in range(1, len(mats)):
        ref = R.nuclear_norm(mats[k])
        assert abs(nuc[k] - ref) <= 1e-12 * ref and offd[k] < 1e-12 and sweeps[k] <= 40, (k, nuc[k], ref, offd[k], sweeps[k])
    # one sweep rotates, the next finds the remainder at rounding level; one more if the remainder was a few ulps large
    assert (sweeps[4:8] <= 3).all(), sweeps


def load_fixture():
    return dict(np.load(os.path.join(HERE, "golden", "ifid_small.npz")))


def assert_against_fixture(got, fix, what):
    ref, orc = fix["exp/ref"], fix["exp/oracle"]
    for k in range(len(ref)):
        e_o, e_r, bound = abs(got[k] - orc[k]) / abs(orc[k]), abs(got[k] - ref[k]), 2.0 * abs(ref[k] - orc[k]) + 1e-9 * abs(ref[k])
        print(f"{what} class {k}: {got[k]:.12f}  {e_o:.2e} relative from the oracle; |got - ref| = {e_r:.2e} (bound {bound:.2e})")
        assert e_o <= 1e-9, (what, k, got[k], orc[k])
        assert e_r <= bound, (what, k, got[k], ref[k], bound)


def fixture_case(M, dev, classes=None):
    """frechet_distance_from_features per class, and intra_class_frechet over all classes (one chunk; one class per chunk), against tests/golden/ifid_small.npz"""
    fix = load_fixture()
    real, rl, fake, fl = fix["in/real"], fix["in/real_labels"], fix["in/fake"], fix["in/fake_labels"]
    K = len(R.CLASS_SIZES)
    if classes is not None:      # (the interpreter's subset: the fixture's small classes, relabelled 0 ..)
        keep_r, keep_f = np.isin(rl, classes), np.isin(fl, classes)
        remap = {c: i for i, c in enumerate(classes)}
        real, fake = real[keep_r], fake[keep_f]
        rl, fl = np.array([remap[c] for c in rl[keep_r]]), np.array([remap[c] for c in fl[keep_f]])
        fix = dict(fix)
        fix["exp/ref"], fix["exp/oracle"] = fix["exp/ref"][list(classes)], fix["exp/oracle"][list(classes)]
        K = len(classes)
    single = [M.frechet_distance_from_features(real[rl == k], fake[fl == k], device=dev) for k in range(K)]
    assert all(isinstance(v, float) for v in single)
    assert_against_fixture(single, fix, "frechet_distance_from_features")
    stats = {}
    batched = M.intra_class_frechet(real, rl, fake, fl, K, stats=stats, device=dev)
    assert batched.dtype == np.float64 and batched.shape == (K,)
    assert_against_fixture(batched, fix, "intra_class_frechet")
    small = [k for k in range(K) if M.takes_sample_route((rl == k).sum(), (fl == k).sum(), real.shape[1])]      # (the 65-sample class has more samples than dimensions: moment route)
    assert stats["route"] == ["lds"] * len(small) and max(stats["sweeps"]) <= 40, stats
    # the sample-route classes alone, relabelled 0 ..: ONE chunk of all of them against one class per chunk (workspace_bytes = 1: later chunks start at k0 > 0)
    keep_r, keep_f = np.isin(rl, small), np.isin(fl, small)
    remap = np.full(K, -1)
    remap[small] = np.arange(len(small))
    args = (torch.from_numpy(real[keep_r]), torch.from_numpy(remap[rl[keep_r]]), torch.from_numpy(fake[keep_f]), torch.from_numpy(remap[fl[keep_f]]), len(small))
    stats = {}
    one = M.intra_class_frechet(*args, stats=stats, device=dev)
    assert stats["route"] == ["lds"] * len(small)
    assert (np.abs(one - batched[small]) <= 1e-13 * np.abs(one)).all()
    chunked = M.intra_class_frechet(*args, workspace_bytes=1, device=dev)
    # (the kernels do the same arithmetic per class whatever the chunk; only the host-side sum of |mu_a - mu_b|^2 runs over another tensor shape)
    assert (np.abs(chunked - one) <= 1e-13 * np.abs(one)).all(), "one class per chunk computes the same values as one chunk"


def many_classes_case(M, dev, K=300, C=8):
    """More classes than one launch's table holds (256 segments, 80 cross-Gram classes, 200 matrices): the later launches of each kernel index mu / tr / nuc / M with
    a class offset. 2 - 4 samples a side, drawn independently (either set may be the smaller one), all in ONE chunk; against the oracle at the distances' bound."""
    rs = np.random.RandomState(77)
    na, nb = rs.randint(2, 5, size=K), rs.randint(2, 5, size=K)
    la, lb = np.repeat(np.arange(K), na), np.repeat(np.arange(K), nb)
    real = R.relu_features(rs, la.size, C, 0.3) + (0.01 * la[:, None]).astype(np.float32)
    fake = R.relu_features(rs, lb.size, C, 0.6, 1.3) + (0.01 * lb[:, None]).astype(np.float32)
    pa, pb = rs.permutation(la.size), rs.permutation(lb.size)
    stats = {}
    got = M.intra_class_frechet(real[pa], la[pa], fake[pb], lb[pb], K, stats=stats, device=dev)
    ref = R.intra_class(real, la, fake, lb, K)
    e = np.abs(got - ref) / np.abs(ref)
    print(f"{K} classes in one chunk: worst {e.max():.2e} relative from the oracle (class {int(e.argmax())}), sweeps up to {max(stats['sweeps'])}")
    assert stats["route"] == ["lds"] * K and e.max() <= 1e-9, (int(e.argmax()), e.max())
