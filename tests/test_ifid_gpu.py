"""GPU: the small-sample Frechet distance (csrc/frechet_small.hip, metrics.intra_class_frechet / calculate_intra_class_fid) against the fp64 oracle of
tests/ifid_ref.py and the fixture tests/golden/ifid_small.npz (the REAL reference's values, tests/make_golden_ifid.py). The checks and their bounds:
tests/ifid_checks.py. Nothing here reads the reference checkout."""
import numpy as np
import pytest
import torch

import ifid_checks as IC
import ifid_ref as R

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 33, 64, 65, 130)      # tile edges of the 64 x 64 cross-Gram tiles; odd and even row counts


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("C", [64, 100])      # 100: a k-tile tail (tiles of 16), and columns beyond the first 64 threads
def test_seg_moments_vs_oracle(sg, dev, C):
    IC.moments_case(sg._lib, dev, C, SIZES)


@pytest.mark.parametrize("C", [64, 100])
def test_seg_cross_gram_vs_oracle(sg, dev, C):
    IC.cross_gram_case(sg._lib, dev, C, SIZES, SIZES)


@pytest.mark.parametrize("C", [64, 100])
def test_seg_cross_gram_unequal_counts(sg, dev, C):
    """(7, 33): a along the rows; (50, 3): b along the rows (the smaller set), M is 3 x 50"""
    IC.cross_gram_case(sg._lib, dev, C, (7, 50), (33, 3))


def test_nuclear_norm_one_launch(sg, dev):
    IC.nuclear_case(sg._lib, dev, [(2, 2), (7, 33), (33, 33), (40, 40), (64, 64)])


def test_nuclear_norm_rows_of_zero_norm(sg, dev):
    IC.zero_row_case(sg._lib, dev)


def test_route_selection_and_padded_route(sg, dev):
    """64 x 64 takes the LDS kernel, 200 x 200 cannot; a 200-sample class (dim 256: still the sample route) goes through the padded square route of
    sg_jacobi_sweep / sg_row_norm_sum and agrees with the oracle, next to a class on the LDS route. More samples than dimensions: the moment route."""
    from studiogan_amd import metrics as M
    lib = sg.lib()
    assert lib.sg_seg_nuclear_fits(64, 64) == 1 and lib.sg_seg_nuclear_fits(200, 200) == 0
    fa, sega = IC.make_sets((200, 12), 256, seed=41)
    fb, segb = IC.make_sets((200, 9), 256, seed=42, shift=0.2, scale=1.3)
    la, lb = np.repeat([0, 1], [200, 12]), np.repeat([0, 1], [200, 9])
    stats = {}
    got = M.intra_class_frechet(fa, la, fb, lb, 2, stats=stats, device=dev)
    assert stats["route"] == ["square", "lds"] and max(stats["sweeps"]) <= 40, stats
    ref = R.intra_class(fa, la, fb, lb, 2)
    print("padded route:", got, ref, stats)
    assert (np.abs(got - ref) <= 1e-9 * np.abs(ref)).all(), (got, ref)
    rs = np.random.RandomState(5)
    xa, xb = R.relu_features(rs, 100, 16), R.relu_features(rs, 90, 16, 0.2, 1.3)      # min(n) > dim: both covariances positive definite
    got = M.frechet_distance_from_features(xa, xb, device=dev)
    assert abs(got - R.frechet(xa, xb)) <= 1e-9 * R.frechet(xa, xb)


def test_distances_vs_reference_fixture(sg, dev):
    from studiogan_amd import metrics as M
    IC.fixture_case(M, dev)


def test_more_classes_than_one_launch_table(sg, dev):
    from studiogan_amd import metrics as M
    IC.many_classes_case(M, dev)


class _PooledPixels:
    """stub eval model: 4 x 4 average-pooled pixels -> a fixed projection to 64 ReLU features; records every feature batch it returns"""

    def __init__(self, dev):
        g = torch.Generator().manual_seed(17)
        self.w = (torch.randn(48, 64, generator=g) * 0.5).to(dev)
        self.b = (torch.randn(64, generator=g) * 0.1).to(dev)
        self.seen = []

    def get_outputs(self, x, quantize=False):
        p = torch.nn.functional.adaptive_avg_pool2d(x.float(), 4).reshape(x.shape[0], -1)
        f = torch.relu(p @ self.w + self.b).contiguous()
        self.seen.append(f.clone())
        return f, f[:, :10].contiguous()


@pytest.mark.parametrize("trim", [False, True])
def test_calculate_intra_class_fid_end_to_end(sg, dev, trim):
    """A width-8 conditional BigGAN generator at 32 x 32, 10 classes with 2 .. 9 real samples, batches of 4: every generated batch carries ONE label, class c
    gets ceil(n_c / 4) batches (trim: the last one only n_c % 4 rows), exactly the first n_c rows are kept, and the per-class values are the oracle's on the
    rows the eval model returned."""
    from studiogan_amd import metrics as M
    from util import load_golden, sub
    from test_model_gpu import build_from_yaml
    fix, meta = load_golden("biggan32")
    G, _ = build_from_yaml(meta["yaml"], False, dev)
    G.load_state_dict({k: v.to(dev) for k, v in sub(fix, "G_init/").items()}, strict=True)
    G.eval()
    counts = (2, 3, 5, 4, 6, 9, 2, 7, 4, 8)
    rs = np.random.RandomState(23)
    real = R.relu_features(rs, sum(counts), 64, 0.1)
    real_labels = rs.permutation(np.repeat(np.arange(10), counts))
    batches = []

    def generator(zs, ys, eval=True):
        batches.append(ys.detach().cpu().numpy().copy())
        return G(zs, ys, eval=eval)

    model = _PooledPixels(dev)
    torch.manual_seed(3)
    mean, per_class = M.calculate_intra_class_fid(generator, model, torch.from_numpy(real).to(dev), real_labels, 10, 4, 40, trim_last_batch=trim, device=dev)
    assert per_class.shape == (10,) and per_class.dtype == np.float64 and abs(mean - per_class.mean()) <= 1e-12 * abs(mean)
    b = 0
    for c, n in enumerate(counts):
        nb = -(-n // 4)
        rows = []
        for i in range(nb):
            want = 4 if not trim or i < n // 4 else n % 4
            assert batches[b].shape == (want,) and (batches[b] == c).all(), (c, i, batches[b])
            rows.append(model.seen[b].cpu().numpy())
            b += 1
        kept = np.concatenate(rows)[:n]
        assert kept.shape[0] == n
        ref = R.frechet(real[real_labels == c], kept)
        assert abs(per_class[c] - ref) <= 1e-9 * abs(ref), (c, per_class[c], ref)
    assert b == len(batches) == len(model.seen)
