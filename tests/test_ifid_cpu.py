"""Intra-class FID, host side: the oracle against the fixture (and the fixture against the REAL reference where its checkout is present), the C ABI of
csrc/frechet_small.hip, the argument checks that run before anything touches the device, and the fixed-label sampler."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu  # noqa: E402
import ifid_checks as IC  # noqa: E402
import ifid_ref as R  # noqa: E402
from oracle import ref_import  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
needs_emu = pytest.mark.skipif(not emu.available(), reason="host clang++ of the ROCm toolchain not found")
NEW_SYMBOLS = ("sg_seg_moments", "sg_seg_cross_gram", "sg_seg_nuclear_norm", "sg_seg_nuclear_fits", "sg_seg_nuclear_lds_budget")


@pytest.fixture(scope="module")
def fix():
    return dict(np.load(os.path.join(HERE, "golden", "ifid_small.npz")))


def test_oracle_reproduces_fixture(fix):
    """tests/ifid_ref.py on the fixture's rows gives the recorded oracle values (fp64 SVD: 1e-12), and those sit where the issue's CPU check found the formula
    against the reference's sqrtm route: 1e-7 relative, 1e-5 for the n = 2 class that takes the reference's eps branch."""
    assert fix["in/real"].dtype == np.float32 and fix["in/real"].shape == (sum(R.CLASS_SIZES), R.DIM)
    for lab in (fix["in/real_labels"], fix["in/fake_labels"]):
        assert tuple(np.bincount(lab)) == R.CLASS_SIZES
    got = R.intra_class(fix["in/real"], fix["in/real_labels"], fix["in/fake"], fix["in/fake_labels"], len(R.CLASS_SIZES))
    rel = np.abs(got - fix["exp/oracle"]) / np.abs(fix["exp/oracle"])
    assert rel.max() <= 1e-12, rel
    rel_ref = np.abs(fix["exp/oracle"] - fix["exp/ref"]) / np.abs(fix["exp/ref"])
    print("oracle against the reference, per class:", rel_ref)
    assert rel_ref[0] <= 1e-5 and rel_ref[1:].max() <= 1e-7, rel_ref


@pytest.mark.skipif(not ref_import.available(), reason="the reference checkout is not present")
def test_fixture_regenerates_from_the_reference(fix):
    """tests/make_golden_ifid.py run again: the same inputs bit for bit, the same oracle values, and the reference's values to 1e-9 (scipy's sqrtm on a singular
    product is not bit-stable across LAPACK builds; its distance from the exact value is 1e-8 and more, test above)."""
    import make_golden_ifid
    new = make_golden_ifid.compute()
    assert sorted(new) == sorted(fix)
    for k in fix:
        if k.startswith("in/"):
            assert np.array_equal(new[k], fix[k]) and new[k].dtype == fix[k].dtype, k
    assert np.abs(new["exp/oracle"] - fix["exp/oracle"]).max() <= 1e-12 * np.abs(fix["exp/oracle"]).max()
    assert (np.abs(new["exp/ref"] - fix["exp/ref"]) <= 1e-9 * np.abs(fix["exp/ref"])).all(), (new["exp/ref"], fix["exp/ref"])


def test_new_symbols_are_bound(sg):
    from studiogan_amd import _lib
    lib = sg.lib()
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sgamd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib._PROTOS and hasattr(lib, name) and name + "(" in hdr, name
    # the route predicate and the budget run on the host: every matrix up to 64 x 64 fits, 200 x 200 (320 KB of doubles) cannot
    assert all(lib.sg_seg_nuclear_fits(r, c) == 1 for r in range(1, 65) for c in range(r, 65))
    assert lib.sg_seg_nuclear_fits(200, 200) == 0
    budget = lib.sg_seg_nuclear_lds_budget()
    assert 64 * 64 * 8 < budget <= 160 * 1024
    # 128 KiB: the matrix, one norm per row and the sweep's measures -- 126 x 126 is the largest square
    assert budget == 128 * 1024 and lib.sg_seg_nuclear_fits(126, 126) == 1 and lib.sg_seg_nuclear_fits(128, 128) == 0


def test_route_predicate_keeps_wide_pairs_off_the_padded_square(sg):
    """takes_sample_route (host): fewer samples than dimensions -> sample route, but not when the matrix is beyond the LDS budget AND would be padded to a square of
    more than SQUARE_ROUTE_MAX rows (2000 fakes against 50000 real rows at 2048 dimensions: a 20 GB matrix); a few rows against many still fit the LDS kernel."""
    from studiogan_amd import metrics as M
    assert M.SQUARE_ROUTE_MAX == 4096
    assert M.takes_sample_route(50, 50, 2048) and M.takes_sample_route(1000, 1000, 2048) and M.takes_sample_route(1300, 1300, 1536)
    assert M.takes_sample_route(2000, 4096, 2048) and not M.takes_sample_route(2000, 4097, 2048) and not M.takes_sample_route(2000, 50000, 2048)
    assert M.takes_sample_route(2, 8000, 2048) and sg.lib().sg_seg_nuclear_fits(2, 8000) == 1          # 2 x 8000 doubles: 125 KiB, in LDS
    assert not M.takes_sample_route(65, 65, 64) and not M.takes_sample_route(3000, 2500, 2048)          # more samples than dimensions on both sides


def test_undersized_class_raises_value_error(sg, fix):
    """a class with fewer than 2 samples on either side is named, before anything is sent to a device"""
    from studiogan_amd import metrics as M
    real, rl, fake, fl = fix["in/real"], fix["in/real_labels"], fix["in/fake"], fix["in/fake_labels"]
    keep = np.ones(len(fl), dtype=bool)
    keep[np.nonzero(fl == 0)[0][0]] = False            # class 0 has 2 fakes: drop one
    with pytest.raises(ValueError, match=r"class 0: 2 real and 1 fake"):
        M.intra_class_frechet(real, rl, fake[keep], fl[keep], len(R.CLASS_SIZES))
    with pytest.raises(ValueError, match=r"class 6: 0 real and 0 fake"):
        M.intra_class_frechet(real, rl, fake, fl, len(R.CLASS_SIZES) + 1)
    with pytest.raises(ValueError, match="labels outside"):
        M.intra_class_frechet(real, rl, fake, fl, len(R.CLASS_SIZES) - 1)
    with pytest.raises(ValueError, match="class 3: 1 real samples"):
        M.calculate_intra_class_fid(None, None, real[:7], np.array([0, 0, 1, 1, 2, 2, 3]), 4, 8, 16)
    with pytest.raises(NotImplementedError):
        M.calculate_intra_class_fid(None, None, real, rl, len(R.CLASS_SIZES), 8, 16, world_size=2)


def test_y_sampler_fixed_label_and_default_draws(sg):
    """y_sampler: an int gives that label everywhere and draws NOTHING for the labels (reference src/utils/sample.py:56-57); the default draws exactly what
    sample_zy / sample_latents drew before the keyword existed: labels first, then the latents."""
    from studiogan_amd import metrics as M
    from studiogan_amd.worker import sample_latents, sample_zy
    for fn in (sample_zy, sample_latents):
        torch.manual_seed(11)
        ys_exp = torch.randint(low=0, high=10, size=(6,), dtype=torch.long)
        zs_exp = torch.randn(6, 16)
        torch.manual_seed(11)
        zs, ys = fn(6, 16, 10, "cpu")
        assert torch.equal(ys, ys_exp) and torch.equal(zs, zs_exp), fn.__name__
        torch.manual_seed(11)
        zs, ys = fn(6, 16, 10, "cpu", y_sampler="totally_random")
        assert torch.equal(ys, ys_exp) and torch.equal(zs, zs_exp), fn.__name__
        torch.manual_seed(11)
        z_first = torch.randn(6, 16)
        torch.manual_seed(11)
        zs, ys = fn(6, 16, 10, "cpu", y_sampler=7)
        assert ys.dtype == torch.long and ys.tolist() == [7] * 6 and torch.equal(zs, z_first), fn.__name__
        with pytest.raises(NotImplementedError):
            fn(6, 16, 10, "cpu", y_sampler="acending_all")
    g = torch.Generator().manual_seed(5)
    ys_exp, zs_exp = torch.randint(low=0, high=10, size=(4,), dtype=torch.long, generator=g), torch.randn(4, 8, generator=g)
    zs, ys = sample_zy(4, 8, 10, "cpu", generator=torch.Generator().manual_seed(5))
    assert torch.equal(ys, ys_exp) and torch.equal(zs, zs_exp)
    assert inspect.signature(M.generate_images_and_stack_features).parameters["y_sampler"].default == "totally_random"


# ---- the kernels themselves on the CPU interpreter (tests/hipemu), tiny shapes; the issue's shapes run on the GPU in tests/test_ifid_gpu.py --------------------
@pytest.fixture(scope="module")
def installed():
    import fullemu
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    with fullemu.Installed(dma_late=1, greedy=1, seed=5) as E:
        yield E
    torch.set_num_threads(n)


@needs_emu
def test_emulated_moments_and_cross_gram(installed):
    """C = 20: a k-tile tail; 66 rows: a second 64-row tile; (9, 3): b along the rows"""
    IC.moments_case(installed.L, torch.device("cpu"), 20, (2, 3, 9))
    IC.cross_gram_case(installed.L, torch.device("cpu"), 20, (2, 9, 66), (2, 3, 5))


@needs_emu
def test_emulated_nuclear_norm(installed):
    """an odd row count (zero row in LDS), more pairs than half waves (18 rows: 9 pairs for 8 half waves), more columns than a half wave (33)"""
    IC.nuclear_case(installed.L, torch.device("cpu"), [(2, 2), (7, 33), (18, 18)])
    IC.zero_row_case(installed.L, torch.device("cpu"))


@needs_emu
def test_emulated_distances_vs_reference_fixture(installed):
    """metrics.frechet_distance_from_features / intra_class_frechet on the fixture's three smallest classes (2, 7 and 24 samples)"""
    from studiogan_amd import metrics as M
    IC.fixture_case(M, torch.device("cpu"), classes=(0, 1, 2))


@needs_emu
def test_emulated_more_classes_than_one_launch_table(installed):
    """300 classes of 2 - 4 samples: every kernel's second launch (class offset k0 > 0 into mu / tr / nuc / M)"""
    from studiogan_amd import metrics as M
    IC.many_classes_case(M, torch.device("cpu"))
