"""Writes tests/golden/ifid_small.npz: seeded fp32 features (dim 64) of 6 classes with 2, 7, 24, 33, 40 and 65 samples on each side, and per class
  exp/ref     what the REAL reference computes for intra-class FID (src/worker.py:1380-1465): np.mean / np.cov of the real rows in fp64 as src/metrics/fid.py:94-97,
              fid.calculate_moments(fake_feats=...) for the fakes (fid.py:67-69,96-97: the mean of the fp32 stack), then fid.frechet_inception_distance (scipy sqrtm);
  exp/oracle  tests/ifid_ref.py on the same rows (fp64 SVD of the centred cross-Gram matrix).

    python tests/make_golden_ifid.py      (needs the reference checkout: imported through oracle/ref_import.py)

Data only; TEST INFRASTRUCTURE ONLY."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import ifid_ref as R      # noqa: E402

OUT = os.path.join(HERE, "golden", "ifid_small.npz")


def inputs():
    """rows in a seeded shuffled order (the product sorts them by class), per class a shifted / rescaled fake distribution"""
    rs = np.random.RandomState(20261019)
    real, fake, labels = [], [], []
    for k, n in enumerate(R.CLASS_SIZES):
        real.append(R.relu_features(rs, n, R.DIM, shift=0.1 * k))
        fake.append(R.relu_features(rs, n, R.DIM, shift=0.1 * k + 0.15, scale=1.2))
        labels += [k] * n
    labels = np.array(labels, dtype=np.int64)
    pr, pf = rs.permutation(len(labels)), rs.permutation(len(labels))
    return {"in/real": np.concatenate(real)[pr], "in/real_labels": labels[pr], "in/fake": np.concatenate(fake)[pf], "in/fake_labels": labels[pf]}


def compute():
    from oracle import ref_import as RI
    RI._prepare()
    fid = importlib.import_module("metrics.fid")
    fix = inputs()
    ref = []
    for k, n in enumerate(R.CLASS_SIZES):
        acts = fix["in/real"][fix["in/real_labels"] == k].astype(np.float64)
        mu, sigma = np.mean(acts, axis=0), np.cov(acts, rowvar=False)
        ff = torch.from_numpy(fix["in/fake"][fix["in/fake_labels"] == k])
        m2, s2 = fid.calculate_moments(data_loader="N/A", eval_model=None, num_generate=n, batch_size=8, quantize=True, world_size=1, DDP=False,
                                       disable_tqdm=True, fake_feats=ff)
        ref.append(float(np.real(fid.frechet_inception_distance(mu, sigma, m2, s2))))
    fix["exp/ref"] = np.array(ref, dtype=np.float64)
    fix["exp/oracle"] = R.intra_class(fix["in/real"], fix["in/real_labels"], fix["in/fake"], fix["in/fake_labels"], len(R.CLASS_SIZES))
    return fix


if __name__ == "__main__":
    fix = compute()
    np.savez_compressed(OUT, **fix)
    for k, n in enumerate(R.CLASS_SIZES):
        r, o = fix["exp/ref"][k], fix["exp/oracle"][k]
        print(f"class {k} (n = {n}): reference {r:.12f}  oracle {o:.12f}  relative difference {abs(r - o) / abs(r):.2e}")
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB")
