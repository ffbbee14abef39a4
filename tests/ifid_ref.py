"""fp64 numpy oracle of the small-sample Frechet distance (csrc/frechet_small.hip, metrics.intra_class_frechet): centre the rows, form A B^T, take its singular
values with np.linalg.svd. Shared by tests/test_ifid_cpu.py, tests/test_ifid_gpu.py and tests/make_golden_ifid.py. TEST INFRASTRUCTURE ONLY."""
import numpy as np

CLASS_SIZES = (2, 7, 24, 33, 40, 65)      # tests/golden/ifid_small.npz
DIM = 64


def centred(x):
    """(mu, A) with A = (x - mu) / sqrt(n - 1), fp64: np.cov(x, rowvar=False) == A.T @ A"""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(0)
    return mu, (x - mu) / np.sqrt(x.shape[0] - 1.0)


def moments(x):
    """(mu [C], tr cov)"""
    mu, a = centred(x)
    return mu, float((a * a).sum())


def cross_gram(xa, xb):
    """A B^T with the smaller set along the rows (ties: a)"""
    _, a = centred(xa)
    _, b = centred(xb)
    return a @ b.T if a.shape[0] <= b.shape[0] else b @ a.T


def nuclear_norm(m):
    return float(np.linalg.svd(np.asarray(m, dtype=np.float64), compute_uv=False).sum())


def frechet(xa, xb):
    mua, tra = moments(xa)
    mub, trb = moments(xb)
    d = mua - mub
    return float(d.dot(d) + tra + trb - 2.0 * nuclear_norm(cross_gram(xa, xb)))


def intra_class(real, real_labels, fake, fake_labels, num_classes):
    real_labels, fake_labels = np.asarray(real_labels), np.asarray(fake_labels)
    return np.array([frechet(real[real_labels == k], fake[fake_labels == k]) for k in range(num_classes)], dtype=np.float64)


def relu_features(rs, n, dim, shift=0.0, scale=1.0):
    """seeded fp32 rows that look like pooled post-ReLU activations: non-negative, about half of them zero"""
    return np.maximum(rs.randn(n, dim) * scale + shift, 0.0).astype(np.float32)
