"""fp64 brute-force k-nearest-neighbour oracle of the stage-two tests (test infrastructure; the product never imports it).

``brute_force`` is pinned to sklearn 1.7.2 by tests/test_two_stage_host.py on the fixtures tests/golden/knn_*.npz and is then the
reference for every larger case (tests/test_gpu_two_stage.py).  Its rules: difference-form Euclidean distances in float64, neighbours
ascending, equal distances to the lower training index (a stable sort), the most frequent class among the k, a tied vote to the
smallest class.
"""
import numpy as np
import torch


def distances(X, Q):
    """float64 [n_query, n_train], difference form (no |q|^2 + |x|^2 - 2 q.x)"""
    X64, Q64 = torch.from_numpy(np.asarray(X, dtype=np.float64)), torch.from_numpy(np.asarray(Q, dtype=np.float64))
    return torch.cdist(Q64, X64, compute_mode="donot_use_mm_for_euclid_dist").numpy()


def brute_force(X, y, Q, k, d=None):
    """-> (pred labels [nq], idx [nq, k], dist [nq, k]) in float64"""
    d = distances(X, Q) if d is None else d
    y = np.asarray(y)
    classes, cls = np.unique(y, return_inverse=True)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    votes = np.zeros((d.shape[0], classes.size), dtype=np.int64)
    np.add.at(votes, (np.arange(d.shape[0])[:, None], cls[idx]), 1)
    return classes[np.argmax(votes, axis=1)], idx, np.take_along_axis(d, idx, axis=1)       # (argmax: the first maximum)


def tau(D):
    """twice the worst-case rounding bound of a sequential fp32 sum of D squared differences followed by a square root:
    (D + 2) 2^-22, relative"""
    return (D + 2) * 2.0 ** -22


def undecided(d, y, k, band):
    """bool [nq]: the training rows whose distance lies within band[q] of the k-th distance carry more than one label (a swap of rows
    inside the band could change the vote)"""
    y = np.asarray(y)
    dk = np.sort(d, axis=1)[:, k - 1:k]
    near = np.abs(d - dk) <= np.asarray(band).reshape(-1, 1)
    lo = np.where(near, y[None, :], y.max() + 1).min(axis=1)
    hi = np.where(near, y[None, :], y.min() - 1).max(axis=1)
    return lo != hi


def synthetic(seed, n_train, n_query, D, C, offset):
    """numpy.random.default_rng(seed): labels of both sets, centres 0.5 N(0,1) [C, D], rows offset + centre[label] + N(0,1), fp32"""
    rng = np.random.default_rng(seed)
    y, yq = rng.integers(0, C, n_train), rng.integers(0, C, n_query)
    centre = 0.5 * rng.normal(size=(C, D))
    X = (offset + centre[y] + rng.normal(size=(n_train, D))).astype(np.float32)
    Q = (offset + centre[yq] + rng.normal(size=(n_query, D))).astype(np.float32)
    return X, y, Q, yq
