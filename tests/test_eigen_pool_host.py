"""EigenGCN host coarsening (two_stage_gnn_amd.eigen_pool.coarsen) against a per-cluster loop restatement of the reference's
coarsen_pooling_with_last_eigen_padding.py; no GPU needed."""
import numpy as np
import pytest

from two_stage_gnn_amd import eigen_pool as ep


def ring_plus(rng, n, extra=2):
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, (i + 1) % n] = 1
    for _ in range(extra * n // 2):
        a, b = rng.integers(0, n, 2)
        if a != b:
            A[a, b] = 1
    return np.maximum(A, A.T)


def lap(W, normalize):
    d = W.sum(axis=0)
    if not normalize:
        return np.diag(d) - W
    d = 1 / np.sqrt(d + np.spacing(0.0))
    return np.eye(len(d)) - d[:, None] * W * d[None, :]


def loop_level(A, lab, normalize, count=5):
    """one level the reference's way: cluster by cluster, column by column"""
    n, K = len(lab), lab.max() + 1
    P = np.zeros((count, n, K))
    for c in range(K):
        mem = [v for v in range(n) if lab[v] == c]
        _, U = np.linalg.eigh(lap(A[np.ix_(mem, mem)], normalize))
        for j in range(count):
            jj = min(j, len(mem) - 1)
            u = U[:, jj] * (-1 if U[0, jj] < 0 else 1)
            P[j, mem, c] = u
    Ac = np.zeros((K, K))
    for u in range(n):
        for v in range(n):
            if lab[u] != lab[v]:
                Ac[lab[u], lab[v]] += A[u, v]
    return P, Ac


def projector_close(got, ref, tol=1e-6):
    """columns equal up to the basis of a degenerate eigenspace: compare the projectors onto their span"""
    Pg, Pr = got @ np.linalg.pinv(got), ref @ np.linalg.pinv(ref)
    return np.abs(Pg - Pr).max() < tol


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("seed,n,pool_sizes", [(0, 23, [4]), (1, 40, [5, 2]), (2, 9, [3])])
def test_coarsen_matches_loop_restatement(seed, n, pool_sizes, normalize):
    rng = np.random.default_rng(seed)
    A = ring_plus(rng, n)

    def labels(Al, k, level):
        return np.arange(Al.shape[0]) * k // Al.shape[0]
    r = ep.coarsen(A, pool_sizes, normalize=normalize, labels=labels)
    assert r is not None
    cur = A
    for i, _ in enumerate(pool_sizes):
        lab = r["labels"][i]
        P, Ac = loop_level(cur, lab, normalize)
        np.testing.assert_array_equal(r["graphs"][i + 1], Ac)          # pooled adjacency: exact
        for c in range(lab.max() + 1):
            mem = lab == c
            for j in range(5):
                got, ref = r["coef"][i][mem, j], P[j, mem, c]
                if np.abs(got - ref).max() > 1e-6:                       # degenerate spectrum: the eigenspace must agree
                    ev = np.linalg.eigvalsh(lap(cur[np.ix_(mem, mem)], normalize))
                    jj = min(j, mem.sum() - 1)
                    same = np.abs(ev - ev[jj]) < 1e-8
                    _, U = np.linalg.eigh(lap(cur[np.ix_(mem, mem)], normalize))
                    assert same.sum() > 1 and abs(np.linalg.norm(got) - 1) < 1e-9
                    assert projector_close(np.column_stack([got] + [U[:, same]]), U[:, same])
        cur = Ac
    _, U = np.linalg.eigh(lap(cur, normalize))
    for j in range(4):
        jj = min(j, cur.shape[0] - 1)
        ref = U[:, jj] * (-1 if U[0, jj] < 0 else 1)
        if np.abs(r["final"][:, j] - ref).max() > 1e-6:
            ev = np.linalg.eigvalsh(lap(cur, normalize))
            assert (np.abs(ev - ev[jj]) < 1e-8).sum() > 1


def test_padding_rule_repeats_the_last_eigenvector():
    A = ring_plus(np.random.default_rng(3), 12)
    r = ep.coarsen(A, [4], labels=[np.arange(12) // 3])                  # clusters of 3 < 5 matrices
    c = r["coef"][0]
    np.testing.assert_array_equal(c[:, 2], c[:, 3])
    np.testing.assert_array_equal(c[:, 2], c[:, 4])


def test_rejections():
    A = ring_plus(np.random.default_rng(4), 10)
    lab = np.arange(10) // 2
    lab[9] = 5                                                           # a singleton cluster
    assert ep.coarsen(A, [2], labels=[lab]) is None
    # a last coarsened graph of one node
    assert ep.coarsen(A, [10], labels=[np.zeros(10, dtype=int)]) is None


def test_l1_normalisation_divides_each_column_by_its_l1_norm():
    coef = np.array([[1.0, -2.0], [3.0, 2.0], [0.5, 0.0], [-0.5, 0.0]])
    lab = np.array([0, 0, 1, 1])
    got = ep.l1_normalize(coef, lab)
    np.testing.assert_allclose(got, [[0.25, -0.5], [0.75, 0.5], [0.5, 0.0], [-0.5, 0.0]])
    np.testing.assert_allclose(ep.l1_normalize(coef[:, :1]), coef[:, :1] / 5.0)


def test_sklearn_clustering_path():
    pytest.importorskip("sklearn")
    A = ring_plus(np.random.default_rng(5), 30, extra=1)
    r = ep.coarsen(A, [5], labels=None, random_state=0)
    assert r is None or (r["graphs"][1].shape[0] == 6 and r["coef"][0].shape == (30, 5))


def test_restatement_pool_is_the_dense_product():
    import torch
    import eigen_ref as R
    rng = np.random.default_rng(6)
    A = ring_plus(rng, 16)
    r = ep.coarsen(A, [4], labels=[np.arange(16) // 4])
    adj, pooled, nn0, nnl, pm = ep.dense_inputs([r], 16, 3, 2)
    x = torch.from_numpy(rng.standard_normal((1, 16, 5)))
    y = R.pool(pm[0], x)
    for j in range(3):
        for c in range(4):
            mem = np.arange(16) // 4 == c
            want = (r["coef"][0][mem, j:j + 1] * x[0].numpy()[mem]).sum(0)
            np.testing.assert_allclose(y[0, c, j * 5:(j + 1) * 5].numpy(), want, rtol=1e-12, atol=1e-12)
    assert float(y[0, 4:].abs().max()) == 0.0
