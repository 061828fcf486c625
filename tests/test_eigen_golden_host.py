"""The host coarsening and the fp64 restatement (tests/eigen_ref.py) pinned to the reference's own EigenGCN outputs
(tests/golden/eigen_*.npz, scripts/gen_golden_eigen.py); no GPU needed."""
import numpy as np
import pytest
import torch

import eigen_golden as G
import eigen_ref as R
from two_stage_gnn_amd import eigen_pool as ep


def _same_span(got, ref, ev, s, count, tol=1e-6):
    """columns j < count of one cluster (s members): equal where the eigenvalue of column min(j, s-1) is simple, else the same
    projector onto the columns of that eigenvalue"""
    idx = np.minimum(np.arange(count), s - 1)
    for j in range(count):
        grp = np.abs(ev - ev[idx[j]]) < 1e-8
        if grp.sum() == 1:
            np.testing.assert_allclose(got[:, j], ref[:, j], atol=tol)
        else:
            cols = sorted({int(i) for i in idx if grp[i]})
            js = [int(np.nonzero(idx == c)[0][0]) for c in cols]
            Pg, Pr = got[:, js] @ got[:, js].T, ref[:, js] @ ref[:, js].T
            np.testing.assert_allclose(Pg, Pr, atol=tol)


@pytest.mark.parametrize("name", G.NAMES)
def test_coarsen_matches_the_reference(name):
    g = G.load(name)
    c = G.cfg(g)
    L = len(c["pool_sizes"])
    for b, n in enumerate(g["sizes"]):
        A = g["adj"][b, :n, :n]
        labs = [g["labels_%d" % i][b][g["labels_%d" % i][b] >= 0] for i in range(L)]
        r = ep.coarsen(A, c["pool_sizes"], normalize=bool(c["normalize"]), labels=labs)
        assert r is not None
        cur = A
        for i in range(L):
            k, ni = int(g["sizes_%d" % i][b]), cur.shape[0]
            np.testing.assert_array_equal(r["graphs"][i + 1], g["adj_pooled_%d" % i][b, :k, :k])      # pooled adjacency: exact
            lab = labs[i]
            for cl in range(k):
                mem = np.nonzero(lab == cl)[0]
                ref = np.stack([g["pool_%d_%d" % (i, j)][b, mem, cl] for j in range(5)], axis=1)
                ev = np.linalg.eigvalsh(ep.laplacian(cur[np.ix_(mem, mem)], bool(c["normalize"])))
                _same_span(r["coef"][i][mem], ref, ev, len(mem), 5)
                # nothing outside the cluster's column
                for j in range(5):
                    assert np.count_nonzero(np.delete(g["pool_%d_%d" % (i, j)][b, mem, :k], cl, axis=1)) == 0
            cur = r["graphs"][i + 1]
        ref = np.stack([g["final_%d" % j][b, :cur.shape[0]] for j in range(4)], axis=1)
        _same_span(r["final"], ref, np.linalg.eigvalsh(ep.laplacian(cur, bool(c["normalize"]))), cur.shape[0], 4)


@pytest.mark.parametrize("name", G.NAMES)
def test_dense_inputs_and_l1_match_the_reference(name):
    """eigen_pool.dense_inputs (the sampler's padded tensors, --norm l1 included) rebuilt from coarsen() = what the reference fed"""
    g = G.load(name)
    c = G.cfg(g)
    L = len(c["pool_sizes"])
    res = []
    for b, n in enumerate(g["sizes"]):
        labs = [g["labels_%d" % i][b][g["labels_%d" % i][b] >= 0] for i in range(L)]
        r = ep.coarsen(g["adj"][b, :n, :n], c["pool_sizes"], normalize=bool(c["normalize"]), labels=labs)
        for i in range(L):                          # the reference's vectors (a degenerate eigenspace may have another basis)
            for j in range(5):
                r["coef"][i][:, j] = g["pool_%d_%d" % (i, j)][b, :len(labs[i]), :].sum(axis=1)
        r["final"] = np.stack([g["final_%d" % j][b, :r["graphs"][L].shape[0]] for j in range(4)], axis=1)
        res.append(r)
    got = ep.dense_inputs(res, c["nmax"], c["J"], c["Jf"], norm="l1" if c["l1"] else None)
    want = G.model_inputs(g)
    np.testing.assert_array_equal(got[0].numpy(), want[1].numpy())
    for i in range(L):
        np.testing.assert_array_equal(got[1][i].numpy(), want[2][i].numpy())
    assert got[2] == want[3] and got[3] == want[4]
    for i, mats in want[5].items():
        for j, m in enumerate(mats):
            np.testing.assert_allclose(got[4][i][j].numpy(), m.numpy(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", G.NAMES)
def test_restatement_reproduces_the_reference(name):
    g = G.load(name)
    c = G.cfg(g)
    p = G.params(g)
    x, adj, pooled, nn0, nnl, pm = G.model_inputs(g)
    logits = R.wave_pooling_forward(p, x.double(), adj.double(), pooled, nn0, nnl, pm, c["num_layers"], c["pool_sizes"], c["J"],
                                    c["Jf"], concat=c["concat"], mask=c["mask"], con_final=c["con_final"],
                                    n_linear=len(c["pred_hidden"]) + 1)
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(g["label"]))
    loss.backward()
    np.testing.assert_allclose(logits.detach().numpy(), g["logits"], rtol=1e-4, atol=1e-4)
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4
    for k, v in p.items():
        ref = g["g." + k]
        got = v.grad.numpy() if v.grad is not None else np.zeros_like(ref)
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-4, err_msg=k)


def test_fixtures_cover_the_edge_cases():
    gs = {n: G.load(n) for n in G.NAMES}
    cs = {n: G.cfg(g) for n, g in gs.items()}
    assert {1, 3} <= {c["J"] for c in cs.values()}
    assert any(len(c["pool_sizes"]) == 2 for c in cs.values())
    assert {(0, 0), (0, 1), (2, 0), (2, 1)} <= {(min(c["Jf"], 2), c["con_final"]) for c in cs.values() if c["Jf"] in (0, 2)}
    assert any(not c["concat"] for c in cs.values()) and any(c["mask"] == 0 for c in cs.values())
    assert any(c["normalize"] for c in cs.values()) and any(c["l1"] for c in cs.values())
    assert any(len(g["sizes"]) == 1 and int(g["sizes"][0]) == cs[n]["nmax"] for n, g in gs.items())
    small = zero_entry = all_zero = False
    for n, g in gs.items():
        c = cs[n]
        for i in range(len(c["pool_sizes"])):
            lab = g["labels_%d" % i]
            for b in range(lab.shape[0]):
                cnt = np.bincount(lab[b][lab[b] >= 0])
                small |= bool((cnt < c["J"]).any())
                n_b = int((lab[b] >= 0).sum())
                P = np.stack([g["pool_%d_%d" % (i, j)][b, :n_b] for j in range(c["J"])])     # [J, n, K]
                own = np.take_along_axis(P, lab[b][None, :n_b, None].repeat(c["J"], 0), axis=2)[..., 0]
                zero_entry |= bool((own == 0).any())
                all_zero |= bool((own == 0).all(axis=0).any())
    assert small and zero_entry and all_zero
