"""eigen_triplet without a GPU: the fixtures of the reference's own EigenGCN tripletnet (tests/golden/triplet_eigen_*.npz, written by
scripts/gen_golden_eigen_triplet.py), the fp64 restatement as their arbiter, and the host pack of a ``.graph`` dict.

  1. tests/eigen_ref.py three times at B = 1 in fp64 + torch distances and MarginRankingLoss(1.5) reproduces every fixture (the
     tolerances of tests/test_eigen_golden_host.py: outputs and loss rtol = atol = 1e-4, gradients rtol 2e-3 / atol 2e-4);
  2. every fixture has an active hinge and a non-zero gradient on every conv and pred_model weight;
  3. pack_host on every fixture's dicts, checked in numpy: cluster labels, the dense matrices rebuilt from the compact form, the
     bucket rule; ValueError on each malformed input;
  4. args / model mismatches raise.
"""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eigen_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("triplet_eigen_") and f.endswith(".npz"))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def cfg(g):
    return dict(J=int(g["J"]), Jf=int(g["Jf"]), con_final=int(g["con_final"]), mask=int(g["mask"]), nmax=int(g["nmax"]),
                num_layers=int(g["num_layers"]), hidden=int(g["hidden"]), emb=int(g["emb"]), label_dim=int(g["label_dim"]),
                pred_hidden=[int(v) for v in g["pred_hidden"]], pool_sizes=[int(v) for v in g["pool_sizes"]],
                same_ap=int(g["same_ap"]), margin=float(g["margin"]))


class GraphObj:
    """stands for the networkx graph whose ``.graph`` dict the triplet loop hands over"""

    def __init__(self, d):
        self.graph = d


def graph_dicts(g):
    """the three ``.graph`` dicts of a fixture (anchor and positive the same dict where the fixture says so) + their labels"""
    out, labels = [], []
    for t in range(3):
        pre = "t%d." % t
        d = {k[len(pre):]: (int(v) if v.ndim == 0 else v) for k, v in g.items() if k.startswith(pre) and ".labels_" not in k}
        labels.append([g["%slabels_%d" % (pre, i)] for i in range(len(g["pool_sizes"]))])
        out.append(d)
    if int(g["same_ap"]):
        out[1] = out[0]
    return out, labels


def args_of(c):
    return types.SimpleNamespace(bias=True, con_final=c["con_final"], pool_sizes="_".join(str(s) for s in c["pool_sizes"]),
                                 num_pool_matrix=c["J"], num_pool_final_matrix=c["Jf"])


def params(g, dtype=torch.float64):
    p = {k[2:]: torch.tensor(v, dtype=dtype).requires_grad_(True) for k, v in g.items() if k.startswith("p.")}
    return p


def _ref_params(p):
    """eigen_ref.pred reads pred_model.{0,2,..}: a single nn.Linear's keys (pred_model.weight) under the name it expects"""
    q = dict(p)
    if "pred_model.weight" in p:
        q["pred_model.0.weight"], q["pred_model.0.bias"] = p["pred_model.weight"], p["pred_model.bias"]
    return q


def dense_inputs(d, c, dtype):
    """one ``.graph`` dict -> the arguments of the model at B = 1, as the reference's tripletnet builds them"""
    L, J, Jf = len(c["pool_sizes"]), c["J"], c["Jf"]
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).unsqueeze(0)
    pm = {i: [t(d["pool_adj_%d_%d" % (i, j)]) for j in range(J)] for i in range(L)}
    if Jf:
        pm[L] = [t(d["pool_adj_%d_%d" % (L, j)]) for j in range(Jf)]
    return (t(d["feats"]), t(d["adj"]), [t(d["adj_pool_%d" % (i + 1)]) for i in range(L)], [int(d["num_nodes"])],
            [[int(d["num_nodes_%d" % (i + 1)])] for i in range(L)], pm)


def ref_step(p, dicts, c, dtype, margin=None):
    """the restatement three times at B = 1, both distances, the margin loss and its backward -> (dist_p, dist_n, [e_a, e_p, e_n], loss)"""
    q = _ref_params(p)
    es = []
    for d in dicts:
        x, adj, pooled, n0, nl, pm = dense_inputs(d, c, dtype)
        es.append(R.wave_pooling_forward(q, x, adj, pooled, n0, nl, pm, c["num_layers"], c["pool_sizes"], c["J"], c["Jf"], concat=True,
                                         mask=c["mask"], con_final=c["con_final"], n_linear=len(c["pred_hidden"]) + 1))
    dp, dn = F.pairwise_distance(es[0], es[1], 2), F.pairwise_distance(es[0], es[2], 2)
    loss = torch.nn.MarginRankingLoss(margin=c["margin"] if margin is None else margin)(dp, dn, torch.full_like(dp, -1.0))
    loss.backward()
    return dp.detach(), dn.detach(), [e.detach() for e in es], loss.detach()


def test_fixture_list():
    assert len(NAMES) >= 6
    cs = [cfg(load(n)) for n in NAMES]
    assert any(c["J"] == 1 and c["Jf"] == 0 for c in cs) and any(c["J"] == 2 and c["Jf"] == 1 and c["con_final"] == 1 for c in cs)
    assert any(len(c["pool_sizes"]) == 2 and c["con_final"] == 0 for c in cs) and any(c["Jf"] == 2 and c["mask"] == 0 for c in cs)
    assert any(c["pred_hidden"] == [] for c in cs) and any(c["same_ap"] for c in cs)


# ------------------------------------------------------------------------------------------------ 1. the restatement is a valid arbiter
@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_tripletnet(name):
    g = load(name)
    c = cfg(g)
    p = params(g)
    dicts, _ = graph_dicts(g)
    dp, dn, es, loss = ref_step(p, dicts, c, torch.float64)
    np.testing.assert_allclose(dp.numpy(), g["dist_p"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dn.numpy(), g["dist_n"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(torch.cat(es).numpy(), g["embed"], rtol=1e-4, atol=1e-4)
    assert abs(float(loss) - float(g["loss"])) < 1e-4
    for k, v in p.items():
        ref = g["g." + k]
        got = v.grad.numpy() if v.grad is not None else np.zeros_like(ref)
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-4, err_msg=k)


# ------------------------------------------------------------------------------------------------ 2. the fixtures are not vacuous
@pytest.mark.parametrize("name", NAMES)
def test_fixture_has_an_active_hinge(name):
    g = load(name)
    assert float(g["loss"]) > 0.0
    weights = [k for k in g if k.startswith("g.") and k.endswith(".weight")]
    assert any(k.startswith("g.conv_first") for k in weights) and any(k.startswith("g.pred_model") for k in weights)
    assert any("after_pool" in k for k in weights)
    for k in weights:
        assert np.any(g[k] != 0), k


# ------------------------------------------------------------------------------------------------ 3. pack_host
@pytest.mark.parametrize("name", NAMES)
def test_pack_host_is_the_compact_form_of_the_dicts(name):
    from two_stage_gnn_amd import eigen_triplet as ET
    g = load(name)
    c = cfg(g)
    L, J, Jf, N = len(c["pool_sizes"]), c["J"], c["Jf"], c["nmax"]
    dicts, labels = graph_dicts(g)
    for d, labs in zip(dicts, labels):
        h = ET.pack_host(d, L, J, Jf)
        assert h["nmax"] == N and h["n"] == [int(d["num_nodes"])] + [int(d["num_nodes_%d" % (i + 1)]) for i in range(L)]
        for i, (rp, col, val, sym) in enumerate(h["graphs"]):           # the CSRs rebuilt to dense: exact
            n = h["n"][i]
            A = np.zeros((N, N), dtype=np.float32)
            rows = np.repeat(np.arange(n), np.diff(rp))
            A[rows, col] = val
            want = np.asarray(d["adj"] if i == 0 else d["adj_pool_%d" % i], dtype=np.float32)
            np.testing.assert_array_equal(A, want)
            assert rp.dtype == np.int32 and col.dtype == np.int32 and rp.shape == (n + 1,)
            assert sym == bool(np.array_equal(want, want.T))
            assert all(np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0) for r in range(n))        # columns ascending inside a row
        for i, lv in enumerate(h["levels"]):
            n, k = h["n"][i], h["n"][i + 1]
            clus, coef = lv["cluster_of"], lv["coef"]
            assert clus.shape == (n,) and coef.shape == (n, J)
            dense = np.stack([np.asarray(d["pool_adj_%d_%d" % (i, j)], dtype=np.float32) for j in range(J)])
            own = dense[:, np.arange(n), labs[i]].T                    # the entries in the row's own cluster column
            zero = (own == 0).all(axis=1)
            np.testing.assert_array_equal(clus, np.where(zero, -1, labs[i]))
            for j in range(J):                                           # the dense matrices rebuilt from the compact form: exact
                P = np.zeros((N, N), dtype=np.float32)
                a = clus >= 0
                P[np.nonzero(a)[0], clus[a]] = coef[a, j]
                np.testing.assert_array_equal(P, dense[j])
            assert not coef[~(clus >= 0)].any()
            bptr, members = lv["bptr"], lv["members"]                   # bucket 0: unassigned rows, bucket c + 1: cluster c, rows ascending
            assert bptr.shape == (k + 2,) and bptr[0] == 0 and bptr[-1] == n and sorted(members) == list(range(n))
            for b in range(k + 1):
                mem = members[bptr[b]:bptr[b + 1]]
                assert np.all(np.diff(mem) > 0) and np.all(clus[mem] == b - 1)
        if Jf:
            nL = h["n"][L]
            want = np.stack([np.asarray(d["pool_adj_%d_%d" % (L, j)], dtype=np.float32)[:nL, 0] for j in range(Jf)], axis=1)
            np.testing.assert_array_equal(h["final"], want)
        else:
            assert h["final"] is None


def test_pack_host_rejects_malformed_dicts():
    from two_stage_gnn_amd import eigen_triplet as ET
    g = load("triplet_eigen_j2_final")
    c = cfg(g)
    L, J, Jf = len(c["pool_sizes"]), c["J"], c["Jf"]
    good = graph_dicts(g)[0][0]
    ET.pack_host(good, L, J, Jf)
    n, k = int(good["num_nodes"]), int(good["num_nodes_1"])

    def broken(key, fn):
        d = dict(good)
        d[key] = fn(np.array(good[key], copy=True))
        return d

    def poke(r, col, v=0.5):
        def fn(a):
            a[r, col] = v
            return a
        return fn
    row = int(np.nonzero(np.asarray(good["pool_adj_0_0"])[:n].any(axis=1))[0][0])
    own = int(np.nonzero(np.asarray(good["pool_adj_0_0"])[row])[0][0])
    cases = {
        "column >= pooled count": broken("pool_adj_0_1", poke(row, k)),
        "two columns in one row": broken("pool_adj_0_0", poke(row, (own + 1) % k)),
        "two columns across the J matrices": broken("pool_adj_0_1", poke(row, (own + 1) % k)),
        "non-zero in a row >= n": broken("pool_adj_0_0", poke(n, 0)) if n < c["nmax"] else None,
        "pooling matrix not [Nmax, Nmax]": broken("pool_adj_0_0", lambda a: a[:-1, :-1]),
        "pooled adjacency not [Nmax, Nmax]": broken("adj_pool_1", lambda a: a[:, :-1]),
        "final matrix not [Nmax, Nmax]": broken("pool_adj_1_0", lambda a: a[:-1]),
        "final matrix with a second column": broken("pool_adj_1_0", poke(0, 1)),
    }
    assert cases["non-zero in a row >= n"] is not None
    for what, d in cases.items():
        with pytest.raises(ValueError):
            ET.pack_host(d, L, J, Jf)
            pytest.fail("accepted: " + what)
    with pytest.raises(ValueError):
        ET.pack_host({k_: v for k_, v in good.items() if k_ != "pool_adj_0_1"}, L, J, Jf)


# ------------------------------------------------------------------------------------------------ 4. args must agree with the model
def test_args_must_agree_with_the_model():
    from two_stage_gnn_amd import eigen_encoders as EE
    from two_stage_gnn_amd import eigen_triplet as ET
    c = cfg(load("triplet_eigen_j2_final"))
    a = args_of(c)
    m = EE.WavePoolingGcnEncoder(c["nmax"], 7, c["hidden"], c["emb"], c["label_dim"], c["num_layers"], num_pool_matrix=c["J"],
                                 num_pool_final_matrix=c["Jf"], pool_sizes=c["pool_sizes"], pred_hidden_dims=c["pred_hidden"], args=a)
    net = ET.tripletnet(m, a)
    assert net.model is m and (net.L, net.J, net.Jf) == (1, 2, 1)
    for field, bad in (("pool_sizes", "4_2"), ("pool_sizes", "3"), ("num_pool_matrix", 1), ("num_pool_final_matrix", 0)):
        b = args_of(c)
        setattr(b, field, bad)
        with pytest.raises(ValueError):
            ET.tripletnet(m, b)
