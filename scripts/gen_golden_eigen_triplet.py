#!/usr/bin/env python3
"""Golden vectors of the reference's EigenGCN triplet step (test infrastructure; never imported by the product path).

Same rules and stubs as scripts/gen_golden_eigen.py (whose helpers it imports): the reference's Code/eigengcn is imported read-only
with ``.cuda()`` turned into the identity and SpectralClustering replaced by fixed chunk labels.  For every case it builds three
``.graph`` dicts the way the reference's sampler fills them (graph_sampler.py:130-176) from the reference's own
``Graphs(...).coarsening_pooling``, runs the reference's ``tripletnet(model, args)``, ``MarginRankingLoss(margin=1.5)`` with target
-1 and backward (train_triplet.py:292-317), and stores the dicts' arrays, the cluster labels, parameters, both distances, the three
embeddings, the loss and every parameter gradient as data-only fixtures tests/golden/triplet_eigen_*.npz.  (The name does not start
with ``eigen_``: tests/eigen_golden.py lists every ``eigen_*.npz`` as a fixture of the B-graph classification step.)

Every fixture has an active hinge (loss > 0) and a non-zero gradient on every conv and pred_model weight: the seed of a case is the
first one from its start value that gives both (asserted).

Usage:  python scripts/gen_golden_eigen_triplet.py REFERENCE_ROOT        (rewrites tests/golden/triplet_eigen_*.npz)
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_eigen as GE  # noqa: E402

MARGIN = 1.5

CASES = {
    "triplet_eigen_j1": dict(J=1, Jf=0, con_final=1, pool_sizes=[4], sizes=[17, 10, 14], nmax=20),
    "triplet_eigen_j2_final": dict(J=2, Jf=1, con_final=1, pool_sizes=[4], sizes=[16, 13, 18], nmax=18),
    "triplet_eigen_two_levels": dict(J=1, Jf=0, con_final=0, pool_sizes=[3, 2], sizes=[18, 14, 16], nmax=18),
    "triplet_eigen_jf2_nomask": dict(J=2, Jf=2, con_final=1, mask=0, pool_sizes=[3], sizes=[13, 9, 16], nmax=16),
    "triplet_eigen_linear": dict(J=2, Jf=1, con_final=1, pool_sizes=[4], sizes=[12, 19, 15], nmax=19, pred_hidden=[]),
    # anchor and positive the SAME object: dist_p = |eps| sqrt(E), so the hinge is active only if dist_n < margin.  Independent random
    # graphs under randn * 0.5 parameters lie further apart than 1.5 (120 seeds searched: smallest dist_n 2.37), so the negative is
    # the anchor's graph with features moved by 0.05 * randn
    "triplet_eigen_same_ap": dict(J=2, Jf=1, con_final=1, pool_sizes=[4], sizes=[15, 15, 15], nmax=16, same_ap=1, neg_noise=0.05),
}


class _G:
    """stands for the networkx graph object whose ``.graph`` dict the reference reads"""

    def __init__(self, d):
        self.graph = d


def graph_dict(cp, rng, gen, n, N, cfg, F_in):
    """one graph's dict as graph_sampler.py:130-176 fills it, + the labels the clustering stub handed out"""
    J, Jf, L = cfg["J"], cfg["Jf"], len(cfg["pool_sizes"])
    A = GE.ring_graph(rng, n)
    g = cp.Graphs(A, cfg["pool_sizes"])
    del GE._GIVEN[:]
    with contextlib.redirect_stdout(io.StringIO()):
        ok = g.coarsening_pooling(0)
    assert ok == 1
    d, labels = {}, []
    adj = np.zeros((N, N))
    adj[:n, :n] = A
    feats = np.zeros((N, F_in), dtype=np.float32)
    feats[:n] = torch.randn(n, F_in, generator=gen).numpy()
    d.update(adj=adj, feats=feats, num_nodes=n, assign_feats=feats.copy())
    for i in range(L):
        k = g.graphs[i + 1].shape[0]
        d["num_nodes_%d" % (i + 1)] = k
        P = np.zeros((N, N))
        P[:k, :k] = np.asarray(g.graphs[i + 1].todense(), dtype=np.float64)
        d["adj_pool_%d" % (i + 1)] = P
        for j in range(J):
            m = np.asarray(g.layer2pooling_matrices[i][j].todense(), dtype=np.float64)
            P = np.zeros((N, N))
            P[:m.shape[0], :m.shape[1]] = m
            d["pool_adj_%d_%d" % (i, j)] = P
        labels.append(GE._GIVEN[i].copy())
    for j in range(Jf):
        m = np.asarray(g.layer2pooling_matrices[L][j].todense(), dtype=np.float64)
        P = np.zeros((N, N))
        P[:m.shape[0], :m.shape[1]] = m
        d["pool_adj_%d_%d" % (L, j)] = P
    return d, labels


def run_case(cp, enc, tn, cfg, seed):
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    J, Jf, N = cfg["J"], cfg["Jf"], cfg["nmax"]
    F_in, H, E, layers, label_dim = 7, 12, 8, 3, 6
    pred_hidden = cfg.get("pred_hidden", [10])
    dicts, labels = [], []
    for n in cfg["sizes"]:
        d, lab = graph_dict(cp, rng, gen, n, N, cfg, F_in)
        dicts.append(d)
        labels.append(lab)
    objs = [_G(d) for d in dicts]
    if cfg.get("same_ap"):
        objs[1], dicts[1], labels[1] = objs[0], dicts[0], labels[0]
    if cfg.get("neg_noise"):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in dicts[0].items()}
        n = d["num_nodes"]
        d["feats"][:n] += cfg["neg_noise"] * torch.randn(n, F_in, generator=gen).numpy()
        d["assign_feats"] = d["feats"].copy()
        objs[2], dicts[2], labels[2] = _G(d), d, labels[0]

    class Args:
        bias = True
        con_final = cfg["con_final"]
        pool_sizes = "_".join(str(s) for s in cfg["pool_sizes"])
        num_pool_matrix = J
        num_pool_final_matrix = Jf
    with contextlib.redirect_stdout(io.StringIO()):
        m = enc.WavePoolingGcnEncoder(N, F_in, H, E, label_dim, layers, num_pool_matrix=J, num_pool_final_matrix=Jf,
                                      pool_sizes=cfg["pool_sizes"], pred_hidden_dims=pred_hidden, concat=True, bn=True,
                                      mask=cfg.get("mask", 1), args=Args())
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
    net = tn.tripletnet(m, Args())
    with contextlib.redirect_stdout(io.StringIO()):
        dist_p, dist_n, ea, e_p, en = net(*objs)
    loss = torch.nn.MarginRankingLoss(margin=MARGIN)(dist_p, dist_n, torch.full_like(dist_p, -1.0))
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy() for k, p in m.named_parameters()}
    active = float(loss.item()) > 0 and all(np.any(v != 0) for k, v in grads.items() if k.endswith("weight"))
    out = dict(J=J, Jf=Jf, con_final=cfg["con_final"], mask=cfg.get("mask", 1), nmax=N, num_layers=layers, hidden=H, emb=E,
               label_dim=label_dim, pred_hidden=np.asarray(pred_hidden, dtype=np.int64), pool_sizes=np.asarray(cfg["pool_sizes"]),
               same_ap=int(cfg.get("same_ap", 0)), margin=np.float32(MARGIN), seed=seed,
               dist_p=dist_p.detach().numpy(), dist_n=dist_n.detach().numpy(),
               embed=torch.cat([ea, e_p, en]).detach().numpy(), loss=np.float32(loss.item()))
    for t, (d, lab) in enumerate(zip(dicts, labels)):
        for k, v in d.items():
            if k != "assign_feats":                          # (read by the reference, never used)
                out["t%d.%s" % (t, k)] = np.asarray(v)
        for i, l in enumerate(lab):
            out["t%d.labels_%d" % (t, i)] = l
    for k, v in m.state_dict().items():
        out["p." + k] = v.detach().numpy().copy()
    for k, v in grads.items():
        out["g." + k] = v
    return out, active


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.join(sys.argv[1], "Code", "eigengcn")
    if not os.path.isdir(ref_dir):
        sys.exit("no Code/eigengcn under %s" % sys.argv[1])
    cp, enc = GE._import_reference(ref_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        import tripletnet as tn
    for s, (name, cfg) in enumerate(CASES.items()):
        for seed in range(300 + 10 * s, 310 + 10 * s):
            out, active = run_case(cp, enc, tn, cfg, seed)
            if active:
                break
        assert active, "%s: no seed with an active hinge and non-zero weight gradients" % name
        path = os.path.join(GE.OUT_DIR, name + ".npz")
        np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
        print("wrote", path, "seed %d loss %.4f" % (seed, float(out["loss"])), "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
