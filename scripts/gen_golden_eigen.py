#!/usr/bin/env python3
"""Golden vectors of the reference's EigenGCN (test infrastructure; never imported by the product path).

Runs only where a checkout of the reference exists (its root is the argument).  It imports Code/eigengcn read-only, with ``.cuda()`` turned into the
identity inside this process, the ``community`` package stubbed and SpectralClustering replaced by a stub that hands out fixed
cluster labels (contiguous chunks of the node order).  For every case it runs the reference's own
coarsening (``Graphs(...).coarsening_pooling``), builds the padded model inputs the way its sampler does (graph_sampler.py:102-175,
``--norm l1`` included), runs ``WavePoolingGcnEncoder`` forward + ``loss`` + backward, and stores inputs, coarsening outputs,
parameters, logits, loss and parameter gradients as data-only fixtures tests/golden/eigen_*.npz.  No reference source is copied.

Usage:  python scripts/gen_golden_eigen.py REFERENCE_ROOT        (rewrites tests/golden/eigen_*.npz)
"""
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn as nn

OUT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

_GIVEN = []           # the labels every call of the stub's fit handed out, in call order


class _FixedClustering:
    def __init__(self, n_clusters, **kw):
        self.k = n_clusters

    def fit(self, A):
        n = A.shape[0]
        self.labels_ = np.arange(n, dtype=np.int64) * self.k // n       # contiguous chunks of the node order
        _GIVEN.append(self.labels_.copy())
        return self


def _import_reference(ref_dir):
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self
    sys.modules.setdefault("community", types.ModuleType("community"))
    sys.path.insert(0, ref_dir)
    warnings.filterwarnings("ignore")
    with contextlib.redirect_stdout(io.StringIO()):
        import coarsen_pooling_with_last_eigen_padding as cp
        import encoders
    cp.SpectralClustering = _FixedClustering
    return cp, encoders


def ring_graph(rng, n, extra=2):
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, (i + 1) % n] = 1
    for _ in range(extra * n // 2):
        a, b = rng.integers(0, n, 2)
        if a != b:
            A[a, b] = 1
    return np.maximum(A, A.T)


def zero_entry_graph():
    """12 nodes, chunks of 3: cluster 0 a path 0-1-2 (its second eigenvector has a zero at node 1), cluster 1 an edge 3-4 and a node 5
    with no edge inside its cluster (with normalize = 1 the first eigenvector is zero there), clusters 2 and 3 triangles"""
    A = np.zeros((12, 12))
    for u, v in [(0, 1), (1, 2), (3, 4), (6, 7), (7, 8), (6, 8), (9, 10), (10, 11), (9, 11), (2, 3), (5, 6), (8, 9), (11, 0), (4, 7)]:
        A[u, v] = A[v, u] = 1
    return A


CASES = {
    # name: config; graphs from ring_graph unless "graphs" says otherwise
    "eigen_j1": dict(J=1, Jf=0, con_final=1, pool_sizes=[4], sizes=[17, 10], nmax=20),
    "eigen_j3_small": dict(J=3, Jf=2, con_final=1, pool_sizes=[2], sizes=[12, 9], nmax=14),       # clusters of 2 < J: padding
    "eigen_zero": dict(J=1, Jf=2, con_final=0, normalize=1, pool_sizes=[3], sizes=[12, 12], nmax=12, graphs="zero"),
    "eigen_norm": dict(J=2, Jf=1, con_final=1, normalize=1, pool_sizes=[4], sizes=[16, 13], nmax=18),
    "eigen_two_levels": dict(J=2, Jf=0, con_final=0, pool_sizes=[3, 2], sizes=[20, 14], nmax=20),
    "eigen_final_con0": dict(J=2, Jf=2, con_final=0, pool_sizes=[4], sizes=[15, 18], nmax=18),
    "eigen_noconcat": dict(J=2, Jf=1, con_final=1, concat=False, pool_sizes=[4], sizes=[14, 19], nmax=19),
    "eigen_nomask": dict(J=2, Jf=2, con_final=1, mask=0, pool_sizes=[3], sizes=[13, 9], nmax=16),
    "eigen_l1": dict(J=2, Jf=1, con_final=1, l1=1, pool_sizes=[4], sizes=[16, 12], nmax=16),
    "eigen_b1_full": dict(J=3, Jf=1, con_final=1, pool_sizes=[4], sizes=[22], nmax=22),
}


def gen_case(cp, enc, name, cfg, seed):
    from sklearn import preprocessing
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    J, Jf, L, N = cfg["J"], cfg["Jf"], len(cfg["pool_sizes"]), cfg["nmax"]
    normalize, l1 = cfg.get("normalize", 0), cfg.get("l1", 0)
    sizes = cfg["sizes"]
    B = len(sizes)
    out = {}
    adj = np.zeros((B, N, N))
    pooled = [np.zeros((B, N, N)) for _ in range(L)]
    labels = [np.full((B, N), -1, dtype=np.int64) for _ in range(L)]
    sizes_l = [np.zeros(B, dtype=np.int64) for _ in range(L)]
    raw = {(i, j): np.zeros((B, N, N)) for i in range(L) for j in range(5)}
    fin = {j: np.zeros((B, N)) for j in range(4)}
    inp = {(i, j): np.zeros((B, N, N)) for i in range(L) for j in range(J)}
    inp.update({(L, j): np.zeros((B, N, N)) for j in range(Jf)})
    for b, n in enumerate(sizes):
        A = zero_entry_graph() if cfg.get("graphs") == "zero" else ring_graph(rng, n)
        adj[b, :n, :n] = A
        g = cp.Graphs(A, cfg["pool_sizes"])
        del _GIVEN[:]
        with contextlib.redirect_stdout(io.StringIO()):
            ok = g.coarsening_pooling(normalize)
        assert ok == 1, (name, b)
        for i in range(L):
            k = g.graphs[i + 1].shape[0]
            ni = g.graphs[i].shape[0]
            sizes_l[i][b] = k
            pooled[i][b, :k, :k] = np.asarray(g.graphs[i + 1].todense(), dtype=np.float64)
            for j in range(5):
                P = np.asarray(g.layer2pooling_matrices[i][j].todense(), dtype=np.float64)
                raw[i, j][b, :ni, :k] = P
                if j < J:
                    inp[i, j][b, :ni, :k] = preprocessing.normalize(P, norm="l1", axis=0) if l1 else P
            labels[i][b, :ni] = _GIVEN[i]
        nL = g.graphs[L].shape[0]
        for j in range(4):
            col = np.asarray(g.layer2pooling_matrices[L][j].todense(), dtype=np.float64)
            fin[j][b, :nL] = col[:, 0]
            if j < Jf:
                inp[L, j][b, :nL, :1] = preprocessing.normalize(col, norm="l1", axis=0) if l1 else col
    F_in, H, E, layers, label_dim = 7, 12, 8, 3, 3
    x = torch.zeros(B, N, F_in)
    for b, n in enumerate(sizes):
        x[b, :n] = torch.randn(n, F_in, generator=gen)
    y = torch.tensor(rng.integers(0, label_dim, B))

    class Args:
        bias = True
        con_final = cfg["con_final"]
    with contextlib.redirect_stdout(io.StringIO()):
        m = enc.WavePoolingGcnEncoder(N, F_in, H, E, label_dim, layers, num_pool_matrix=J, num_pool_final_matrix=Jf,
                                      pool_sizes=cfg["pool_sizes"], pred_hidden_dims=[10], concat=cfg.get("concat", True), bn=True,
                                      mask=cfg.get("mask", 1), args=Args())
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
    pm = {i: [torch.from_numpy(inp[i, j]) for j in range(J if i < L else Jf)] for i in range(L + (1 if Jf else 0))}
    ypred = m(x, torch.from_numpy(adj).float(), [torch.from_numpy(p) for p in pooled], list(sizes),
              [list(s) for s in sizes_l], pm)
    loss = m.loss(ypred, y)
    loss.backward()
    out.update(J=J, Jf=Jf, con_final=cfg["con_final"], concat=int(cfg.get("concat", True)), mask=cfg.get("mask", 1),
               normalize=normalize, l1=l1, nmax=N, num_layers=layers, hidden=H, emb=E, label_dim=label_dim, pred_hidden=np.array([10]),
               pool_sizes=np.asarray(cfg["pool_sizes"]), sizes=np.asarray(sizes, dtype=np.int64), x=x.numpy(), adj=adj,
               label=y.numpy(), logits=ypred.detach().numpy(), loss=np.float32(loss.item()))
    for i in range(L):
        out["adj_pooled_%d" % i] = pooled[i]
        out["sizes_%d" % i] = sizes_l[i]
        out["labels_%d" % i] = labels[i]
        for j in range(5):
            out["pool_%d_%d" % (i, j)] = raw[i, j]
    for j in range(4):
        out["final_%d" % j] = fin[j]
    if l1:
        for (i, j), v in inp.items():
            out["in_pool_%d_%d" % (i, j)] = v
    for k, v in m.state_dict().items():
        out["p." + k] = v.detach().numpy().copy()
    for k, p in m.named_parameters():
        out["g." + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy()
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.join(sys.argv[1], "Code", "eigengcn")
    if not os.path.isdir(ref_dir):
        sys.exit("no Code/eigengcn under %s" % sys.argv[1])
    cp, enc = _import_reference(ref_dir)
    for s, (name, cfg) in enumerate(CASES.items()):
        gen_case(cp, enc, name, cfg, 100 + s)


if __name__ == "__main__":
    main()
