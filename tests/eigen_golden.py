"""Loading the reference's EigenGCN fixtures (tests/golden/eigen_*.npz, written by scripts/gen_golden_eigen.py)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("eigen_") and f.endswith(".npz"))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def cfg(g):
    return dict(J=int(g["J"]), Jf=int(g["Jf"]), con_final=int(g["con_final"]), concat=bool(g["concat"]), mask=int(g["mask"]),
                normalize=int(g["normalize"]), l1=int(g["l1"]), nmax=int(g["nmax"]), num_layers=int(g["num_layers"]),
                hidden=int(g["hidden"]), emb=int(g["emb"]), label_dim=int(g["label_dim"]),
                pred_hidden=[int(v) for v in g["pred_hidden"]], pool_sizes=[int(v) for v in g["pool_sizes"]])


def model_inputs(g):
    """(x, adj, adj_pooled_list, batch_num_nodes, batch_num_nodes_list, pool_matrices_dic) as the reference model consumed them"""
    c = cfg(g)
    L, J, Jf = len(c["pool_sizes"]), c["J"], c["Jf"]
    B, N = g["adj"].shape[0], c["nmax"]
    pm = {}
    for i in range(L):
        pm[i] = [torch.from_numpy(g["in_pool_%d_%d" % (i, j)] if c["l1"] else g["pool_%d_%d" % (i, j)]) for j in range(J)]
    if Jf:
        mats = []
        for j in range(Jf):
            if c["l1"]:
                mats.append(torch.from_numpy(g["in_pool_%d_%d" % (L, j)]))
            else:
                P = np.zeros((B, N, N))
                P[:, :, 0] = g["final_%d" % j]
                mats.append(torch.from_numpy(P))
        pm[L] = mats
    return (torch.from_numpy(g["x"]), torch.from_numpy(g["adj"]), [torch.from_numpy(g["adj_pooled_%d" % i]) for i in range(L)],
            [int(s) for s in g["sizes"]], [[int(s) for s in g["sizes_%d" % i]] for i in range(L)], pm)


def params(g, dtype=torch.float64, requires_grad=True):
    return {k[2:]: torch.tensor(v, dtype=dtype).requires_grad_(requires_grad) for k, v in g.items() if k.startswith("p.")}
