#!/usr/bin/env python3
"""Golden vectors of the reference's triplet step around its GAT encoder (test infrastructure; never imported by the product path).

Same rules and stubs as oracle/gen_golden.py (whose helpers it imports) for the GAT encoder fixtures: the reference's
Code/sage+gat+diffpool is imported read-only with ``.cuda()`` turned into the identity and the ``DGATHead_V3`` name the constructor of
``DGATLayer`` trips over defined as an empty class.  For both ``final_dim`` modes it builds ONE ``DGATEncoderGraph`` (Nmax 16, 2
layers x 2 heads x 8) and four triplets of graph objects whose ``.graph`` dicts are filled as cross_val.py fills them, runs the
reference's own ``tripletnet(model)`` on each, ``MarginRankingLoss(margin)`` with target -1 and backward (train_triplet.py:235-277),
and stores the state dict and, per triplet, the three graphs, the five outputs, the loss and every parameter gradient as data-only
fixtures tests/golden/triplet_gat_{output_dim,classes}.npz.

The set holds a graph with n == Nmax (no padded row) and a graph with an isolated real node (an edge-less column that is not padding).
Every stored triplet has an active hinge (loss > 0); the script refuses to write otherwise.

Usage:  python scripts/gen_golden_gat_triplet.py REFERENCE_ROOT        (rewrites tests/golden/triplet_gat_*.npz)
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as GG  # noqa: E402

NMAX, FIN, HID, EMB, LAB = 16, 6, 8, 8, 2
MARGIN = 5.0
TRIPLETS = [[16, 9, 12], [7, 14, 10], [11, 16, 5], [13, 8, 15]]         # (16 == Nmax: no padded row)
ISOLATED = {(0, 2): 4, (3, 1): 0}                                       # (triplet, graph) -> a real node that loses all its edges
CASES = {"triplet_gat_output_dim": "output_dim", "triplet_gat_classes": "number_classes"}


class _G:
    """stands for the networkx graph object whose ``.graph`` dict the reference reads"""

    def __init__(self, d):
        self.graph = d


def graph_dict(gen, n, isolated=None):
    x, adj, _ = GG.make_batch(gen, 1, NMAX, FIN, sizes=[n], p_edge=0.3)
    a = adj[0].numpy().copy()
    if isolated is not None:
        a[isolated, :] = 0.0
        a[:, isolated] = 0.0
    f = x[0].numpy().copy()
    return {"adj": a, "feats": f, "num_nodes": n, "assign_feats": f.copy()}


def run_case(gat, tn, final_dim, seed):
    gen = torch.Generator().manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = gat.DGATEncoderGraph(FIN, HID, EMB, LAB, None, num_layers=2, num_heads=[2, 2], neg_input_slopes=[0.2, 0.2],
                                 dropouts=[0.0, 0.0], final_dim=final_dim)
    GG.randomise_(m, gen, 0.4)
    net = tn.tripletnet(m)
    crit = torch.nn.MarginRankingLoss(margin=MARGIN)
    out = dict(dims=np.array([FIN, HID, EMB, LAB]), nmax=NMAX, num_layers=2, heads=np.array([2, 2]), final_dim=np.array(final_dim),
               margin=np.float32(MARGIN), seed=seed, n_triplets=len(TRIPLETS), **GG.sd_np(m))
    for t, sizes in enumerate(TRIPLETS):
        dicts = [graph_dict(gen, n, ISOLATED.get((t, j))) for j, n in enumerate(sizes)]
        m.zero_grad(set_to_none=True)
        dist_p, dist_n, ea, e_p, en = net(*[_G(d) for d in dicts])
        loss = crit(dist_p, dist_n, torch.full_like(dist_p, -1.0))
        loss.backward()
        assert float(loss.item()) > 0, "triplet %d of %s: the hinge is not active (loss = 0): nothing is written" % (t, final_dim)
        for j, d in enumerate(dicts):
            out["t%d.g%d.adj" % (t, j)] = d["adj"].astype(np.float32)
            out["t%d.g%d.feats" % (t, j)] = d["feats"].astype(np.float32)
            out["t%d.g%d.num_nodes" % (t, j)] = np.int64(d["num_nodes"])
        out["t%d.dist_p" % t] = dist_p.detach().numpy().copy()
        out["t%d.dist_n" % t] = dist_n.detach().numpy().copy()
        out["t%d.embed" % t] = torch.cat([ea, e_p, en]).detach().numpy().copy()
        out["t%d.loss" % t] = np.float32(loss.item())
        out.update(GG.grads_np(m, prefix="t%d.g." % t))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.join(sys.argv[1], "Code", "sage+gat+diffpool")
    if not os.path.isdir(ref_dir):
        sys.exit("no Code/sage+gat+diffpool under %s" % sys.argv[1])
    GG.REF_DIR = ref_dir
    _, gat = GG._import_reference()
    with contextlib.redirect_stdout(io.StringIO()):
        import tripletnet as tn
    for s, (name, final_dim) in enumerate(CASES.items()):
        out = run_case(gat, tn, final_dim, 500 + s)
        path = os.path.join(GG.OUT_DIR, name + ".npz")
        np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
        print("wrote", path, "losses", [float(out["t%d.loss" % t]) for t in range(len(TRIPLETS))], "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
