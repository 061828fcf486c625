#!/usr/bin/env python3
"""Golden vectors of the reference's classification loop around its GAT encoder (test infrastructure; never imported by the product
path).

Same rules and stubs as oracle/gen_golden.py (whose helpers it imports) and scripts/gen_golden_gat_triplet.py: the reference's
Code/sage+gat+diffpool is imported read-only with ``.cuda()`` turned into the identity and the ``DGATHead_V3`` name the constructor of
``DGATLayer`` trips over defined as an empty class.  The driver file train.py does not run here (it imports the loaders of a whole
experiment), so its loop is restated line by line around the reference's own model:

  * train.py:257-261  ``DGATEncoderGraph(input_dim, hidden_dim, output_dim, num_classes, final_dim='number_classes', ...)``
  * train.py:89       ``torch.optim.Adam(filter(requires_grad, model.parameters()), lr=0.001)``
  * train.py:110-130  per batch (``batch_size`` 1, the reference's default): ``model.zero_grad()``,
                      ``_, ypred = model(h0, adj, batch_num_nodes)``, ``loss = model.loss(ypred, label)``, backward,
                      ``clip_grad_norm(model.parameters(), 2.0)``, ``optimizer.step()``

The model: Nmax 16, 2 layers x 2 heads x 8, embedding 8, 3 classes.  The data: 8 labelled graph dicts filled as cross_val.py fills
them, sizes [16, 9, 1, 12, 5, 14, 7, 11] (16 == Nmax: no padded row; a one-node graph), labels [0, 1, 2, 1, 0, 2, 2, 1]; node 3 of
graph 3 loses all its edges (an edge-less column that is not padding).  Stored as data only in tests/golden/minibatch_gat.npz:

  * the initial state dict (``p.``), the graphs with their labels (``g<i>.``)
  * per graph, from the initial parameters at B = 1: the readout row ``x``, ``ypred``, ``model.loss`` and every parameter gradient
    (``b<i>.x / .ypred / .loss / .g.<name>``; a parameter the loss does not reach is stored as zeros)
  * the loop for 6 steps over graphs ``loop.order`` with clip 2.0 and Adam lr 1e-3: the per-step losses (``loop.loss``) and the final
    state dict (``final.``)

Usage:  python scripts/gen_golden_gat_minibatch.py REFERENCE_ROOT        (rewrites tests/golden/minibatch_gat.npz)
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as GG  # noqa: E402

NMAX, FIN, HID, EMB, LAB = 16, 6, 8, 8, 3
SIZES = [16, 9, 1, 12, 5, 14, 7, 11]          # (16 == Nmax: no padded row; 1: a one-node graph)
LABELS = [0, 1, 2, 1, 0, 2, 2, 1]
ISOLATED = {3: 3}                             # graph -> a real node that loses all its edges
ORDER = [0, 3, 2, 5, 7, 1]                    # the loop's six steps: the full graph, the isolated node, the one-node graph, ...
LR, CLIP, SEED = 1e-3, 2.0, 810
NAME = "minibatch_gat"


def graph_dict(gen, n, label, isolated=None):
    x, adj, _ = GG.make_batch(gen, 1, NMAX, FIN, sizes=[n], p_edge=0.3)
    a = adj[0].numpy().copy()
    if isolated is not None:
        a[isolated, :] = 0.0
        a[:, isolated] = 0.0
    f = x[0].numpy().copy()
    return {"adj": a, "feats": f, "num_nodes": n, "assign_feats": f.copy(), "label": label}


def call_model(model, d):
    adj = torch.Tensor(np.array([d["adj"]]))
    h0 = torch.Tensor(np.array([d["feats"]]))
    return model(h0, adj, np.array([d["num_nodes"]]), assign_x=torch.Tensor(d["assign_feats"]))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.join(sys.argv[1], "Code", "sage+gat+diffpool")
    if not os.path.isdir(ref_dir):
        sys.exit("no Code/sage+gat+diffpool under %s" % sys.argv[1])
    GG.REF_DIR = ref_dir
    _, gat = GG._import_reference()
    warnings.filterwarnings("ignore")
    gen = torch.Generator().manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        model = gat.DGATEncoderGraph(FIN, HID, EMB, LAB, None, num_layers=2, num_heads=[2, 2], neg_input_slopes=[0.2, 0.2],
                                     dropouts=[0.0, 0.0], final_dim="number_classes")
    GG.randomise_(model, gen, 0.4)
    dicts = [graph_dict(gen, n, y, ISOLATED.get(i)) for i, (n, y) in enumerate(zip(SIZES, LABELS))]
    out = dict(dims=np.array([FIN, HID, EMB, LAB]), nmax=NMAX, num_layers=2, heads=np.array([2, 2]), final_dim=np.array("number_classes"),
               lr=np.float64(LR), clip=np.float64(CLIP), seed=SEED, n_graphs=len(dicts), **GG.sd_np(model))
    for i, d in enumerate(dicts):
        out["g%d.adj" % i] = d["adj"].astype(np.float32)
        out["g%d.feats" % i] = d["feats"].astype(np.float32)
        out["g%d.num_nodes" % i] = np.int64(d["num_nodes"])
        out["g%d.label" % i] = np.int64(d["label"])
    model.train()
    for i, d in enumerate(dicts):                           # every graph alone, from the initial parameters
        model.zero_grad(set_to_none=True)
        x, ypred = call_model(model, d)
        loss = model.loss(ypred, torch.LongTensor([int(d["label"])]))
        loss.backward()
        out["b%d.x" % i] = x.detach().numpy().copy()
        out["b%d.ypred" % i] = ypred.detach().numpy().copy()
        out["b%d.loss" % i] = np.float32(loss.item())
        out.update(GG.grads_np(model, prefix="b%d.g." % i))
    optimizer = torch.optim.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=LR)              # train.py:89
    losses = []
    for i in ORDER:                                                                                         # train.py:110-130
        d = dicts[i]
        model.zero_grad()
        _, ypred = call_model(model, d)
        loss = model.loss(ypred, torch.LongTensor([int(d["label"])]))
        loss.backward()
        nn.utils.clip_grad_norm_(model.parameters(), CLIP)
        optimizer.step()
        losses.append(loss.item())
    out["loop.order"] = np.array(ORDER, dtype=np.int64)
    out["loop.loss"] = np.array(losses, dtype=np.float32)
    out.update(GG.sd_np(model, prefix="final."))
    path = os.path.join(GG.OUT_DIR, NAME + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, "per-graph losses", [float(out["b%d.loss" % i]) for i in range(len(dicts))], "loop losses", losses,
          "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
