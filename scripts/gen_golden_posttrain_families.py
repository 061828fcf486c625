#!/usr/bin/env python3
"""Golden vectors of the reference's 2stg+ post-training phase for --method=GAT and --method=soft-assign (test infrastructure; never
imported by the product path).

scripts/gen_golden_posttrain.py does this for --method=base; the rules and stubs are the same (oracle/gen_golden.py's helpers: the
reference's Code/sage+gat+diffpool is imported read-only with ``.cuda()`` turned into the identity and the ``DGATHead_V3`` name the
constructor of ``DGATLayer`` trips over defined as an empty class).  The reference's constructors run as they stand, with the
arguments of train_triplet_pre_train.py:387-404; the driver file itself does not run here (it imports the loaders and samplers of a
whole experiment), so its two loops are restated line by line around the reference's own models:

  * :201-211  the replacement ``map2_model`` Linear(output_dim, 64) - LeakyReLU - Linear(64, 32) - LeakyReLU - Linear(32, 2) and
              ``torch.optim.Adam(model.parameters(), lr=0.001)``
  * :233-262  per anchor graph: zero_grad, ``pred, out = model(h0, adj, [n], assign_x=...)``,
              ``loss = F.cross_entropy(F.softmax(pred), label)``, backward, step (no clipping: :261 is commented out)
  * :36-72    ``evaluate()``: eval mode, the argmax of ``pred`` per graph, sklearn's macro precision / recall, accuracy, micro F1

``DGATEncoderGraph(final_dim='output_dim')`` returns ``(x, map2_model(map_model(x)))`` with ``x`` the max-readout row
(encoders_GAT.py:189-198), so the loop's ``pred`` is that row: the loss runs over embedding_dim columns and ``map_model`` /
``map2_model`` never receive a gradient (stored as absent: Adam skips them).  ``SoftPoolingGcnEncoder(final_dim='pretrain')`` returns
``(map2_model(map_model(r)), map_model(r))`` on the concatenated readout rows of every level.

Both fixtures: Nmax 16, fin 8, six graph dicts filled as cross_val.py fills them, sizes [16, 1, 9, 12, 5, 14] (a full graph n == Nmax,
a one-node graph), labels [0, 1, 1, 0, 1, 0]; the GAT fixture adds a seventh graph without any edge.  GAT: 2 layers x 2 heads x 8,
embedding_dim 8.  DiffPool: 3 layers, hidden 8, assign_ratio 0.25, one pooling level, bn.  One step per graph; stored as data only in
tests/golden/posttrain_gat.npz and tests/golden/posttrain_diffpool.npz: the initial state dict, the graphs with their labels, per step
``pred`` / ``out`` / loss, every parameter gradient of step 0 that exists (``None`` is stored as absent), the parameters after the last
step, and ``evaluate()``'s predictions and metrics of the final model on the graphs.

Usage:  python scripts/gen_golden_posttrain_families.py REFERENCE_ROOT        (rewrites the two fixtures)
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as GG  # noqa: E402

NMAX, FIN, HID, EMB, LAB = 16, 8, 8, 8, 2
SIZES = [16, 1, 9, 12, 5, 14]                 # (16 == Nmax: no padded row; 1: a one-node graph)
LABELS = [0, 1, 1, 0, 1, 0]
EDGELESS = (7, 1)                             # GAT only: (size, label) of a graph without any edge
LR = 1e-3


def graph_dict(gen, n, label, edges=True):
    x, adj, _ = GG.make_batch(gen, 1, NMAX, FIN, sizes=[n], p_edge=0.3 if edges else 0.0)
    f = x[0].numpy().copy()
    return {"adj": adj[0].numpy().copy(), "feats": f, "num_nodes": n, "assign_feats": f.copy(), "label": label}


def call_model(model, d):
    adj = torch.Tensor(np.array([d["adj"]]))
    h0 = torch.Tensor(np.array([d["feats"]]))
    assign = torch.Tensor(d["assign_feats"])
    return model(h0, adj, np.array([d["num_nodes"]]), assign_x=assign)


def pred_model(dim):
    return nn.Sequential(nn.Linear(dim, 64), nn.LeakyReLU(), nn.Linear(64, 32), nn.LeakyReLU(), nn.Linear(32, 2))      # :201-208


def run(model, dicts, out, metrics):
    for i, d in enumerate(dicts):
        out["g%d.adj" % i] = d["adj"].astype(np.float32)
        out["g%d.feats" % i] = d["feats"].astype(np.float32)
        out["g%d.num_nodes" % i] = np.int64(d["num_nodes"])
        out["g%d.label" % i] = np.int64(d["label"])
    optimizer_2 = torch.optim.Adam(model.parameters(), lr=LR)                                                              # :211
    model.train()
    for s, d in enumerate(dicts):                                                                                         # :233-262
        optimizer_2.zero_grad()
        label = torch.LongTensor([int(d["label"])])
        pred, emb = call_model(model, d)
        loss = F.cross_entropy(F.softmax(pred), label)
        loss.backward()
        if s == 0:
            for k, p in model.named_parameters():
                if p.grad is not None:                      # (None stays absent: Adam skips such a parameter)
                    out["s0.g." + k] = p.grad.detach().numpy().copy()
        optimizer_2.step()
        out["s%d.pred" % s] = pred.detach().numpy().copy()
        out["s%d.out" % s] = emb.detach().numpy().copy()
        out["s%d.loss" % s] = np.float32(loss.item())
    out.update(GG.sd_np(model, prefix="final."))
    model.eval()                                                                                                          # :36-72
    labels, preds = [], []
    with torch.no_grad():
        for d in dicts:
            feat, _ = call_model(model, d)
            _, indices = torch.max(feat, 1)
            preds.append(indices.numpy())
            labels.append(d["label"])
    out["eval.pred"] = np.concatenate(preds).astype(np.int64)
    out["eval.prec"] = np.float64(metrics.precision_score(labels, preds, average="macro"))
    out["eval.recall"] = np.float64(metrics.recall_score(labels, preds, average="macro"))
    out["eval.acc"] = np.float64(metrics.accuracy_score(labels, preds))
    out["eval.F1"] = np.float64(metrics.f1_score(labels, preds, average="micro"))
    return out


def write(name, out, n):
    path = os.path.join(GG.OUT_DIR, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    grads = sorted(k for k in out if k.startswith("s0.g."))
    print("wrote", path, "losses", [float(out["s%d.loss" % s]) for s in range(n)], "eval pred", out["eval.pred"].tolist(),
          "%d gradients, largest %.3e" % (len(grads), max(float(np.abs(out[k]).max()) for k in grads)),
          "%.1f KB" % (os.path.getsize(path) / 1024))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.join(sys.argv[1], "Code", "sage+gat+diffpool")
    if not os.path.isdir(ref_dir):
        sys.exit("no Code/sage+gat+diffpool under %s" % sys.argv[1])
    GG.REF_DIR = ref_dir
    enc, gat = GG._import_reference()
    import sklearn.metrics as metrics
    warnings.filterwarnings("ignore")

    class A:
        bias = True

    # --method=GAT (:400-404)
    gen = torch.Generator().manual_seed(710)
    with contextlib.redirect_stdout(io.StringIO()):
        model = gat.DGATEncoderGraph(FIN, HID, EMB, LAB, num_layers=2, args=A(), final_dim="output_dim")
    model.map2_model = pred_model(EMB)                                                                                    # :210
    GG.randomise_(model, gen, 0.4)          # (the readout row is a max over ELU rows of order 1: neither soft-max saturates)
    GG.randomise_(model.map2_model, gen, 0.12)
    dicts = [graph_dict(gen, n, y) for n, y in zip(SIZES, LABELS)] + [graph_dict(gen, EDGELESS[0], EDGELESS[1], edges=False)]
    out = dict(dims=np.array([FIN, HID, EMB, LAB]), nmax=NMAX, num_layers=2, heads=np.array([2, 2]), lr=np.float64(LR), seed=710,
               n_graphs=len(dicts), **GG.sd_np(model))
    write("posttrain_gat", run(model, dicts, out, metrics), len(dicts))

    # --method=soft-assign (:387-392)
    gen = torch.Generator().manual_seed(720)
    with contextlib.redirect_stdout(io.StringIO()):
        model = enc.SoftPoolingGcnEncoder(NMAX, FIN, HID, EMB, LAB, 3, HID, assign_ratio=0.25, num_pooling=1, bn=True, dropout=0.0,
                                          linkpred=False, args=A(), assign_input_dim=FIN, final_dim="pretrain")
    model.map2_model = pred_model(EMB)
    GG.randomise_(model, gen, 0.4)
    GG.randomise_(model.map2_model, gen, 0.12)          # (logits of a few tenths: at 0.4 both soft-maxes saturate and every gradient vanishes)
    dicts = [graph_dict(gen, n, y) for n, y in zip(SIZES, LABELS)]
    out = dict(dims=np.array([FIN, HID, EMB, LAB]), nmax=NMAX, num_layers=3, num_pooling=1, ratio=np.float64(0.25), lr=np.float64(LR), seed=720,
               n_graphs=len(dicts), **GG.sd_np(model))
    write("posttrain_diffpool", run(model, dicts, out, metrics), len(dicts))


if __name__ == "__main__":
    main()
