#!/usr/bin/env python3
"""Golden vectors of the reference's 2stg+ post-training phase (test infrastructure; never imported by the product path).

Same rules and stubs as oracle/gen_golden.py (whose helpers it imports): the reference's Code/sage+gat+diffpool/encoders.py is imported
read-only with ``.cuda()`` turned into the identity.  The reference's constructor runs as it stands; what does NOT run here is the
driver file itself (train_triplet_pre_train.py imports the data loaders and the samplers of a whole experiment), so its two loops are
restated below line by line around the reference's own model:

  * :201-211  the replacement ``map2_model`` Linear(output_dim, 64) - LeakyReLU - Linear(64, 32) - LeakyReLU - Linear(32, 2) and
              ``torch.optim.Adam(model.parameters(), lr=0.001)``
  * :233-262  per anchor graph: zero_grad, ``pred, out = model(h0, adj, [n], assign_x=...)``,
              ``loss = F.cross_entropy(F.softmax(pred), label)``, backward, step (no clipping: :261 is commented out)
  * :36-72    ``evaluate()``: eval mode, the argmax of ``pred`` per graph, sklearn's macro precision / recall, accuracy, micro F1

It builds ONE ``GcnEncoderGraph(final_dim='pretrain')`` (Nmax 16, fin 8, 3 layers, hidden 8, output_dim 8, bn), six graph dicts filled
as cross_val.py fills them (a full graph n == Nmax, a one-node graph, both labels), runs six steps, one per graph, and stores as data
only in tests/golden/posttrain_gcn.npz: the initial state dict, the graphs with their labels, per step ``pred`` / ``out`` / loss, every
parameter gradient of step 0, the parameters after the sixth step, and ``evaluate()``'s predictions and metrics of the final model on
the six graphs.

Usage:  python scripts/gen_golden_posttrain.py REFERENCE_ROOT        (rewrites tests/golden/posttrain_gcn.npz)
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

NMAX, FIN, HID, EMB, LAB, LAYERS = 16, 8, 8, 8, 2, 3
SIZES = [16, 1, 9, 12, 5, 14]                 # (16 == Nmax: no padded row; 1: a one-node graph)
LABELS = [0, 1, 1, 0, 1, 0]
SEED, LR = 700, 1e-3


def graph_dict(gen, n, label):
    x, adj, _ = GG.make_batch(gen, 1, NMAX, FIN, sizes=[n], p_edge=0.3)
    f = x[0].numpy().copy()
    return {"adj": adj[0].numpy().copy(), "feats": f, "num_nodes": n, "assign_feats": f.copy(), "label": label}


def call_model(model, d):
    adj = torch.Tensor(np.array([d["adj"]]))
    h0 = torch.Tensor(np.array([d["feats"]]))
    assign = torch.Tensor(d["assign_feats"])
    return model(h0, adj, np.array([d["num_nodes"]]), assign_x=assign)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.join(sys.argv[1], "Code", "sage+gat+diffpool")
    if not os.path.isdir(ref_dir):
        sys.exit("no Code/sage+gat+diffpool under %s" % sys.argv[1])
    GG.REF_DIR = ref_dir
    enc, _ = GG._import_reference()
    import sklearn.metrics as metrics
    warnings.filterwarnings("ignore")

    class A:
        bias = True
    gen = torch.Generator().manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        model = enc.GcnEncoderGraph(FIN, HID, EMB, LAB, LAYERS, bn=True, args=A(), final_dim="pretrain")
    model.map2_model = nn.Sequential(nn.Linear(EMB, 64), nn.LeakyReLU(), nn.Linear(64, 32), nn.LeakyReLU(), nn.Linear(32, 2))   # :201-210
    GG.randomise_(model, gen, 0.4)
    GG.randomise_(model.map2_model, gen, 0.12)          # (logits of a few tenths: at 0.4 both soft-maxes saturate and every gradient vanishes)
    dicts = [graph_dict(gen, n, y) for n, y in zip(SIZES, LABELS)]
    out = dict(dims=np.array([FIN, HID, EMB, LAB]), nmax=NMAX, num_layers=LAYERS, lr=np.float64(LR), seed=SEED, n_graphs=len(dicts),
               **GG.sd_np(model))
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
            out.update(GG.grads_np(model, prefix="s0.g."))
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
    path = os.path.join(GG.OUT_DIR, "posttrain_gcn.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, "losses", [float(out["s%d.loss" % s]) for s in range(len(dicts))], "eval pred", out["eval.pred"].tolist(),
          "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
