#!/usr/bin/env python3
"""Golden vectors of stage two (test infrastructure; never imported by the product path).

1. tests/golden/knn_*.npz — sklearn (1.7.2 when the committed files were written) on small seeded data: ``KNeighborsClassifier
   (n_neighbors=k)`` fit / predict / kneighbors and the four ``sklearn.metrics`` values of the reference's ``evaluate()``
   (train_triplet.py:90-94).  Non-contiguous integer labels, k in {1, 3, 5}, one case whose validation labels lack a class.
   These pin tests/knn_oracle.py (the fp64 brute force every larger test compares with) and ``two_stage.metrics_from_confusion``.

2. tests/golden/two_stage_eval_{base,diffpool}.npz — the reference's own ``evaluate()`` on a small seeded dataset: its encoders
   (Code/sage+gat+diffpool/encoders.py, imported read-only at run time with ``.cuda()`` turned into the identity in this process) run
   eval-mode B = 1 forwards exactly as train_triplet.py:49-75 calls them, sklearn classifies, and the file keeps DATA only: the
   ``.graph`` dictionaries' arrays, the state_dict, the B = 1 embeddings, sklearn's predictions and the metrics dictionary.  The
   dataset of a fixture is the first seed from its start value for which NO query is undecided under the widest band the GPU test may
   apply (see ``_undecided_any``), checked with the fp32 embeddings against their fp64 distances.

Usage:  python scripts/gen_golden_knn.py [REFERENCE_ROOT]        (without REFERENCE_ROOT only part 1 is rewritten)
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_oracle as KO  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden")
LABELS = np.array([3, 7, 11, 12, 40, 41])

KNN_CASES = {
    # name: (seed, n_train, n_query, D, k, labels of the validation set)
    "knn_k1_d16": (11, 300, 60, 16, 1, LABELS),
    "knn_k3_d32": (12, 300, 60, 32, 3, LABELS),
    "knn_k5_d24": (13, 280, 64, 24, 5, LABELS),
    "knn_k3_absent": (14, 300, 60, 20, 3, LABELS[:5]),        # no validation graph of class 41 (it is still predicted)
}


def save(name, **arrs):
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


def sk_metrics(y_true, y_pred):
    from sklearn import metrics
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # (a class without predictions: precision 0, with a warning)
        return np.array([metrics.precision_score(y_true, y_pred, average="macro"), metrics.recall_score(y_true, y_pred, average="macro"),
                         metrics.accuracy_score(y_true, y_pred), metrics.f1_score(y_true, y_pred, average="micro")])


def gen_knn():
    import sklearn
    from sklearn.neighbors import KNeighborsClassifier
    for name, (seed, n, nq, D, k, qlabels) in KNN_CASES.items():
        rng = np.random.default_rng(seed)
        centre = 0.5 * rng.normal(size=(LABELS.size, D))
        y, yq = LABELS[rng.integers(0, LABELS.size, n)], qlabels[rng.integers(0, qlabels.size, nq)]
        X = (centre[np.searchsorted(LABELS, y)] + rng.normal(size=(n, D))).astype(np.float32)
        Q = (centre[np.searchsorted(LABELS, yq)] + rng.normal(size=(nq, D))).astype(np.float32)
        X64, Q64 = X.astype(np.float64), Q.astype(np.float64)        # (sklearn computes in the dtype it is given: float64 distances of the fp32 rows)
        sk = KNeighborsClassifier(n_neighbors=k).fit(X64, y)
        pred, pred_train = sk.predict(Q64), sk.predict(X64)
        dist, idx = sk.kneighbors(Q64)
        save(name, X=X, y=y, Q=Q, y_q=yq, k=k, pred=pred, pred_train=pred_train, nbr_dist=dist, nbr_index=idx,
             metrics=sk_metrics(yq, pred), train_acc=float((pred_train == y).mean()), sklearn_version=np.array(sklearn.__version__))


# ----------------------------------------------------------------------------- the reference's evaluate()
def _import_reference(root):
    torch.Tensor.cuda = lambda self, *a, **k: self            # in THIS process only
    nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(root, "Code", "sage+gat+diffpool"))
    warnings.filterwarnings("ignore")
    import encoders  # noqa
    return encoders


class _G:
    """stands for the networkx graph whose ``.graph`` dictionary the reference reads (cross_val.py:158-184)"""

    def __init__(self, adj, feats, n, label):
        self.graph = {"adj": adj, "feats": feats, "num_nodes": n, "assign_feats": feats, "label": label}


NMAX, FIN, N_CLASSES = 20, 6, 3


def dataset(seed, n_graphs):
    """graphs of three classes that differ in edge density and feature mean; sizes 1 .. NMAX, the first graph fills NMAX, the second
    has two nodes"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_graphs):
        c = int(rng.integers(0, N_CLASSES))
        n = NMAX if i == 0 else (2 if i == 1 else int(rng.integers(5, NMAX + 1)))
        a = np.triu((rng.random((n, n)) < (0.12 + 0.14 * c)).astype(np.float32), 1)
        adj = np.zeros((NMAX, NMAX), dtype=np.float32)
        adj[:n, :n] = a + a.T
        feats = np.zeros((NMAX, FIN), dtype=np.float32)
        feats[:n] = (rng.normal(size=(n, FIN)) + 0.6 * c).astype(np.float32)
        out.append(_G(adj, feats, n, c))
    return out


def reference_embeddings(model, graphs):
    """train_triplet.py:49-59, one graph at a time"""
    model.eval()
    rows = []
    with torch.no_grad():
        for g in graphs:
            adj = torch.Tensor(np.array([g.graph["adj"]]))
            h0 = torch.Tensor(np.array([g.graph["feats"]]))
            assign = torch.Tensor(g.graph["assign_feats"])
            _, feat = model(h0, adj, np.array([g.graph["num_nodes"]]), assign_x=assign)
            rows.append(feat[0].numpy())
    return np.stack(rows).astype(np.float32)


# what the GPU test allows its embeddings to be off by (rtol = atol = 1e-4 on every element) turned into the band of its undecided rule
def _undecided_any(E_tr, y_tr, E_q, k):
    d = KO.distances(E_tr, E_q)
    dk = np.sort(d, axis=1)[:, k - 1]
    e_max = np.sqrt(E_tr.shape[1]) * 1e-4 * (1.0 + max(np.abs(E_tr).max(), np.abs(E_q).max()))
    return bool(KO.undecided(d, y_tr, k, KO.tau(E_tr.shape[1]) * dk + 2 * e_max).any())


def gen_eval(root):
    from sklearn.neighbors import KNeighborsClassifier
    enc = _import_reference(root)

    class A:
        bias = True
    n_train, n_val, k = 48, 16, 3
    for kind, seed0 in (("base", 100), ("diffpool", 200)):
        for seed in range(seed0, seed0 + 50):
            gen = torch.Generator().manual_seed(seed)
            graphs = dataset(seed, n_train + n_val)
            if kind == "base":
                m = enc.GcnEncoderGraph(FIN, 8, 8, 2, 3, bn=True, args=A(), final_dim="output_dim")
            else:
                m = enc.SoftPoolingGcnEncoder(NMAX, FIN, 8, 8, 2, 3, 8, assign_ratio=0.25, num_pooling=1, bn=True, linkpred=False,
                                              args=A(), assign_input_dim=FIN, final_dim="output_dim")
            with torch.no_grad():
                for p in m.parameters():
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.4)
            E = reference_embeddings(m, graphs)
            y = np.array([g.graph["label"] for g in graphs])
            E_tr, y_tr, E_va, y_va = E[:n_train], y[:n_train], E[n_train:], y[n_train:]
            if _undecided_any(E_tr, y_tr, E_va, k) or _undecided_any(E_tr, y_tr, E_tr, k):
                continue
            sk = KNeighborsClassifier(n_neighbors=k).fit(E_tr, y_tr)
            pred_val, pred_train = sk.predict(E_va), sk.predict(E_tr)
            # the fp64 brute force on the same rows must agree with sklearn: the fixture is then free of ties sklearn resolves its own way
            assert (KO.brute_force(E_tr, y_tr, E_va, k)[0] == pred_val).all() and (KO.brute_force(E_tr, y_tr, E_tr, k)[0] == pred_train).all()
            save("two_stage_eval_" + kind, adj=np.stack([g.graph["adj"] for g in graphs]).astype(np.uint8),
                 feats=np.stack([g.graph["feats"] for g in graphs]), num_nodes=np.array([g.graph["num_nodes"] for g in graphs]),
                 label=y, n_train=n_train, k=k, embed=E, pred_val=pred_val, pred_train=pred_train, metrics=sk_metrics(y_va, pred_val),
                 train_acc=float((pred_train == y_tr).mean()), seed=seed,
                 **{"p." + name: v.detach().numpy().copy() for name, v in m.state_dict().items()})
            break
        else:
            raise SystemExit("no seed without an undecided query for " + kind)


if __name__ == "__main__":
    gen_knn()
    if len(sys.argv) > 1:
        gen_eval(sys.argv[1])
