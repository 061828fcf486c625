#!/usr/bin/env python3
"""Golden vectors of the reference's EigenGCN stage two (test infrastructure; never imported by the product path).

Same rules and stubs as scripts/gen_golden_eigen.py and scripts/gen_golden_eigen_triplet.py (whose helpers it imports): the
reference's Code/eigengcn is imported read-only with ``.cuda()`` turned into the identity and SpectralClustering replaced by fixed
chunk labels.  For every case it builds a small seeded dataset of ``.graph`` dicts the way the reference's sampler fills them, over
three classes (the class moves the features' mean), and runs the reference's OWN ``evaluate()`` (train_triplet.py:30-135) on two
batch-1 ``DataLoader``s WITHOUT shuffling, so row i of the stored embeddings is graph i.  ``evaluate()`` returns only the metrics; the
embeddings it fits on and what sklearn's ``KNeighborsClassifier`` predicts are recorded by a subclass put in the classifier's place
for the call.  Stored, as data only (float32, compressed): the dicts' arrays, the labels, the state_dict, the B = 1 embeddings,
sklearn's predictions for both sets and the metrics dictionary -> tests/golden/two_stage_eval_eigen_*.npz.

The dataset's seed is the first one from its start value for which no query (validation rows and the training rows themselves) is
undecided under the band of scripts/gen_golden_knn.py's ``_undecided_any``: the GPU test then has no query it may skip.

Usage:  python scripts/gen_golden_eigen_two_stage.py REFERENCE_ROOT        (rewrites tests/golden/two_stage_eval_eigen_*.npz)
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_eigen as GE  # noqa: E402
import gen_golden_eigen_triplet as GT  # noqa: E402
import gen_golden_knn as GK  # noqa: E402

N_TRAIN, N_VAL, CLASSES, K = 24, 12, 3, 3
CASES = {
    "two_stage_eval_eigen_j2_final": dict(J=2, Jf=1, con_final=1, pool_sizes=[4], nmax=16, seed0=500),
    "two_stage_eval_eigen_two_levels": dict(J=1, Jf=0, con_final=0, pool_sizes=[3, 2], nmax=18, nmin=12, seed0=600),      # (12 nodes: 4, then 2 clusters)
}


def run_case(cp, enc, tt, cfg, seed):
    from sklearn.neighbors import KNeighborsClassifier
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    J, Jf, N = cfg["J"], cfg["Jf"], cfg["nmax"]
    F_in, H, E, layers, label_dim, pred_hidden = 7, 12, 8, 3, 6, [10]
    dicts = []
    for b in range(N_TRAIN + N_VAL):
        n = int(rng.integers(cfg.get("nmin", 9), N + 1))
        d, _ = GT.graph_dict(cp, rng, gen, n, N, cfg, F_in)
        d["label"] = b % CLASSES
        d["feats"][:n] += 0.6 * d["label"]
        d["assign_feats"] = d["feats"].copy()
        dicts.append(d)

    class Args:
        bias = True
        con_final = cfg["con_final"]
        pool_sizes = "_".join(str(s) for s in cfg["pool_sizes"])
        num_pool_matrix = J
        num_pool_final_matrix = Jf
    with contextlib.redirect_stdout(io.StringIO()):
        m = enc.WavePoolingGcnEncoder(N, F_in, H, E, label_dim, layers, num_pool_matrix=J, num_pool_final_matrix=Jf,
                                      pool_sizes=cfg["pool_sizes"], pred_hidden_dims=pred_hidden, concat=True, bn=True, mask=1, args=Args())
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
    seen = {}

    class Recording(KNeighborsClassifier):
        def fit(self, X, y):
            seen["train"], seen["y_train"] = np.asarray(X, dtype=np.float32), np.asarray(y).reshape(-1)
            return super().fit(X, y)

        def predict(self, X):
            out = super().predict(X)
            seen.setdefault("preds", []).append((np.asarray(X, dtype=np.float32), np.asarray(out).reshape(-1)))
            return out
    loader = lambda ds: torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    prev = tt.KNeighborsClassifier
    tt.KNeighborsClassifier = Recording
    try:
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            result = tt.evaluate(loader(dicts[:N_TRAIN]), loader(dicts[N_TRAIN:]), m, Args())
    finally:
        tt.KNeighborsClassifier = prev
    (E_va, pred_val), (E_tr, pred_train) = seen["preds"]            # (evaluate() predicts the validation rows first)
    assert np.array_equal(E_tr, seen["train"]) and E_tr.shape == (N_TRAIN, label_dim) and E_va.shape == (N_VAL, label_dim)
    y = np.array([d["label"] for d in dicts])
    assert np.array_equal(seen["y_train"], y[:N_TRAIN])
    decided = not (GK._undecided_any(E_tr, y[:N_TRAIN], E_va, K) or GK._undecided_any(E_tr, y[:N_TRAIN], E_tr, K))
    out = dict(J=J, Jf=Jf, con_final=cfg["con_final"], mask=1, nmax=N, num_layers=layers, hidden=H, emb=E, label_dim=label_dim,
               pred_hidden=np.asarray(pred_hidden, dtype=np.int64), pool_sizes=np.asarray(cfg["pool_sizes"]), n_train=N_TRAIN, k=K,
               seed=seed, embed=np.concatenate([E_tr, E_va]), pred_val=pred_val, pred_train=pred_train,
               metric_names=np.array(sorted(result)), metrics=np.array([result[k] for k in sorted(result)], dtype=np.float64))
    keys = [k for k in dicts[0] if k != "assign_feats"]            # (read by the reference, never used)
    for k in keys:
        a = np.stack([np.asarray(d[k]) for d in dicts])
        if k == "adj":
            assert np.isin(a, (0.0, 1.0)).all()
            a = a.astype(np.uint8)
        elif a.dtype.kind == "f":
            a = a.astype(np.float32)                                 # (what evaluate() feeds the model: every tensor goes through .float())
        out["d." + k] = a
    for k, v in m.state_dict().items():
        out["p." + k] = v.detach().numpy().copy()
    return out, decided


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.join(sys.argv[1], "Code", "eigengcn")
    if not os.path.isdir(ref_dir):
        sys.exit("no Code/eigengcn under %s" % sys.argv[1])
    cp, enc = GE._import_reference(ref_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        import train_triplet as tt
    for name, cfg in CASES.items():
        for seed in range(cfg["seed0"], cfg["seed0"] + 50):
            out, decided = run_case(cp, enc, tt, cfg, seed)
            if decided:
                break
        else:
            raise SystemExit("no seed without an undecided query for " + name)
        path = os.path.join(GE.OUT_DIR, name + ".npz")
        np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
        print("wrote", path, "seed %d" % seed, dict(zip(out["metric_names"].tolist(), np.round(out["metrics"], 4).tolist())),
              "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
