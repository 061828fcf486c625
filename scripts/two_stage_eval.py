#!/usr/bin/env python3
"""Stage two measured: ``two_stage.evaluate`` (chunked embedding + the HIP k-NN launch) against the same evaluation done the
reference's way on this code base (train_triplet.py:36-101: one B = 1 forward per graph from dense host inputs, ``.cpu()`` per
embedding, the classifier and the metrics on the host), in ONE process, as the median of five alternating windows.

  DD    1,168 DD-shaped synthetic graphs (1,051 train / 117 validation), Nmax 1000, GcnEncoderGraph 3 layers h = 128, output_dim 64
  IMDB  1,000 IMDB-B-shaped graphs (900 / 100), sag_layers.Net nhid 128, ratio 0.5, final_dim 64

    python scripts/two_stage_eval.py              both configurations, each in a child process under its own time limit
    python scripts/two_stage_eval.py DD [N]       one configuration in this process (N: number of graphs, default as above)
    python scripts/two_stage_eval.py knn          only the k-NN launches of the DD-sized problem (to run under rocprofv3 --kernel-trace --stats)

Reported per configuration: wall time of both ways (host clock around a call that ends in a synchronise), the embedding and
classifier parts of the batched way from device events, the k-NN launch alone (device events around 200 launches) with its achieved
bytes/s against (n_train + n_query) D 4 algorithmic bytes, device kernels per evaluation, and embedding time per chunk size."""
import os
import subprocess
import sys
import time

REPS, LIMIT_S = 5, 420


def main_all():
    for cfg in ("DD", "IMDB"):
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), cfg])
        if r.returncode != 0:                                # (a fault or a time-out: nothing more is started on the device)
            print("configuration %s ended with status %d: stopping" % (cfg, r.returncode))
            sys.exit(r.returncode)


def _setup():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Obj:
    pass


def dense_dataset(n_graphs, nmax=1000):
    """``.graph`` dictionaries as cross_val.split_train_val prepares them: dense [Nmax, Nmax] adjacency, padded features"""
    import numpy as np
    from two_stage_gnn_amd import synthetic
    hb = synthetic.host_batch(7, n_graphs, "DD", nmax)
    gp = np.concatenate([[0], np.cumsum(hb["sizes"])])
    rp, col, fin = hb["rowptr"], hb["col"], hb["fin"]
    out = []
    for b in range(n_graphs):
        lo, hi = int(gp[b]), int(gp[b + 1])
        n = hi - lo
        adj = np.zeros((nmax, nmax), dtype=np.float32)
        adj[np.repeat(np.arange(n), np.diff(rp[lo:hi + 1])), col[rp[lo]:rp[hi]] - lo] = 1.0
        feats = np.zeros((nmax, fin), dtype=np.float32)
        feats[:n] = hb["x"][lo:hi] + 0.25 * hb["label"][b]                 # (a class signal, so that the classifier has something to find)
        g = _Obj()
        g.graph = {"adj": adj, "feats": feats, "num_nodes": n, "assign_feats": feats, "label": int(hb["label"][b])}
        out.append(g)
    return out, fin


def data_dataset(n_graphs, dev):
    import numpy as np
    import torch
    from two_stage_gnn_amd import synthetic
    hb = synthetic.host_batch(7, n_graphs, "IMDB-BINARY", 136)
    gp = np.concatenate([[0], np.cumsum(hb["sizes"])])
    rp, col = hb["rowptr"], hb["col"]
    out = []
    for b in range(n_graphs):
        lo, hi = int(gp[b]), int(gp[b + 1])
        d = _Obj()
        d.x = torch.from_numpy(np.ascontiguousarray(hb["x"][lo:hi] + 0.25 * hb["label"][b])).float().to(dev)
        d.edge_index = torch.from_numpy(np.stack([col[rp[lo]:rp[hi]].astype(np.int64) - lo,
                                                  np.repeat(np.arange(hi - lo), np.diff(rp[lo:hi + 1])).astype(np.int64)])).to(dev)
        d.y = torch.tensor([int(hb["label"][b])])
        out.append(d)
    return out, int(hb["x"].shape[1])


def host_classifier():
    """the reference's classifier and metrics on the host: sklearn when this machine has it, else a numpy brute force"""
    import numpy as np
    try:
        from sklearn import metrics
        from sklearn.neighbors import KNeighborsClassifier

        def run(E_tr, y_tr, E_va, y_va):
            neigh = KNeighborsClassifier(n_neighbors=3).fit(E_tr, y_tr)
            tp, vp = neigh.predict(E_tr), neigh.predict(E_va)
            return {"prec": metrics.precision_score(y_va, vp, average="macro"), "recall": metrics.recall_score(y_va, vp, average="macro"),
                    "acc": metrics.accuracy_score(y_va, vp), "F1": metrics.f1_score(y_va, vp, average="micro"),
                    "train acc": metrics.accuracy_score(y_tr, tp)}
        return "sklearn", run
    except ImportError:
        from two_stage_gnn_amd import two_stage as TS

        def run(E_tr, y_tr, E_va, y_va):
            labels = np.unique(np.concatenate([y_tr, y_va]))

            def predict(Q):
                d = ((Q[:, None, :].astype(np.float64) - E_tr[None].astype(np.float64)) ** 2).sum(-1)
                votes = np.stack([(y_tr[np.argsort(d, axis=1, kind="stable")[:, :3]] == c).sum(1) for c in labels], axis=1)
                return labels[votes.argmax(1)]
            res = TS.metrics_from_confusion(TS.confusion_matrix(y_va, predict(E_va), labels))
            res["train acc"] = float((predict(E_tr) == y_tr).mean())
            return res
        return "numpy brute force (no sklearn on this machine)", run


def main_one(cfg, n_graphs=None):
    import numpy as np
    import torch
    from torch.profiler import profile, ProfilerActivity
    _setup()
    from two_stage_gnn_amd import _native as nat, dense_encoders as E, sag_layers as S, two_stage as TS
    dev = torch.device("cuda")
    torch.manual_seed(5)
    if cfg == "DD":
        n_graphs = n_graphs or 1168
        graphs, fin = dense_dataset(n_graphs)

        class A:
            bias = True
        model = E.GcnEncoderGraph(fin, 128, 64, 2, 3, bn=True, args=A(), final_dim="output_dim").to(dev)
        chunks = (16, 32, 64, 128)
        label_of = lambda g: g.graph["label"]

        def one(g):                                                       # train_triplet.py:52-59
            adj = torch.Tensor(g.graph["adj"][None]).cuda()
            h0 = torch.Tensor(g.graph["feats"][None]).cuda()
            _, feat = model(h0, adj, np.array([g.graph["num_nodes"]]), assign_x=h0)
            return feat[0].cpu().numpy()
    else:
        n_graphs = n_graphs or 1000
        graphs, fin = data_dataset(n_graphs, dev)
        model = S.Net(fin, 128, 64, 0.5, 0.5).to(dev)
        chunks = (64, 128, 256, 512, 1000)
        label_of = lambda g: int(g.y)

        def one(g):                                                       # Code/sag/train_triplet.py:45-47 (the graph already on the device)
            return model(g)[0].cpu().numpy()
    n_val = max(1, int(round(0.1 * n_graphs)))                           # (DD: 1,051 / 117)
    train, val = graphs[:n_graphs - n_val], graphs[n_graphs - n_val:]
    y_tr, y_va = np.array([label_of(g) for g in train]), np.array([label_of(g) for g in val])
    clf_name, clf = host_classifier()

    def per_graph():
        model.eval()
        with torch.no_grad():                                             # (the reference does not switch autograd off; this is its way at its best)
            E_tr, E_va = np.stack([one(g) for g in train]), np.stack([one(g) for g in val])
        return clf(E_tr, y_tr, E_va, y_va)

    def batched():
        return TS.evaluate(train, val, model, n_neighbors=3)

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    t_first, res_b = wall(batched)                                        # first evaluation: the graphs become resident
    _, res_p = wall(per_graph)
    times = {"batched": [], "per_graph": []}
    for _ in range(REPS):
        times["batched"].append(wall(batched)[0])
        times["per_graph"].append(wall(per_graph)[0])

    def events(f, reps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps, r

    parts = {"embed": [], "knn": []}
    for _ in range(REPS):
        t, emb = events(lambda: TS.embed_dataset(model, train + val))
        parts["embed"].append(t)
        parts["knn"].append(events(lambda: TS.knn_confusions_device(emb[:len(train)], y_tr, emb[len(train):], y_va, 3))[0])
    knn = TS.KNeighborsClassifier(3).fit(emb[:len(train)], y_tr)
    assert knn.kernel_ok()
    q_va, q_tr = emb[len(train):], emb[:len(train)]
    knn.classify(q_va)
    assert nat.last_kernel().startswith("knn_classify_kernel")
    t_va = events(lambda: knn.classify(q_va), 200)[0] * 1e3
    t_tr = events(lambda: knn.classify(q_tr), 200)[0] * 1e3
    D = int(emb.size(1))
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        batched()
        torch.cuda.synchronize()
    n_kernels = len([e for e in prof.events() if e.device_type.name == "CUDA"])
    sweep = []
    for c in chunks:
        TS.embed_dataset(model, train + val, chunk=c)
        sweep.append((c, float(np.median([events(lambda: TS.embed_dataset(model, train + val, chunk=c))[0] for _ in range(3)]))))

    fmt = lambda v: "%9.2f [%9.2f .. %9.2f] ms" % (float(np.median(v)), min(v), max(v))
    print("%s: %d graphs (%d train / %d validation), embedding width %d, k = 3; median [min .. max] of %d alternating windows"
          % (cfg, n_graphs, len(train), len(val), D, REPS))
    print("  two_stage.evaluate (chunked embedding + HIP k-NN)          : %s   (first call, graphs not yet resident: %.1f ms)"
          % (fmt(times["batched"]), t_first))
    print("  per graph: B = 1 forward + .cpu() each, classifier = %s : %s" % (clf_name, fmt(times["per_graph"])))
    print("  batched faster in every window: %s   (ratio of medians %.1fx)"
          % (all(b < p for b, p in zip(times["batched"], times["per_graph"])), np.median(times["per_graph"]) / np.median(times["batched"])))
    print("  parts of the batched way (device events): embed_dataset %s, fit + both predictions + confusion %s" % (fmt(parts["embed"]), fmt(parts["knn"])))
    for name, t, nq in (("validation", t_va, len(val)), ("train-on-train", t_tr, len(train))):
        by = (len(train) + nq) * D * 4
        print("  k-NN launch alone, %-14s: %7.1f us   %d + %d rows x %d: %.2f MB algorithmic, %.1f GB/s" % (name, t, len(train), nq, D, by / 1e6, by / t / 1e3))
    print("  device kernels per evaluation: %d" % n_kernels)
    print("  embed_dataset by chunk (ms): " + ", ".join("%d: %.2f" % kv for kv in sweep))
    print("  metrics, batched  :", {k: round(v, 4) for k, v in res_b.items()})
    print("  metrics, per graph:", {k: round(float(v), 4) for k, v in res_p.items()})
    sys.stdout.flush()


def main_knn():
    """the k-NN launches of a DD-sized evaluation on synthetic embeddings: 20 x (validation on train, train on train)"""
    import numpy as np
    import torch
    _setup()
    from two_stage_gnn_amd import two_stage as TS
    rng = np.random.default_rng(0)
    y = rng.integers(0, 2, 1051)
    X = torch.from_numpy((0.5 * rng.normal(size=(2, 64))[y] + rng.normal(size=(1051, 64))).astype(np.float32)).cuda()
    Q = torch.from_numpy(rng.normal(size=(117, 64)).astype(np.float32)).cuda()
    knn = TS.KNeighborsClassifier(3).fit(X, y)
    for _ in range(20):
        knn.classify(Q)
        knn.classify(X)
    torch.cuda.synchronize()
    print("40 launches done")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "knn":
        main_knn()
    elif len(sys.argv) >= 2:
        main_one(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else None)
    else:
        main_all()
