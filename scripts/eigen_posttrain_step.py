#!/usr/bin/env python3
"""The post-training step of 2stg+ for the EigenGCN family, measured (Code/eigengcn/train_triplet_pre_train.py:192-247: ONE optimiser
step on the sampler's anchor at B = 1, loss = model.loss(model(...), label), clip, the TRIPLET phase's Adam): 256 DD-shaped synthetic
labelled graphs (scripts/eigen_step.py's generator and chunked clusters), Nmax 1000, WavePoolingGcnEncoder 3 layers h128, pool_sizes
'10', J = 2, Jf = 1, con_final 1, pred_hidden_dims [50], label_dim 64, FlatTrainer(lr 1e-3, clip 2.0), a seeded schedule of 2,000
anchors.  Three figures in ONE process, five alternating windows each (``sag_posttrain_step.measure3``):

  (a) streamed: eigen_stream.PostTrainStream, a NEW anchor per replay of one hipGraph (a window = 400 consecutive schedule entries)
  (b) the eager eigen_stream.post_train_step on the resident piece, fed the same objects in the same order (a window = 40 entries)
  (c) the plain module call on dense [1, N, N] host arrays + model.loss, same objects and order

plus the device kernels of one streamed step.

    python scripts/eigen_posttrain_step.py [OUTPUT_FILE]     (appends to OUTPUT_FILE; the GPU work runs in ONE child process under its
                                                              own time limit)"""
import os
import subprocess
import sys

GRAPHS, STEPS = 256, 2000
NMAX, J, JF, LABEL_DIM = 1000, 2, 1, 64
LIMIT_S = 600


def main_all(out_path):
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--run"] + ([out_path] if out_path else []))
    if r.returncode != 0:                                    # (a fault or a time-out: nothing more is started on the device)
        print("the run ended with status %d" % r.returncode)
        sys.exit(r.returncode)


def main_one(out_path):
    import time
    import types
    import numpy as np
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import eigen_step
    from sag_posttrain_step import measure3
    from two_stage_gnn_amd import eigen_encoders as EE, eigen_pool as ep, eigen_stream
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    args = types.SimpleNamespace(bias=True, con_final=1, pool_sizes="10", num_pool_matrix=J, num_pool_final_matrix=JF)

    class Graph:
        pass

    t0 = time.perf_counter()
    results, xp, _ = eigen_step.batch(7, B=GRAPHS, nmax=NMAX)
    fin = int(xp.shape[2])
    labels = np.random.default_rng(3).integers(0, LABEL_DIM, size=GRAPHS)
    pool = []
    f32 = lambda t: np.ascontiguousarray(t[0].numpy().astype(np.float32))
    for b, r in enumerate(results):
        adj, pooled, n0, nl, pm = ep.dense_inputs([r], NMAX, J, JF)
        g = Graph()
        g.graph = {"adj": f32(adj), "feats": xp[b], "num_nodes": int(n0[0]), "adj_pool_1": f32(pooled[0]), "num_nodes_1": int(nl[0][0]),
                   "label": int(labels[b])}
        for j in range(J):
            g.graph["pool_adj_0_%d" % j] = f32(pm[0][j])
        for j in range(JF):
            g.graph["pool_adj_1_%d" % j] = f32(pm[1][j])
        pool.append(g)
    del results
    t_data = time.perf_counter() - t0
    sizes = np.array([g.graph["num_nodes"] for g in pool])
    anchors = np.random.default_rng(1).integers(0, GRAPHS, size=STEPS)

    def make():
        torch.manual_seed(5)
        m = EE.WavePoolingGcnEncoder(NMAX, fin, 128, 128, LABEL_DIM, 3, num_pool_matrix=J, num_pool_final_matrix=JF, pool_sizes=[10],
                                     pred_hidden_dims=[50], args=args).train()
        return m, FlatTrainer(m, lr=1e-3, clip=2.0)

    def plain(m, g):
        d = g.graph
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)[None]).to(dev)
        pm = {0: [t(d["pool_adj_0_%d" % j]) for j in range(J)], 1: [t(d["pool_adj_1_%d" % j]) for j in range(JF)]}
        ypred = m(t(d["feats"]), t(d["adj"]), [t(d["adj_pool_1"])], [int(d["num_nodes"])], [[int(d["num_nodes_1"])]], pm)
        return m.loss(ypred, torch.tensor([int(d["label"])], device=dev))

    measure3("DD-shaped: %d labelled graphs (%d..%d nodes, mean %.0f; built in %.0f s), Nmax %d, %d features; WavePoolingGcnEncoder 3 layers h128, "
             "pool_sizes '10', J %d, Jf %d, con_final 1, pred_hidden_dims [50], label_dim %d; cross-entropy + clip 2.0 + Adam under FlatTrainer"
             % (GRAPHS, sizes.min(), sizes.max(), sizes.mean(), t_data, NMAX, fin, J, JF, LABEL_DIM), pool, anchors, make,
             lambda m: eigen_stream.PostTrainStream(m, pool, max_steps=STEPS), lambda m, g: eigen_stream.post_train_step(m, g)[0], plain,
             out_path, note="the three-graph triplet step of profiles/r18/eigen_stream.txt: 379 us/step")


if __name__ == "__main__":
    a = sys.argv[1:]
    if a[:1] == ["--run"]:
        main_one(a[1] if len(a) > 1 else None)
    else:
        main_all(a[0] if a else None)
