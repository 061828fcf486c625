#!/usr/bin/env python3
"""EigenGCN (WavePoolingGcnEncoder) replayed optimiser step at the timed configuration: DD-shaped batches of 32 graphs, Nmax 1000,
3 layers h128, pool_sizes [10], J = 2, one final matrix, con_final 1.  Prints the step of seed 0 and the mean over seeds 0-7
(FlatTrainer + GraphedStep: forward, backward and Adam replayed from one hipGraph).

Clusters: ``--labels chunks`` (default) cuts each graph's node order into contiguous chunks of 10; ``--labels uneven`` draws cluster
sizes uniformly from 2 to 30 instead, in the same node order.  SpectralClustering's clusters are uneven and the pooling
launches walk each cluster's members in turn, so the chunked figure is a lower bound for clustered data until it is measured
with the clustering itself (not available where the step is timed)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_gnn_amd import eigen_encoders as EE, eigen_pool as ep, message_passing as mp, synthetic  # noqa: E402
from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep  # noqa: E402


def chunk_labels(A, k, level):
    return np.arange(A.shape[0]) * k // A.shape[0]


def uneven_labels(A, k, level):
    """contiguous runs of 2-30 nodes (seeded by the graph size), as many clusters as the sizes give"""
    n = A.shape[0]
    rng = np.random.default_rng(n)
    cuts, pos = [], 0
    while pos < n:
        step = int(rng.integers(2, 31))
        if n - pos - step < 2:
            step = n - pos
        cuts.append(step)
        pos += step
    return np.repeat(np.arange(len(cuts)), cuts)


def batch(seed, B=32, nmax=1000, fin=89, clusters=chunk_labels):
    """B graphs of DD shape that the coarsening accepts (the reference's driver drops the others), their padded features and labels"""
    res, feats, labels, draw = [], [], [], 0
    while len(res) < B:
        hb = synthetic.host_batch(1000 * seed + draw, B, "DD", nmax)
        draw += 1
        rp, col, x = np.asarray(hb["rowptr"]), np.asarray(hb["col"]), np.asarray(hb["x"], dtype=np.float32)
        off = 0
        for b, n in enumerate(np.asarray(hb["sizes"], dtype=np.int64)):
            A = np.zeros((n, n))
            for v in range(n):
                A[v, col[rp[off + v]:rp[off + v + 1]] - off] = 1.0
            r = ep.coarsen(A, [10], labels=clusters)
            if r is not None and len(res) < B:
                res.append(r)
                feats.append(x[off:off + n])
                labels.append(int(np.asarray(hb["label"])[b]) % 2)
            off += n
    xp = np.zeros((B, nmax, fin), dtype=np.float32)
    for b, f in enumerate(feats):
        xp[b, :f.shape[0]] = f
    return res, xp, np.asarray(labels, dtype=np.int64)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", choices=["chunks", "uneven"], default="chunks")
    kind = ap.parse_args().labels
    clusters = {"chunks": chunk_labels, "uneven": uneven_labels}[kind]
    dev = torch.device("cuda")

    class A:
        bias = True
        con_final = 1
    out = []
    for seed in range(8):
        res, xp, lab = batch(seed, clusters=clusters)
        eb = ep.collate(res, 1000, 2, 1)
        torch.manual_seed(seed)
        m = EE.WavePoolingGcnEncoder(1000, 89, 128, 128, 2, 3, num_pool_matrix=2, num_pool_final_matrix=1, pool_sizes=[10],
                                     args=A())
        x = torch.from_numpy(xp).to(dev)
        y = torch.from_numpy(lab).to(dev)
        tr = FlatTrainer(m, lr=1e-3)
        gs = GraphedStep(tr, lambda: mp.cross_entropy(m(x, eb), y), warmup=3)
        for _ in range(5):
            gs.step()
        gs.loss_value()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(gs.stream)
        for _ in range(100):
            gs.step()
        e1.record(gs.stream)
        e1.synchronize()
        loss = gs.loss_value()
        ms = e0.elapsed_time(e1) / 100
        out.append(ms)
        print("seed %d: %d graphs, %d nodes, %d clusters: %.4f ms/step (loss %.4f; %s)"
              % (seed, len(res), eb.g0.n_rows, eb.levels[0].g.n_rows, ms, loss, gs.describe()))
    print("eigengcn step b32 Nmax1000 h128 J2, %s clusters: seed 0 %.4f ms, mean of seeds 0-7 %.4f ms (min %.4f, max %.4f)"
          % (kind, out[0], float(np.mean(out)), min(out), max(out)))


if __name__ == "__main__":
    main()
