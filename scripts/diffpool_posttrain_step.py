#!/usr/bin/env python3
"""The post-training step of 2stg+ with --method=soft-assign, measured (train_triplet_pre_train.py:233-262: ONE anchor graph per
optimiser step): 256 DD-shaped synthetic labelled graphs, Nmax 1000, SoftPoolingGcnEncoder 3 layers x hidden (64 and 128),
assign_ratio 0.1, one pooling level, final_dim pretrain with the replacement head (post_train.install_head), Adam at lr 1e-3 without
clipping under FlatTrainer(clip=0), a seeded schedule of 2,000 anchors.  The rows of scripts/gat_posttrain_step.py (whose ``measure``
this script runs) per hidden width, in ONE process:

  (a) streamed: diffpool_stream.PostTrainStream, a NEW anchor per replay of one hipGraph
  (b) a resident single anchor re-taken by the same captured step (triplet.assemble once, lr = 0)
  (c) the eager post_train.post_train_step, fed the same objects in the same order
  (d) what post_train_step did for this model before it had a resident branch: the module call on dense [1, N, N] arrays

    python scripts/diffpool_posttrain_step.py [OUTPUT_FILE [HIDDEN ...]]       (appends to OUTPUT_FILE)"""
import os
import sys


def main():
    import numpy as np
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import gat_posttrain_step as S
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import dense_encoders as E, diffpool_stream, post_train as PT, triplet
    from two_stage_gnn_amd import resident as R
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    dev = torch.device("cuda")
    pool, fin = dense_dataset(S.GRAPHS)
    anchors = np.random.default_rng(1).integers(0, S.GRAPHS, size=S.STEPS)
    out = sys.argv[1] if len(sys.argv) > 1 else None
    for h in [int(v) for v in sys.argv[2:]] or [64, 128]:
        def make(lr, h=h):
            torch.manual_seed(5)
            m = E.SoftPoolingGcnEncoder(1000, fin, h, h, 2, 3, h, assign_ratio=0.1, num_pooling=1, linkpred=False, final_dim="pretrain").to(dev).train()
            PT.install_head(m)
            return m, FlatTrainer(m, lr=lr, clip=0)

        def resident_loss_of(m, obj):
            g, x, xa, sizes = triplet.assemble([triplet.resident_graph(obj, dev, R.resident_cache(m))], dev)
            ids = torch.zeros(1, dtype=torch.int32, device=dev)
            lab = torch.tensor([int(obj.graph["label"])], dtype=torch.int32, device=dev)
            return lambda: PT.apply_head(m, PT._readout(m, x, g, sizes, x if xa is None else xa), ids, lab)[0]

        S.measure("DD-shaped, Nmax 1000, %d features; SoftPoolingGcnEncoder 3 layers x %d, assign_ratio 0.1 (K = 100), one pooling level, final_dim "
                  "pretrain: readout rows of P = %d columns into the fused head" % (fin, h, 2 * 3 * h), pool, anchors, make,
                  lambda m: diffpool_stream.PostTrainStream(m, pool, max_steps=S.STEPS), resident_loss_of, out)


if __name__ == "__main__":
    main()
