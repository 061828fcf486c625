#!/usr/bin/env python3
"""The post-training step of 2stg+, measured (train_triplet_pre_train.py:233-262: ONE anchor graph per optimiser step): DD-shaped
synthetic dataset of 256 labelled graphs, Nmax 1000, GcnEncoderGraph 3 layers x 128, output_dim 64, final_dim pretrain with the
replacement head (post_train.install_head), Adam at lr 1e-3 without clipping under FlatTrainer(clip=0), a seeded schedule of 2,000
anchors.  Three figures in ONE process, five alternating windows each:

  (a) streamed: post_train.PostTrainStream, a NEW anchor per replay of one hipGraph (a window = 400 consecutive schedule entries)
  (b) a resident single graph re-taken by the same captured step (the fused stack + the fused head on fixed buffers)
  (c) what the package offered before post_train: the eager loop of ``model(h0, adj, [n], assign_x=...)`` on freshly uploaded dense
      arrays with the torch ``Sequential`` head and ``F.cross_entropy(F.softmax(pred), label)``, fed the same objects in the same
      order (a window = 100 entries)

plus the device kernels of one streamed step.

    python scripts/posttrain_step.py [OUTPUT_FILE]

Replayed rows: device events around the window's replays; the eager row: host clock around steps that end in a synchronise.
Reported: median [min .. max] over the windows."""
import os
import sys
import time

GRAPHS, STEPS, REPS, EAGER_STEPS, OUT_DIM = 256, 2000, 5, 100, 64


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import dense_encoders as E, post_train as PT, triplet
    from two_stage_gnn_amd import resident as R
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    dev = torch.device("cuda")
    pool, fin = dense_dataset(GRAPHS)
    anchors = np.random.default_rng(1).integers(0, GRAPHS, size=STEPS)
    per = STEPS // REPS

    class A:
        bias = True

    def make():
        torch.manual_seed(5)
        m = E.GcnEncoderGraph(fin, 128, OUT_DIM, 2, 3, bn=True, args=A(), final_dim="pretrain").to(dev).train()
        PT.install_head(m)
        return m, FlatTrainer(m, lr=1e-3, clip=0)

    # (a)
    m_a, tr_a = make()
    t0 = time.perf_counter()
    st = PT.PostTrainStream(m_a, pool, max_steps=STEPS)
    t_pack = time.perf_counter() - t0
    gs_a = GraphedStep(tr_a, st.step_loss(), warmup=3)
    # (b)
    m_b, tr_b = make()
    g_b, x_b, _, sizes_b = triplet.assemble([triplet.resident_graph(pool[anchors[0]], dev, R.resident_cache(m_b))], dev)
    ids_b = torch.zeros(1, dtype=torch.int32, device=dev)
    lab_b = torch.tensor([int(pool[anchors[0]].graph["label"])], dtype=torch.int32, device=dev)
    gs_b = GraphedStep(tr_b, lambda: PT.apply_head(m_b, PT._readout(m_b, x_b, g_b, sizes_b, x_b), ids_b, lab_b)[0], warmup=3)
    # (c)
    m_c, tr_c = make()

    def reference_step(obj):
        d = obj.graph
        label = torch.tensor([int(d["label"])], device=dev)
        adj = torch.as_tensor(d["adj"][None]).to(dev)
        h0 = torch.as_tensor(d["feats"][None]).to(dev)
        pred, _ = m_c(h0, adj, np.array([d["num_nodes"]]), assign_x=h0)
        return F.cross_entropy(F.softmax(pred, dim=1), label)

    def replayed(gs, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(gs.stream)
        for _ in range(n):
            gs.step()
        e1.record(gs.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    def eager(w):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in anchors[w * per:w * per + EAGER_STEPS]:
            tr_c.step(lambda: reference_step(pool[i]))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / EAGER_STEPS * 1e6

    st.load(anchors)
    replayed(gs_a, 50); replayed(gs_b, 50); eager(0)         # warm-up of every row
    st.load(anchors)                                         # the epoch starts here: window w replays entries [w * per, (w + 1) * per)
    times = {"a": [], "b": [], "c": []}
    losses = {"a": [], "b": []}
    for w in range(REPS):
        times["a"].append(replayed(gs_a, per))
        times["b"].append(replayed(gs_b, per))
        times["c"].append(eager(w))
        losses["a"].append(gs_a.loss_value()); losses["b"].append(gs_b.loss_value())
    pos = st.position()

    def kernels(gs):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs.step()
            torch.cuda.synchronize()
        return [e for e in prof.events() if e.device_type.name == "CUDA"]

    def short(n):
        n = n.replace("void ", "").replace("(anonymous namespace)::", "").replace("at::native::", "")
        return n.split("(")[0].split("<")[0][:40] or n[:40]

    ka, kb = kernels(gs_a), kernels(gs_b)
    sizes = np.array([int(o.graph["num_nodes"]) for o in pool])
    fmt = lambda v: "%8.1f [%8.1f .. %8.1f] us/step" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in times.items()}
    ar = st.arena
    lines = []
    lines.append("DD-shaped, %d labelled graphs (%d..%d nodes, mean %.0f), Nmax %d, %d features, 3 layers x 128, output_dim %d (readout %d), final_dim "
                 "pretrain + Linear(%d, 64)-LeakyReLU-Linear(64, 32)-LeakyReLU-Linear(32, 2), Adam lr 1e-3, no clipping; schedule of %d seeded "
                 "anchors; median [min .. max] of %d alternating windows"
                 % (GRAPHS, sizes.min(), sizes.max(), sizes.mean(), ar.nmax, fin, OUT_DIM, m_a.pred_input_dim, OUT_DIM, STEPS, REPS))
    lines.append("  arena: %.1f MB, packed + uploaded in %.2f s; slot: %d rows + %d ghost slots, tail %d"
                 % ((ar.buf.nbytes + ar.feats.nbytes + ar.records.nbytes) / 1e6, t_pack, st.row_cap, st.g.ghost_slots_fixed, st.tail_cap))
    lines.append("  (a) streamed, a new anchor per replay, one hipGraph        : %s   %d device kernels per step; cursor after the windows: %d"
                 % (fmt(times["a"]), len(ka), pos))
    lines.append("  (b) resident graph (%d nodes) replayed, one hipGraph      : %s   %d device kernels per step"
                 % (int(sizes_b[0]), fmt(times["b"]), len(kb)))
    lines.append("  (c) eager module call + torch head, same objects and order : %s" % fmt(times["c"]))
    lines.append("      (a) faster than (c) in every window: %s   time (c) / time (a) = %.2fx   time (a) / time (c) = %.4f"
                 % (all(x < y for x, y in zip(times["a"], times["c"])), med["c"] / med["a"], med["a"] / med["c"]))
    lines.append("      time (a) / time (b) = %.3f (the triplet stream's: 1.11)" % (med["a"] / med["b"]))
    lines.append("      (a) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in ka).most_common(40)))
    lines.append("      loss of each window's last step: (a) %s  (b) %s"
                 % (" ".join("%.4f" % v for v in losses["a"]), " ".join("%.4f" % v for v in losses["b"])))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    sys.stdout.flush()


if __name__ == "__main__":
    main()
