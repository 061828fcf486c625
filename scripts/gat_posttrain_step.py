#!/usr/bin/env python3
"""The post-training step of 2stg+ with --method=GAT, measured (train_triplet_pre_train.py:233-262: ONE anchor graph per optimiser
step): 256 DD-shaped synthetic labelled graphs, Nmax 1000, DGATEncoderGraph 2 layers x 4 heads x 64, final_dim output_dim with the
replacement head (post_train.install_head), Adam at lr 1e-3 without clipping under FlatTrainer(clip=0), a seeded schedule of 2,000
anchors.  Four figures in ONE process, five alternating windows each:

  (a) streamed: gat_stream.PostTrainStream, a NEW anchor per replay of one hipGraph (a window = 400 consecutive schedule entries)
  (b) a resident single anchor re-taken by the same captured step (gat_triplet.assemble once, lr = 0)
  (c) the eager post_train.post_train_step, fed the same objects in the same order (a window = 40 entries)
  (d) what post_train_step did for this model before it had a resident branch: the module call on dense [1, N, N] arrays built on
      the host every step and the torch expression of the loss, same objects and order

plus the device kernels of one streamed step.  ``measure`` is shared with scripts/diffpool_posttrain_step.py.

    python scripts/gat_posttrain_step.py [OUTPUT_FILE]       (appends to OUTPUT_FILE)

Replayed rows: device events around the window's replays; the eager rows: host clock around steps that end in a synchronise.
Reported: median [min .. max] over the windows."""
import os
import sys
import time

GRAPHS, STEPS, REPS, EAGER_STEPS = 256, 2000, 5, 40


def dense_step(model, obj, dev):
    """the module call on freshly uploaded dense arrays + the torch loss: train_triplet_pre_train.py:240-256 literally"""
    import numpy as np
    import torch
    import torch.nn.functional as F
    d = obj.graph
    label = torch.tensor([int(d["label"])], device=dev)
    adj = torch.as_tensor(np.asarray(d["adj"], dtype=np.float32)[None]).to(dev)
    h0 = torch.as_tensor(np.asarray(d["feats"], dtype=np.float32)[None]).to(dev)
    pred, _ = model(h0, adj, np.array([int(d["num_nodes"])]), assign_x=h0)
    return F.cross_entropy(F.softmax(pred, dim=1), label)


def measure(title, pool, anchors, make, stream_of, resident_loss_of, out_path, note=""):
    """``make(lr)`` -> (model, FlatTrainer); ``stream_of(model)`` -> a PostTrainStream; ``resident_loss_of(model, obj)`` -> the callable
    of row (b).  Prints the rows and appends them to ``out_path``"""
    import numpy as np
    import torch
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd.data_parallel import GraphedStep
    dev = torch.device("cuda")
    per = STEPS // REPS
    m_a, tr_a = make(1e-3)
    t0 = time.perf_counter()
    st = stream_of(m_a)
    t_pack = time.perf_counter() - t0
    gs_a = GraphedStep(tr_a, st.step_loss(), warmup=3)
    m_b, tr_b = make(0.0)                                    # (lr = 0: Adam on ONE graph would move every weight the same way step after step)
    gs_b = GraphedStep(tr_b, resident_loss_of(m_b, pool[anchors[0]]), warmup=3)
    m_c, tr_c = make(1e-3)
    m_d, tr_d = make(1e-3)

    def replayed(gs, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(gs.stream)
        for _ in range(n):
            gs.step()
        e1.record(gs.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    def eager(tr, step, w):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in anchors[w * per:w * per + EAGER_STEPS]:
            tr.step(lambda: step(pool[i]))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / EAGER_STEPS * 1e6

    step_c = lambda obj: PT.post_train_step(m_c, obj)[0]
    step_d = lambda obj: dense_step(m_d, obj, dev)
    st.load(anchors)
    replayed(gs_a, 50); replayed(gs_b, 50)                   # warm-up of every row (the eager rows: every window's objects once)
    for w in range(REPS):
        eager(tr_c, step_c, w); eager(tr_d, step_d, w)
    st.load(anchors)                                         # the epoch starts here: window w replays entries [w * per, (w + 1) * per)
    times = {"a": [], "b": [], "c": [], "d": []}
    losses = {"a": [], "b": []}
    for w in range(REPS):
        times["a"].append(replayed(gs_a, per))
        times["b"].append(replayed(gs_b, per))
        times["c"].append(eager(tr_c, step_c, w))
        times["d"].append(eager(tr_d, step_d, w))
        losses["a"].append(gs_a.loss_value()); losses["b"].append(gs_b.loss_value())
    pos = st.position()

    def kernels(gs):
        best = []
        for _ in range(3):                                   # (the profiler's first cycles in a process may drop events: keep the fullest)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                gs.step()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type.name == "CUDA"]
            best = ev if len(ev) > len(best) else best
        return best

    def short(n):
        n = n.replace("void ", "").replace("(anonymous namespace)::", "").replace("at::native::", "")
        return n.split("(")[0].split("<")[0][:40] or n[:40]

    ka, kb = kernels(gs_a), kernels(gs_b)
    us = Counter()
    for e in ka:
        us[short(e.name)] += e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
    sizes = np.array([int(o.graph["num_nodes"]) for o in pool])
    fmt = lambda v: "%8.1f [%8.1f .. %8.1f] us/step" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = ["%s; %d labelled graphs (%d..%d nodes, mean %.0f), Adam lr 1e-3, no clipping; schedule of %d seeded anchors; median [min .. max] "
             "of %d alternating windows" % (title, GRAPHS, sizes.min(), sizes.max(), sizes.mean(), STEPS, REPS)]
    lines.append("  arena packed + uploaded in %.2f s; capacity %d rows%s" % (t_pack, st.row_cap, note and "; " + note))
    lines.append("  (a) streamed, a new anchor per replay, one hipGraph          : %s   %d device kernels, %s; cursor after the windows: %d"
                 % (fmt(times["a"]), len(ka), gs_a.describe(), pos))
    lines.append("  (b) resident anchor (%d nodes) replayed, one hipGraph, lr 0 : %s   %d device kernels"
                 % (int(pool[anchors[0]].graph["num_nodes"]), fmt(times["b"]), len(kb)))
    lines.append("  (c) eager post_train_step, same objects in the same order    : %s" % fmt(times["c"]))
    lines.append("  (d) module call on dense host arrays + torch loss (the step before the resident branch) : %s" % fmt(times["d"]))
    lines.append("      (a) faster than (c) in every window: %s   time (c) / time (a) = %.2fx;   (a) faster than (d) in every window: %s   time (d) / time (a) "
                 "= %.2fx" % (all(x < y for x, y in zip(times["a"], times["c"])), med["c"] / med["a"],
                              all(x < y for x, y in zip(times["a"], times["d"])), med["d"] / med["a"]))
    lines.append("      time (a) / time (b) = %.3f" % (med["a"] / med["b"]))
    lines.append("      (a) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in ka).most_common(40)))
    lines.append("      (a) device us of one step, largest first: " + ", ".join("%s %.1f" % kv for kv in us.most_common(12)))
    lines.append("      loss of each window's last step: (a) %s  (b) %s"
                 % (" ".join("%.4f" % v for v in losses["a"]), " ".join("%.4f" % v for v in losses["b"])))
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")
    sys.stdout.flush()
    return med


def main():
    import numpy as np
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import gat_encoders as G, gat_stream, gat_triplet as GT, post_train as PT
    from two_stage_gnn_amd import resident as R
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    dev = torch.device("cuda")
    pool, fin = dense_dataset(GRAPHS)
    anchors = np.random.default_rng(1).integers(0, GRAPHS, size=STEPS)

    def make(lr):
        torch.manual_seed(5)
        m = G.DGATEncoderGraph(fin, 64, 64, 2, None, num_layers=2, num_heads=[4, 4], final_dim="output_dim").to(dev).train()
        PT.install_head(m)
        return m, FlatTrainer(m, lr=lr, clip=0)

    def resident_loss_of(m, obj):
        x, g = GT.assemble([GT.resident_piece(obj, dev, R.resident_cache(m))], dev, GT.head_counts(m))
        ids = torch.zeros(1, dtype=torch.int32, device=dev)
        lab = torch.tensor([int(obj.graph["label"])], dtype=torch.int32, device=dev)
        return lambda: PT.row_loss(GT.readout_rows(m, x, g), ids, lab)

    measure("DD-shaped, Nmax 1000, %d features; DGATEncoderGraph 2 layers x 4 heads x 64, final_dim output_dim: pred = the readout row "
            "(64 columns), loss on it" % fin, pool, anchors, make, lambda m: gat_stream.PostTrainStream(m, pool, max_steps=STEPS),
            resident_loss_of, sys.argv[1] if len(sys.argv) > 1 else None,
            note="the three-graph triplet step of profiles/r17/gat_stream.txt: 142.2 us/step at a capacity of 1443 rows")


if __name__ == "__main__":
    main()
