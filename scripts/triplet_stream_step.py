#!/usr/bin/env python3
"""The triplet stream, measured (train_triplet.py:247-287: ONE new triplet per optimiser step): DD-shaped synthetic dataset of 256
graphs, Nmax 1000, GcnEncoderGraph 3 layers x 128, final_dim output_dim, triplet.MarginRankingLoss + clip 2.0 + Adam under
FlatTrainer, a seeded schedule of 2,000 triplets.  Three figures in ONE process, five alternating windows each:

  (a) streamed: triplet.TripletStream, a NEW triplet per replay of one hipGraph (a window = 400 consecutive schedule entries)
  (b) the resident single triplet replayed from one hipGraph (the figure of bench.py --triplet's kind, re-taken here)
  (c) the eager drop-in, tripletnet.forward(a, p, n), fed the same objects in the same order (a window = 100 entries)

plus the gather launch alone (device events around a burst of launches: a burst, not a step) and the device kernels of one streamed step.

    python scripts/triplet_stream_step.py

Replayed rows: device events around the window's replays; the eager row: host clock around steps that end in a synchronise.
Reported: median [min .. max] over the windows."""
import os
import sys
import time

GRAPHS, STEPS, REPS, EAGER_STEPS, BURST = 256, 2000, 5, 100, 200
# far above any distance either model reaches in the run (the resident triplet of row (b), stepped 2,000 times, pushes its two distances
# more than 1,000 apart): the hinge stays active, so every timed step of (a) and (b) carries real gradients
MARGIN = 1.0e6


def main():
    import numpy as np
    import torch
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import dense_encoders as E, triplet
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    dev = torch.device("cuda")
    pool, fin = dense_dataset(GRAPHS)
    sched = np.random.default_rng(1).integers(0, GRAPHS, size=(STEPS, 3))
    tgt = torch.full((1,), -1.0, device=dev)
    per = STEPS // REPS

    class A:
        bias = True

    def make():
        torch.manual_seed(5)
        m = E.GcnEncoderGraph(fin, 128, 128, 2, 3, bn=True, args=A(), final_dim="output_dim").to(dev).train()
        return m, triplet.tripletnet(m), FlatTrainer(m, lr=1e-3, clip=2.0), triplet.MarginRankingLoss(margin=MARGIN)

    # (a)
    m_a, net_a, tr_a, crit_a = make()
    t0 = time.perf_counter()
    st = triplet.TripletStream(net_a, pool, max_steps=STEPS)
    t_pack = time.perf_counter() - t0
    gs_a = GraphedStep(tr_a, st.loss(crit_a, tgt), warmup=3)
    # (b)
    m_b, net_b, tr_b, crit_b = make()
    parts = [triplet.resident_graph(pool[i], dev, net_b._resident) for i in sched[0]]
    g_b, x_b, _, sizes_b = triplet.assemble(parts, dev)
    gs_b = GraphedStep(tr_b, lambda: crit_b(*net_b._embed(x_b, g_b, sizes_b, x_b)[:2], tgt), warmup=3)
    # (c)
    m_c, net_c, tr_c, crit_c = make()
    for o in pool:                                           # every graph resident before the timed windows
        triplet.resident_graph(o, dev, net_c._resident)

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
        for ids in sched[w * per:w * per + EAGER_STEPS]:
            tr_c.step(lambda: crit_c(*net_c(*[pool[i] for i in ids])[:2], tgt))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / EAGER_STEPS * 1e6

    st.load(sched)
    replayed(gs_a, 50); replayed(gs_b, 50); eager(0)         # warm-up of every row
    st.load(sched)                                           # the epoch starts here: window w replays entries [w * per, (w + 1) * per)
    times = {"a": [], "b": [], "c": []}
    losses = {"a": [], "b": []}                              # the loss of each window's last step: is the hinge still active?
    for w in range(REPS):
        times["a"].append(replayed(gs_a, per))
        times["b"].append(replayed(gs_b, per))
        times["c"].append(eager(w))
        losses["a"].append(gs_a.loss_value()); losses["b"].append(gs_b.loss_value())
    pos = st.position()

    # the gather launch alone: a burst of launches on one stream (each waits for the one before: launch + latency chain, no step around it)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    burst = []
    for _ in range(REPS):
        e0.record()
        for _ in range(BURST):
            st.gather()
        e1.record()
        e1.synchronize()
        burst.append(e0.elapsed_time(e1) / BURST * 1e3)

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
    print("DD-shaped, %d graphs (%d..%d nodes, mean %.0f), Nmax %d, %d features, 3 layers x 128, final_dim output_dim, margin %g, clip 2.0 + Adam; "
          "schedule of %d seeded triplets; median [min .. max] of %d alternating windows"
          % (GRAPHS, sizes.min(), sizes.max(), sizes.mean(), ar.nmax, fin, MARGIN, STEPS, REPS))
    print("  arena: %.1f MB (%d int32 words, %d x %d feature table), packed + uploaded in %.2f s; slot: %d rows + %d ghost slots, tail %d"
          % ((ar.buf.nbytes + ar.feats.nbytes + ar.records.nbytes) / 1e6, ar.words, ar.feats.shape[0], ar.ld, t_pack, st.row_cap,
             st.g.ghost_slots_fixed, st.tail_cap))
    print("  (a) streamed, a new triplet per replay, one hipGraph      : %s   %d device kernels; cursor after the windows: %d"
          % (fmt(times["a"]), len(ka), pos))
    print("  (b) resident triplet (%s nodes) replayed, one hipGraph : %s   %d device kernels"
          % ("/".join(str(int(s)) for s in sizes_b), fmt(times["b"]), len(kb)))
    print("  (c) eager drop-in, same objects in the same order         : %s" % fmt(times["c"]))
    print("      (a) faster than (c) in every window: %s   time (c) / time (a) = %.2fx" % (all(x < y for x, y in zip(times["a"], times["c"])), med["c"] / med["a"]))
    print("      time (a) / time (b) = %.3f; as a rate, (a) runs at %.2f of (b) (bench.py --ingest: a new mini-batch per replay runs at 0.83-0.85 of its resident step's rate)"
          % (med["a"] / med["b"], med["b"] / med["a"]))
    print("  gather launch alone, burst of %d launches (not a step)    : %s" % (BURST, fmt(burst).replace("us/step", "us/launch")))
    print("      (a) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in ka).most_common(40)))
    print("      loss of each window's last step (margin %g: the hinge is active while the loss is above 0): (a) %s  (b) %s"
          % (MARGIN, " ".join("%.0f" % v for v in losses["a"]), " ".join("%.0f" % v for v in losses["b"])))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
