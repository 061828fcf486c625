#!/usr/bin/env python3
"""The mini-batch stream, measured (train.py:104-131: ONE new mini-batch per optimiser step): DD-shaped synthetic TU dataset of 512
graphs (ingest.synthetic_dataset), B 32, Nmax 1000, GcnEncoderGraph 3 layers x 128, final_dim number_classes, node-label (one-hot)
features, cross-entropy + clip 2.0 + Adam under FlatTrainer + GraphedStep, a seeded schedule of 2,000 entries of distinct graphs.
Four step figures in ONE process, five alternating windows of 400 entries each:

  (a) streamed, minibatch_stream.MiniBatchStream at its default capacity (the sum of the 32 largest graphs)
  (b) streamed at row_cap = the schedule's own maximum (the capacity ingest.IngestPipeline uses)
  (c) ingest.IngestPipeline on the same dataset and schedule (collate threads, pinned staging, PCIe pull, three slots)
  (d) the schedule's mean-size entry as an exact resident batch replayed the same way (bench.py's resident_mean_size_batch)

plus (e) the gather launch alone: one launch between two events, and a burst of launches.

    python scripts/minibatch_stream_step.py

Every step row: host clock around the window's steps, ending in a device synchronise (the instrument bench.py --ingest uses).
Reported: median [min .. max] over the windows."""
import os
import sys
import time

GRAPHS, BATCH, NMAX, STEPS, REPS, BURST, SINGLE = 512, 32, 1000, 2000, 5, 200, 50


def main():
    import numpy as np
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    from two_stage_gnn_amd import dense_encoders as E, ingest
    from two_stage_gnn_amd import minibatch_stream as MS
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    dev = torch.device("cuda")
    ds = ingest.synthetic_dataset(seed=4242, n_graphs=GRAPHS, shape="DD", nmax=NMAX)
    fin = ds.num_node_labels
    rng = np.random.default_rng(77)
    sched = np.stack([rng.choice(GRAPHS, size=BATCH, replace=False) for _ in range(STEPS)]).astype(np.int64)
    rows = ds.sizes[sched].sum(1)
    per = STEPS // REPS

    class A:
        bias = True

    def make():
        torch.manual_seed(1234)
        m = E.GcnEncoderGraph(fin, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").to(dev).train()
        return m, FlatTrainer(m, lr=1e-3, clip=2.0, defer_loss=True)

    # (a), (b)
    m_a, tr_a = make()
    t0 = time.perf_counter()
    st_a = MS.MiniBatchStream(m_a, ds, BATCH, nmax=NMAX, features="node-label", max_steps=STEPS)
    t_pack = time.perf_counter() - t0
    gs_a = GraphedStep(tr_a, st_a.loss(), warmup=3)
    m_b, tr_b = make()
    tails = st_a.arena.records[:, 2].astype(np.int64)[sched].sum(1)
    st_b = MS.MiniBatchStream(m_b, ds, BATCH, nmax=NMAX, row_cap=int(rows.max()), tail_cap=max(int(tails.max()), st_a.max_tail),
                              features="node-label", max_steps=STEPS)
    gs_b = GraphedStep(tr_b, st_b.loss(), warmup=3)
    assert st_a.fits(sched).all() and st_b.fits(sched).all()
    # (c)
    m_c, tr_c = make()
    pipe = ingest.IngestPipeline(m_c, tr_c, ds, BATCH, NMAX, dev, list(sched))
    # (d)
    m_d, tr_d = make()
    k_mean = int(np.argmin(np.abs(rows - rows.mean())))
    g_d, x_d, y_d = ds.collate(sched[k_mean], NMAX, ds.features("node-label"), dev)
    gs_d = GraphedStep(tr_d, lambda: m_d.loss(m_d(x_d, g_d)[1], y_d), warmup=3)

    def replayed(gs, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            gs.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    def piped(part):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.run(part)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(part) * 1e6

    st_a.load(sched); st_b.load(sched)
    replayed(gs_a, 50); replayed(gs_b, 50); piped(list(sched[:50])); replayed(gs_d, 50)      # warm-up of every row
    st_a.load(sched); st_b.load(sched)                        # the epoch starts here: window w replays entries [w * per, (w + 1) * per)
    times = {k: [] for k in "abcd"}
    losses = {"a": [], "b": []}                              # the loss of each window's last step
    for w in range(REPS):
        times["a"].append(replayed(gs_a, per))
        times["b"].append(replayed(gs_b, per))
        times["c"].append(piped(list(sched[w * per:(w + 1) * per])))
        times["d"].append(replayed(gs_d, per))
        losses["a"].append(gs_a.loss_value()); losses["b"].append(gs_b.loss_value())
    pos = (st_a.position(), st_b.position())

    # (e) the gather launch alone
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    single, burst = {"a": [], "b": []}, {"a": [], "b": []}
    for key, st in (("a", st_a), ("b", st_b)):
        for _ in range(SINGLE):
            e0.record(); st.gather(); e1.record(); e1.synchronize()
            single[key].append(e0.elapsed_time(e1) * 1e3)
        for _ in range(REPS):
            e0.record()
            for _ in range(BURST):
                st.gather()
            e1.record(); e1.synchronize()
            burst[key].append(e0.elapsed_time(e1) / BURST * 1e3)

    fmt = lambda v, unit="us/step": "%8.1f [%8.1f .. %8.1f] %s" % (float(np.median(v)), min(v), max(v), unit)
    med = {k: float(np.median(v)) for k, v in times.items()}
    ratio = lambda p, q: "%.3f [%.3f .. %.3f]" % (med[p] / med[q], min(x / y for x, y in zip(times[p], times[q])),
                                                  max(x / y for x, y in zip(times[p], times[q])))
    ar = st_a.arena
    print("DD-shaped, %d graphs (%d..%d nodes, mean %.0f), B %d, Nmax %d, %d node labels (one-hot features written by the gather launch), "
          "3 layers x 128, final_dim number_classes, CE + clip 2.0 + Adam; schedule of %d seeded entries of distinct graphs "
          "(rows %d..%d, mean %.0f); median [min .. max] of %d alternating windows of %d steps"
          % (GRAPHS, ds.sizes.min(), ds.sizes.max(), ds.sizes.mean(), BATCH, NMAX, fin, STEPS, rows.min(), rows.max(), rows.mean(), REPS, per))
    print("  arena: %.1f MB (%d int32 words + %d node labels, no feature table), packed + uploaded in %.2f s"
          % ((ar.buf.nbytes + ar.node_label.nbytes + ar.records.nbytes) / 1e6, ar.words, ar.total_nodes, t_pack))
    print("  (a) streamed, default capacity (%5d rows + %d ghost slots, tail %d) : %s   %.0f graphs/s"
          % (st_a.row_cap, st_a.g.ghost_slots_fixed, st_a.tail_cap, fmt(times["a"]), BATCH / med["a"] * 1e6))
    print("  (b) streamed, the schedule's maximum (%5d rows, tail %d)             : %s   %.0f graphs/s"
          % (st_b.row_cap, st_b.tail_cap, fmt(times["b"]), BATCH / med["b"] * 1e6))
    print("  (c) IngestPipeline, same dataset and schedule (%5d rows)             : %s   %.0f graphs/s"
          % (pipe.row_cap, fmt(times["c"]), BATCH / med["c"] * 1e6))
    print("  (d) the mean-size entry (%d rows) as an exact resident batch          : %s   %.0f graphs/s"
          % (int(rows[k_mean]), fmt(times["d"]), BATCH / med["d"] * 1e6))
    print("      time (a) / time (d) = %s   time (b) / time (d) = %s   (median; range of the per-window ratios)" % (ratio("a", "d"), ratio("b", "d")))
    print("      time (b) / time (c) = %s   (b) faster than (c) in every window: %s" % (ratio("b", "c"), all(x < y for x, y in zip(times["b"], times["c"]))))
    print("      the default capacity over (b): time (a) / time (b) = %s" % ratio("a", "b"))
    for key, st in (("a", st_a), ("b", st_b)):
        print("  (e) gather launch alone at (%s)'s capacity, %d workgroups: between two events %s; burst of %d %s"
              % (key, -(-(st.row_cap + ar.nmax) // 8), fmt(single[key], "us"), BURST, fmt(burst[key], "us/launch")))
    print("      cursors after the windows: %s; loss of each window's last step: (a) %s  (b) %s"
          % (pos, " ".join("%.4f" % v for v in losses["a"]), " ".join("%.4f" % v for v in losses["b"])))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
