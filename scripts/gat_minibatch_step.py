#!/usr/bin/env python3
"""The GAT mini-batch stream, measured (Code/sage+gat+diffpool/train.py:104-131 with --method=GAT: ONE new batch per optimiser step):
512 DD-shaped synthetic graphs, Nmax 1000, DGATEncoderGraph 2 layers x 4 heads x 64, final_dim number_classes, model.loss (soft-max
cross-entropy) + clip 2.0 + Adam under FlatTrainer + GraphedStep, a seeded schedule of 2,000 entries of distinct graphs.  Per batch size
(32: BASELINE config 3's; 1: the reference's default) five figures in ONE process, five alternating windows each:

  (a) streamed: gat_stream.MiniBatchStream at its default capacity (the sums of the B largest nr / nnz / k)
  (b) streamed at gat_stream.schedule_capacity (the schedule's own maxima)
  (c) the schedule's mean-size entry as an exact resident batch replayed from one hipGraph (config 3's full optimiser step)
  (d) the eager loop: MiniBatchStream.eager_loss on the same objects in the same order — resident pieces, gat_triplet.assemble,
      an eager FlatTrainer.step (a window = 40 entries)
  (e) the gather launch alone: a burst of launches between two events, and single launches each between two events

plus the device kernels of one streamed and one resident step.

    python scripts/gat_minibatch_step.py               both batch sizes, each in a child process under its own time limit
    python scripts/gat_minibatch_step.py 32            one batch size in this process

Replayed rows: device events around the window's replays; the eager row: host clock around steps that end in a synchronise.
Reported: median [min .. max] over the windows."""
import os
import subprocess
import sys
import time

GRAPHS, STEPS, REPS, EAGER_STEPS, SINGLE, BURST = 512, 2000, 5, 40, 50, 200
BATCHES = (32, 1)
LIMIT_S = 400


def main_all():
    for B in BATCHES:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), str(B)])
        if r.returncode != 0:                                # (a fault or a time-out: nothing more is started on the device)
            print("B = %d ended with status %d: stopping" % (B, r.returncode))
            sys.exit(r.returncode)


def main_one(B):
    import numpy as np
    import torch
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import gat_encoders as G, gat_stream as GS, gat_triplet as GT, resident as R
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    dev = torch.device("cuda")
    per = STEPS // REPS
    pool, fin = dense_dataset(GRAPHS)
    sizes = np.array([int(o.graph["num_nodes"]) for o in pool])
    labels = np.array([int(o.graph["label"]) for o in pool])
    rng = np.random.default_rng(1)
    sched = np.stack([rng.choice(GRAPHS, size=B, replace=False) for _ in range(STEPS)]).astype(np.int64)

    def make():
        torch.manual_seed(5)
        m = G.DGATEncoderGraph(fin, 64, 64, 2, None, num_layers=2, num_heads=[4, 4], final_dim="number_classes").to(dev).train()
        return m, FlatTrainer(m, lr=1e-3, clip=2.0)

    # (a), (b)
    m_a, tr_a = make()
    t0 = time.perf_counter()
    st_a = GS.MiniBatchStream(m_a, pool, B, max_steps=STEPS)
    t_pack = time.perf_counter() - t0
    gs_a = GraphedStep(tr_a, st_a.loss(), warmup=3)
    m_b, tr_b = make()
    own = GS.schedule_capacity(st_a.arena.records, sched)
    st_b = GS.MiniBatchStream(m_b, pool, B, max_steps=STEPS, **own)
    gs_b = GraphedStep(tr_b, st_b.loss(), warmup=3)
    assert st_a.fits(sched).all() and st_b.fits(sched).all()
    need = GS.entry_sums(st_a.arena.records, sched)
    # (c)
    m_c, tr_c = make()
    k_mean = int(np.argmin(np.abs(need[:, 0] - need[:, 0].mean())))
    parts = [GT.resident_piece(pool[int(i)], dev, R.cache_for(m_c)) for i in sched[k_mean]]
    x_c, g_c = GT.assemble(parts, dev, GT.head_counts(m_c))
    y_c = torch.from_numpy(labels[sched[k_mean]].astype(np.int64)).to(dev)
    gs_c = GraphedStep(tr_c, lambda: m_c.loss(m_c.head(GT.readout_rows(m_c, x_c, g_c)), y_c), warmup=3)
    # (d)
    m_d, tr_d = make()
    st_d = GS.MiniBatchStream(m_d, pool, B)
    for o in pool:                                           # every graph resident before the timed windows
        GT.resident_piece(o, dev, st_d._cache)

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
            tr_d.step(lambda: st_d.eager_loss(ids))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / EAGER_STEPS * 1e6

    st_a.load(sched); st_b.load(sched)
    replayed(gs_a, 50); replayed(gs_b, 50); replayed(gs_c, 50)   # warm-up of every row
    for w in range(REPS):
        eager(w)
    st_a.load(sched); st_b.load(sched)                        # the epoch starts here: window w replays entries [w * per, (w + 1) * per)
    times = {k: [] for k in "abcd"}
    losses = {"a": [], "b": []}
    for w in range(REPS):
        times["a"].append(replayed(gs_a, per))
        times["b"].append(replayed(gs_b, per))
        times["c"].append(replayed(gs_c, per))
        times["d"].append(eager(w))
        losses["a"].append(gs_a.loss_value()); losses["b"].append(gs_b.loss_value())
    pos = (st_a.position(), st_b.position())

    # (e)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    single, burst = {"a": [], "b": []}, {"a": [], "b": []}
    for key, st in (("a", st_a), ("b", st_b)):
        st.load(sched)
        for _ in range(SINGLE):
            e0.record(); st.gather(); e1.record(); e1.synchronize()
            single[key].append(e0.elapsed_time(e1) * 1e3)
        for _ in range(REPS):
            e0.record()
            for _ in range(BURST):
                st.gather()
            e1.record(); e1.synchronize()
            burst[key].append(e0.elapsed_time(e1) / BURST * 1e3)

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

    def per_kernel(ev):
        us = Counter()
        for e in ev:
            us[short(e.name)] += e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
        return ", ".join("%s %.1f" % kv for kv in us.most_common(12))

    kb, kc = kernels(gs_b), kernels(gs_c)
    fmt = lambda v, unit="us/step": "%8.1f [%8.1f .. %8.1f] %s" % (float(np.median(v)), min(v), max(v), unit)
    med = {k: float(np.median(v)) for k, v in times.items()}
    ratio = lambda p, q: "%.3f [%.3f .. %.3f]" % (med[p] / med[q], min(x / y for x, y in zip(times[p], times[q])),
                                                  max(x / y for x, y in zip(times[p], times[q])))
    ar = st_a.arena
    print("DD-shaped: %d graphs (%d..%d nodes, mean %.0f), Nmax 1000, %d features; DGATEncoderGraph 2 layers x 4 heads x 64, final_dim "
          "number_classes; B %d; cross-entropy + clip 2.0 + Adam (lr 1e-3) under FlatTrainer; schedule of %d seeded entries of distinct graphs "
          "(rows %d..%d, mean %.0f; entries %d..%d); median [min .. max] of %d alternating windows of %d steps"
          % (GRAPHS, sizes.min(), sizes.max(), sizes.mean(), fin, B, STEPS, need[:, 0].min(), need[:, 0].max(), need[:, 0].mean(),
             need[:, 1].min(), need[:, 1].max(), REPS, per))
    print("  arena: %.1f MB, packed + uploaded in %.2f s" % ((ar.buf.nbytes + ar.records.nbytes) / 1e6, t_pack))
    for key, st, what in (("a", st_a, "default capacity  "), ("b", st_b, "schedule_capacity ")):
        print("  (%s) streamed, %s (%d rows, %d entries, %d listed columns): %s   %.0f graphs/s"
              % (key, what, st.row_cap, st.nnz_cap, st.iso_cap, fmt(times[key]), B / med[key] * 1e6))
    print("  (c) the mean-size entry (%d rows) as an exact resident batch, one hipGraph      : %s   %.0f graphs/s"
          % (int(need[k_mean, 0]), fmt(times["c"]), B / med["c"] * 1e6))
    print("  (d) eager: resident pieces + gat_triplet.assemble + an eager step, same order    : %s   %.0f graphs/s"
          % (fmt(times["d"]), B / med["d"] * 1e6))
    print("      time (b) / time (c) = %s   time (a) / time (b) = %s   (median; range of the per-window ratios)" % (ratio("b", "c"), ratio("a", "b")))
    print("      time (d) / time (b) = %s   (b) faster than (d) in every window: %s   (a) faster than (d) in every window: %s"
          % (ratio("d", "b"), all(x < y for x, y in zip(times["b"], times["d"])), all(x < y for x, y in zip(times["a"], times["d"]))))
    chunks = lambda: sum(-(-n // 2048) for n in (ar.top[0] + 1, ar.top[0] + 1, ar.top[1], ar.top[1], ar.top[1], ar.top[1],
                                                 ar.top[0] * ar.ldf, ar.top[0], max(ar.top[2], 1)))
    for key, st in (("a", st_a), ("b", st_b)):
        print("  (e) gather launch alone at (%s)'s capacity, %d workgroups: burst of %d %s; between two events %s"
              % (key, chunks() * (B + 1), BURST, fmt(burst[key], "us/launch"), fmt(single[key], "us")))
    print("      (b) %d device kernels, %s; (c) %d device kernels, %s" % (len(kb), gs_b.describe(), len(kc), gs_c.describe()))
    print("      (b) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in kb).most_common(40)))
    print("      (c) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in kc).most_common(40)))
    print("      (b) device us of one step, largest first: " + per_kernel(kb))
    print("      (c) device us of one step, largest first: " + per_kernel(kc))
    print("      cursors after the windows: %s; loss of each window's last step: (a) %s  (b) %s"
          % (pos, " ".join("%.4f" % v for v in losses["a"]), " ".join("%.4f" % v for v in losses["b"])))
    sys.stdout.flush()


if __name__ == "__main__":
    if len(sys.argv) >= 2:
        main_one(int(sys.argv[1]))
    else:
        main_all()
