#!/usr/bin/env python3
"""The EigenGCN triplet stream, measured (Code/eigengcn/train_triplet.py:289-317: ONE new triplet per optimiser step): 256 DD-shaped
synthetic graphs (scripts/eigen_step.py's generator and chunked clusters), Nmax 1000, WavePoolingGcnEncoder 3 layers h128, pool_sizes
'10', J = 2, Jf = 1, con_final 1, pred_hidden_dims [50] (the configuration of scripts/eigen_triplet_step.py, label_dim 6),
eigen_triplet.MarginRankingLoss + clip 2.0 + Adam under FlatTrainer, a seeded schedule of 2,000 triplets.  Three figures in ONE
process, five alternating windows each:

  (a) streamed: eigen_stream.TripletStream, a NEW triplet per replay of one hipGraph (a window = 400 consecutive schedule entries)
  (b) the resident single triplet replayed from one hipGraph (the figure of scripts/eigen_triplet_step.py's row (a), re-taken here with
      the same margin and lr = 0, so that the hinge stays active on the one triplet)
  (c) the eager drop-in, tripletnet.forward(a, p, n), fed the same objects in the same order (a window = 40 entries)

plus the device kernels of one streamed and one resident step.

    python scripts/eigen_stream_step.py                in a child process under its own time limit
    python scripts/eigen_stream_step.py run            in this process

Replayed rows: device events around the window's replays; the eager row: host clock around steps that end in a synchronise.
Reported: median [min .. max] over the windows.  (A ``.graph`` dict of this size holds five dense [1000, 1000] arrays: 5 GB of host
memory for the 256 objects while the script runs.)"""
import os
import subprocess
import sys
import time

GRAPHS, STEPS, REPS, EAGER_STEPS = 256, 2000, 5, 40
NMAX, J, JF, LABEL_DIM = 1000, 2, 1, 6
MARGIN = 1.0e6          # far above any distance the model reaches in the run: the hinge stays active, every timed step carries real gradients
LIMIT_S = 600


def main_all():
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "run"])
    if r.returncode != 0:                                    # (a fault or a time-out: nothing more is started on the device)
        print("the run ended with status %d" % r.returncode)
        sys.exit(r.returncode)


def main_one():
    import types
    import numpy as np
    import torch
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import eigen_step
    from two_stage_gnn_amd import eigen_encoders as EE, eigen_pool as ep, eigen_stream, eigen_triplet as ET
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    dev = torch.device("cuda", torch.cuda.current_device())
    args = types.SimpleNamespace(bias=True, con_final=1, pool_sizes="10", num_pool_matrix=J, num_pool_final_matrix=JF)
    per = STEPS // REPS

    class Graph:
        pass

    t0 = time.perf_counter()
    results, xp, _ = eigen_step.batch(7, B=GRAPHS, nmax=NMAX)
    fin = int(xp.shape[2])
    pool = []
    f32 = lambda t: np.ascontiguousarray(t[0].numpy().astype(np.float32))
    for b, r in enumerate(results):
        adj, pooled, n0, nl, pm = ep.dense_inputs([r], NMAX, J, JF)
        g = Graph()
        g.graph = {"adj": f32(adj), "feats": xp[b], "num_nodes": int(n0[0]), "adj_pool_1": f32(pooled[0]), "num_nodes_1": int(nl[0][0])}
        for j in range(J):
            g.graph["pool_adj_0_%d" % j] = f32(pm[0][j])
        for j in range(JF):
            g.graph["pool_adj_1_%d" % j] = f32(pm[1][j])
        pool.append(g)
    del results
    t_data = time.perf_counter() - t0
    sizes = np.array([g.graph["num_nodes"] for g in pool])
    sched = np.random.default_rng(1).integers(0, GRAPHS, size=(STEPS, 3))
    tgt = torch.full((1,), -1.0, device=dev)

    def make(lr=1e-3):
        torch.manual_seed(5)
        m = EE.WavePoolingGcnEncoder(NMAX, fin, 128, 128, LABEL_DIM, 3, num_pool_matrix=J, num_pool_final_matrix=JF, pool_sizes=[10],
                                     pred_hidden_dims=[50], args=args).train()
        return m, ET.tripletnet(m, args), FlatTrainer(m, lr=lr, clip=2.0), ET.MarginRankingLoss(margin=MARGIN)

    # (a)
    m_a, net_a, tr_a, crit_a = make()
    t0 = time.perf_counter()
    st = eigen_stream.TripletStream(net_a, pool, max_steps=STEPS)
    t_pack = time.perf_counter() - t0
    gs_a = GraphedStep(tr_a, st.loss(crit_a, tgt), warmup=3)
    # (b)  (lr = 0: Adam on ONE triplet would move every weight the same way step after step; the launches are the same, the
    # parameters stay, the hinge stays active, every timed step carries real gradients)
    m_b, net_b, tr_b, crit_b = make(lr=0.0)
    fixed = [pool[i] for i in sched[0]]
    batch_b = net_b.batch(*fixed)
    gs_b = GraphedStep(tr_b, lambda: crit_b(*net_b.embed(batch_b)[:2], tgt), warmup=3)
    # (c)
    m_c, net_c, tr_c, crit_c = make()
    for o in pool:                                           # every graph resident before the timed windows
        ET.resident_graph(o, dev, net_c.cache, 1, J, JF)

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
    replayed(gs_a, 50); replayed(gs_b, 50)                   # warm-up of every row (the eager row: every window's size triples once)
    for w in range(REPS):
        eager(w)
    st.load(sched)                                           # the epoch starts here: window w replays entries [w * per, (w + 1) * per)
    times = {"a": [], "b": [], "c": []}
    losses = {"a": [], "b": []}
    for w in range(REPS):
        times["a"].append(replayed(gs_a, per))
        times["b"].append(replayed(gs_b, per))
        times["c"].append(eager(w))
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

    def per_kernel(ev):
        us = Counter()
        for e in ev:
            us[short(e.name)] += e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
        return ", ".join("%s %.1f" % kv for kv in us.most_common(12))

    ka, kb = kernels(gs_a), kernels(gs_b)
    fmt = lambda v: "%8.1f [%8.1f .. %8.1f] us/step" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in times.items()}
    ar = st.arena
    need_n = ar.records[:, 2:4][sched].sum(1)
    need_z = ar.records[:, 6:8][sched].sum(1)
    print("DD-shaped: %d graphs (%d..%d nodes, mean %.0f; built in %.0f s), Nmax %d, %d features; WavePoolingGcnEncoder 3 layers h128, "
          "pool_sizes '10', J %d, Jf %d, con_final 1, pred_hidden_dims [50], label_dim %d; margin %g + clip 2.0 + Adam under FlatTrainer; "
          "schedule of %d seeded triplets; median [min .. max] of %d alternating windows"
          % (GRAPHS, sizes.min(), sizes.max(), sizes.mean(), t_data, NMAX, fin, J, JF, LABEL_DIM, MARGIN, STEPS, REPS))
    print("  arena: %.1f MB, packed + uploaded in %.2f s; capacities: rows %s, entries %s; the schedule's triplets take %d..%d rows (mean "
          "%.0f) and %d..%d entries at level 0, %d..%d rows at the pooled level"
          % ((ar.buf.nbytes + ar.records.nbytes) / 1e6, t_pack, list(st.row_caps), list(st.nnz_caps), need_n[:, 0].min(), need_n[:, 0].max(),
             need_n[:, 0].mean(), need_z[:, 0].min(), need_z[:, 0].max(), need_n[:, 1].min(), need_n[:, 1].max()))
    print("  (a) streamed, a new triplet per replay, one hipGraph        : %s   %d device kernels, %s; cursor after the windows: %d"
          % (fmt(times["a"]), len(ka), gs_a.describe(), pos))
    print("  (b) resident triplet (%s nodes) replayed, one hipGraph, lr 0 : %s   %d device kernels, %s"
          % ("/".join(str(int(o.graph["num_nodes"])) for o in fixed), fmt(times["b"]), len(kb), gs_b.describe()))
    print("  (c) eager drop-in, same objects in the same order           : %s" % fmt(times["c"]))
    print("      (a) faster than (c) in every window: %s   time (c) / time (a) = %.2fx"
          % (all(x < y for x, y in zip(times["a"], times["c"])), med["c"] / med["a"]))
    print("      time (a) / time (b) = %.3f   (the sibling streams: 0.94 .. 1.11; here the capacity is three times the LARGEST graph and the "
          "row-local kernels run over all of it)" % (med["a"] / med["b"]))
    print("      (a) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in ka).most_common(40)))
    print("      (b) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in kb).most_common(40)))
    print("      (a) device us of one step, largest first: " + per_kernel(ka))
    print("      (b) device us of one step, largest first: " + per_kernel(kb))
    print("      loss of each window's last step (margin %g: the hinge is active while the loss is above 0): (a) %s  (b) %s"
          % (MARGIN, " ".join("%.0f" % v for v in losses["a"]), " ".join("%.0f" % v for v in losses["b"])))
    sys.stdout.flush()


if __name__ == "__main__":
    if len(sys.argv) >= 2:
        main_one()
    else:
        main_all()
