#!/usr/bin/env python3
"""The EigenGCN family's triplet pre-training step (Code/eigengcn/train_triplet.py:292-317: ONE triplet per optimiser step) on DD-shaped
synthetic graphs: WavePoolingGcnEncoder, Nmax 1000, 89 features, 3 layers h128, pool_sizes '10', J = 2, Jf = 1, con_final 1,
pred_hidden_dims [50], chunked clusters (scripts/eigen_step.py); margin loss (alpha 1.5) + clip 2.0 + Adam under FlatTrainer.

  (a) eigen_triplet.tripletnet on a resident triplet, replayed from one hipGraph (+ the launch inventory of one step)
  (b) the drop-in fed eagerly from ``.graph`` dicts drawn from a fixed set of 64 (the resident cache at work)
  (c) what the package offered before eigen_triplet: three WavePoolingGcnEncoder forwards at B = 1 on prebuilt one-graph EigenBatches +
      F.pairwise_distance + torch.nn.MarginRankingLoss, replayed from one hipGraph on the same triplet as (a)
  (d) the same composition eager from the dicts' dense [1, Nmax, Nmax] tensors, on the same draws as (b)

    python scripts/eigen_triplet_step.py                 label_dim 6 and 64, each in a child process under its own time limit
    python scripts/eigen_triplet_step.py 6               one configuration in this process
    python scripts/eigen_triplet_step.py 6 trace         only (a), 200 replays (the program to put behind a kernel tracer)

The four rows are timed in alternating windows, REPS times; reported: median [min .. max] over the windows.
(a) / (c): device events around 200 replays; (b) / (d): host clock around the eager steps ending in a synchronise."""
import os
import subprocess
import sys
import time

LABEL_DIMS = [6, 64]
REPS, REPLAYS, EAGER_STEPS, POOL = 5, 200, 40, 64
NMAX, J, JF = 1000, 2, 1
LIMIT_S = 420


def main_all():
    for ld in LABEL_DIMS:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), str(ld)])
        if r.returncode != 0:                                # (a fault or a time-out: nothing more is started on the device)
            print("configuration label_dim %d ended with status %d: stopping" % (ld, r.returncode))
            sys.exit(r.returncode)


def main_one(label_dim, trace_only=False):
    import types
    import numpy as np
    import torch
    import torch.nn.functional as F
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import eigen_step
    from two_stage_gnn_amd import eigen_encoders as EE, eigen_pool as ep, eigen_triplet as ET
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    dev = torch.device("cuda", torch.cuda.current_device())
    args = types.SimpleNamespace(bias=True, con_final=1, pool_sizes="10", num_pool_matrix=J, num_pool_final_matrix=JF)

    class Graph:
        pass

    # a fixed set of graph objects, as a TripletSampler draws from a training set: the dicts cross_val.py would have prepared
    n_pool = 3 if trace_only else POOL
    results, xp, _ = eigen_step.batch(7, B=n_pool, nmax=NMAX)
    fin = int(xp.shape[2])
    pool = []
    for b, r in enumerate(results):
        adj, pooled, n0, nl, pm = ep.dense_inputs([r], NMAX, J, JF)
        f32 = lambda t: np.ascontiguousarray(t[0].numpy().astype(np.float32))
        g = Graph()
        g.graph = {"adj": f32(adj), "feats": xp[b], "num_nodes": int(n0[0]), "adj_pool_1": f32(pooled[0]), "num_nodes_1": int(nl[0][0])}
        for j in range(J):
            g.graph["pool_adj_0_%d" % j] = f32(pm[0][j])
        for j in range(JF):
            g.graph["pool_adj_1_%d" % j] = f32(pm[1][j])
        g.result = r
        pool.append(g)
    sizes = np.array([g.graph["num_nodes"] for g in pool])
    draws = np.random.default_rng(1).integers(0, n_pool, size=(EAGER_STEPS, 3))
    fixed = [pool[0], pool[1], pool[2]]
    tgt = torch.full((1,), -1.0, device=dev)

    def make():
        torch.manual_seed(5)
        net = EE.WavePoolingGcnEncoder(NMAX, fin, 128, 128, label_dim, 3, num_pool_matrix=J, num_pool_final_matrix=JF, pool_sizes=[10],
                                       pred_hidden_dims=[50], args=args).train()
        return net, FlatTrainer(net, lr=1e-3, clip=2.0)

    # (a)
    net_a, tr_a = make()
    t_a, crit_a = ET.tripletnet(net_a, args), ET.MarginRankingLoss(margin=1.5)
    batch_a = t_a.batch(*fixed)
    gs_a = GraphedStep(tr_a, lambda: crit_a(*t_a.embed(batch_a)[:2], tgt), warmup=3)

    def replayed(gs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(gs.stream)
        for _ in range(REPLAYS):
            gs.step()
        e1.record(gs.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / REPLAYS * 1e3

    if trace_only:
        replayed(gs_a)
        print("(a) replayed %d steps, label_dim %d, %s, loss %.5f" % (REPLAYS, label_dim, gs_a.describe(), gs_a.loss_value()))
        return

    # (c): prebuilt one-graph batches and feature rows of the same triplet
    def rows_of(g):
        n = g.graph["num_nodes"]
        ld = (fin + 3) // 4 * 4
        x = torch.zeros(n + NMAX, ld, device=dev)
        x[:n, :fin] = torch.from_numpy(g.graph["feats"][:n]).to(dev)
        return x

    pre = [(rows_of(g), ep.collate([g.result], NMAX, J, JF, device=dev)) for g in fixed]
    net_c, tr_c = make()
    crit_c = torch.nn.MarginRankingLoss(margin=1.5)

    def loss_c():
        e = [net_c(x, eb) for x, eb in pre]
        return crit_c(F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2), tgt)
    gs_c = GraphedStep(tr_c, loss_c, warmup=3)

    # (b), (d)
    net_b, tr_b = make()
    t_b, crit_b = ET.tripletnet(net_b, args), ET.MarginRankingLoss(margin=1.5)
    net_d, tr_d = make()
    crit_d = torch.nn.MarginRankingLoss(margin=1.5)

    def dense_forward(net, g):
        """the reference's tripletnet.forward for one graph: every dense tensor uploaded with a leading batch axis of 1"""
        d = g.graph
        up = lambda a: torch.from_numpy(a).unsqueeze(0).to(dev)
        pm = {0: [up(d["pool_adj_0_%d" % j]) for j in range(J)], 1: [up(d["pool_adj_1_%d" % j]) for j in range(JF)]}
        return net(up(d["feats"]), up(d["adj"]), [up(d["adj_pool_1"])], [d["num_nodes"]], [[d["num_nodes_1"]]], pm)

    def loss_d(trip):
        e = [dense_forward(net_d, g) for g in trip]
        return crit_d(F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2), tgt)

    def eager(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(EAGER_STEPS):
            step([pool[j] for j in draws[i]])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / EAGER_STEPS * 1e6

    step_b = lambda trip: tr_b.step(lambda: crit_b(*t_b(*trip)[:2], tgt))
    step_d = lambda trip: tr_d.step(lambda: loss_d(trip))
    rows = {"a": lambda: replayed(gs_a), "c": lambda: replayed(gs_c), "b": lambda: eager(step_b), "d": lambda: eager(step_d)}
    for f in rows.values():                                  # warm-up: every shape of the timed windows (all draws seen once)
        f()
    times = {k: [] for k in rows}
    for _ in range(REPS):
        for k, f in rows.items():
            times[k].append(f())

    def kernels(gs):
        """the device kernels of one profiled replay (ONE profiler session per row: the profiler sometimes hands back no events for a
        replay, and the count is then reported as not available rather than asked for again)"""
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs.step()
            torch.cuda.synchronize()
        return [e for e in prof.events() if e.device_type.name == "CUDA"]

    def short(n):
        n = n.replace("void ", "").replace("(anonymous namespace)::", "").replace("at::native::", "")
        return n.split("(")[0].split("<")[0][:40] or n[:40]

    ka, kc = kernels(gs_a), kernels(gs_c)
    count = lambda ev: ("%d device kernels" % len(ev)) if ev else "device kernels n/a (no profiler events)"
    med = lambda k: float(np.median(times[k]))
    fmt = lambda v: "%8.1f [%8.1f .. %8.1f] us/step" % (float(np.median(v)), min(v), max(v))
    nodes = "/".join(str(g.graph["num_nodes"]) for g in fixed)
    print("DD-shaped, Nmax %d, %d features, 3 layers h128, pool_sizes '10', J %d, Jf %d, con_final 1, pred_hidden_dims [50], label_dim %d; "
          "resident triplet of %s nodes; eager rows: %d draws from %d graphs (%d..%d nodes); median [min .. max] of %d alternating windows"
          % (NMAX, fin, J, JF, label_dim, nodes, EAGER_STEPS, POOL, sizes.min(), sizes.max(), REPS))
    print("  (a) tripletnet, resident triplet, one hipGraph          : %s   %s, %s" % (fmt(times["a"]), count(ka), gs_a.describe()))
    print("  (c) three B=1 forwards on EigenBatches + torch tail, graph: %s   %s, %s" % (fmt(times["c"]), count(kc), gs_c.describe()))
    print("  (b) tripletnet, eager from .graph dicts                 : %s   cache: %d graphs resident, %d uploads, %d hits"
          % (fmt(times["b"]), len(t_b.cache), t_b.cache.h2d, t_b.cache.hits))
    print("  (d) three B=1 forwards from the dense tensors, eager    : %s" % fmt(times["d"]))
    print("      ratios of the medians: (c) / (a) = %.2f   (d) / (b) = %.2f;  windows overlap: (a)-(c) %s, (b)-(d) %s"
          % (med("c") / med("a"), med("d") / med("b"), "yes" if max(times["a"]) >= min(times["c"]) else "no",
             "yes" if max(times["b"]) >= min(times["d"]) else "no"))
    print("      (a) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in ka).most_common(40)))
    print("      losses after the run: (a) %.5f (c) %.5f" % (gs_a.loss_value(), gs_c.loss_value()))
    sys.stdout.flush()


if __name__ == "__main__":
    if len(sys.argv) >= 2:
        main_one(int(sys.argv[1]), trace_only=len(sys.argv) >= 3 and sys.argv[2] == "trace")
    else:
        main_all()
