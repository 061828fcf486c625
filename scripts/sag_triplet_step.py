#!/usr/bin/env python3
"""The SAGPool family's triplet pre-training step (Code/sag/train_triplet.py:203-214: ONE triplet per optimiser step) on IMDB-B-shaped and
DD-shaped synthetic graphs: sag_layers.Net nhid 128, ratio 0.5, final_dim 64, margin loss (alpha 1.5) + clip 2.0 + Adam under FlatTrainer.

  (a) sag_triplet.tripletnet on a resident triplet, replayed from one hipGraph (+ the launch inventory of one step)
  (b) the drop-in fed eagerly from Data objects drawn from a fixed set (the resident cache at work)
  (c) what the package offered before sag_triplet: three Net forwards at B = 1 + F.pairwise_distance + torch.nn.MarginRankingLoss,
      replayed from one hipGraph on the same triplet as (a), and eager on the same draws as (b)

    python scripts/sag_triplet_step.py                 every configuration, each in a child process under its own time limit
    python scripts/sag_triplet_step.py DD gcn          one configuration in this process

The four rows of a configuration are timed in alternating windows, REPS times; reported: median [min .. max] over the windows.
(a) / (c) replayed: device events around 200 replays; (b) / (c) eager: host clock around 100 steps ending in a synchronise."""
import os
import subprocess
import sys
import time

CONFIGS = [("IMDB-BINARY", "gcn"), ("IMDB-BINARY", "sage"), ("DD", "gcn"), ("DD", "sage")]
REPS, REPLAYS, EAGER_STEPS, POOL = 5, 200, 100, 64
LIMIT_S = 280


def main_all():
    for shape, conv in CONFIGS:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), shape, conv])
        if r.returncode != 0:                                # (a fault or a time-out: nothing more is started on the device)
            print("configuration %s %s ended with status %d: stopping" % (shape, conv, r.returncode))
            sys.exit(r.returncode)


def main_one(shape, conv):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from two_stage_gnn_amd import sag_layers as S, sag_triplet as ST, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    dev = torch.device("cuda")

    class Data:
        pass

    # a fixed set of graph objects, as a TripletSampler draws from a training set
    hb = synthetic.host_batch(7, POOL, shape, 1000 if shape == "DD" else 136)
    sizes = hb["sizes"]
    gp = np.concatenate([[0], np.cumsum(sizes)])
    rp, col, fin = hb["rowptr"], hb["col"], int(hb["x"].shape[1])
    pool = []
    for b in range(POOL):
        lo, hi = int(gp[b]), int(gp[b + 1])
        c = col[rp[lo]:rp[hi]].astype(np.int64) - lo
        t = np.repeat(np.arange(hi - lo), np.diff(rp[lo:hi + 1]))
        d = Data()
        d.x = torch.from_numpy(np.ascontiguousarray(hb["x"][lo:hi])).float().to(dev)
        d.edge_index = torch.from_numpy(np.stack([c, t.astype(np.int64)])).to(dev)
        pool.append(d)
    draws = np.random.default_rng(1).integers(0, POOL, size=(EAGER_STEPS, 3))
    fixed = [pool[0], pool[1], pool[2]]
    tgt = torch.full((1,), -1.0, device=dev)

    def make():
        torch.manual_seed(5)
        net = S.Net(fin, 128, 64, 0.5, 0.5, conv=conv).to(dev).train()
        return net, FlatTrainer(net, lr=1e-3, clip=2.0)

    def parent_loss(net, crit, trip):
        e = [net(d) for d in trip]
        return crit(F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2), tgt)

    # (a)
    net_a, tr_a = make()
    t_a, crit_a = ST.tripletnet(net_a), ST.MarginRankingLoss(margin=1.5)
    batch_a = t_a.batch(*fixed)
    gs_a = GraphedStep(tr_a, lambda: crit_a(*t_a.embed(batch_a)[:2], tgt), warmup=3)
    # (c) replayed
    net_c, tr_c = make()
    crit_c = torch.nn.MarginRankingLoss(margin=1.5)
    gs_c = GraphedStep(tr_c, lambda: parent_loss(net_c, crit_c, fixed), warmup=3)
    # (b), (c) eager
    net_b, tr_b = make()
    t_b, crit_b = ST.tripletnet(net_b), ST.MarginRankingLoss(margin=1.5)
    net_e, tr_e = make()
    crit_e = torch.nn.MarginRankingLoss(margin=1.5)

    def replayed(gs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(gs.stream)
        for _ in range(REPLAYS):
            gs.step()
        e1.record(gs.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / REPLAYS * 1e3

    def eager(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(EAGER_STEPS):
            step([pool[j] for j in draws[i]])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / EAGER_STEPS * 1e6

    step_b = lambda trip: tr_b.step(lambda: crit_b(*t_b(*trip)[:2], tgt))
    step_e = lambda trip: tr_e.step(lambda: parent_loss(net_e, crit_e, trip))
    rows = {"a": lambda: replayed(gs_a), "c_graph": lambda: replayed(gs_c), "b": lambda: eager(step_b), "c_eager": lambda: eager(step_e)}
    for f in rows.values():                                  # warm-up: every shape of the timed windows (all draws seen once)
        f()
    times = {k: [] for k in rows}
    for _ in range(REPS):
        for k, f in rows.items():
            times[k].append(f())

    def kernels(gs):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs.step()
            torch.cuda.synchronize()
        return [e for e in prof.events() if e.device_type.name == "CUDA"]

    def short(n):
        n = n.replace("void ", "").replace("(anonymous namespace)::", "").replace("at::native::", "")
        return n.split("(")[0].split("<")[0][:40] or n[:40]

    ka, kc = kernels(gs_a), kernels(gs_c)
    fmt = lambda v: "%8.1f [%8.1f .. %8.1f] us/step" % (float(np.median(v)), min(v), max(v))
    nodes = "/".join(str(int(d.x.size(0))) for d in fixed)
    print("%s-shaped, conv=%s, nhid 128, ratio 0.5, final_dim 64, dropout 0.5; resident triplet of %s nodes; eager rows: %d draws from %d graphs "
          "(%d..%d nodes); median [min .. max] of %d alternating windows" % (shape, conv, nodes, EAGER_STEPS, POOL, sizes.min(), sizes.max(), REPS))
    print("  (a) tripletnet, resident triplet, one hipGraph : %s   %d device kernels, %s" % (fmt(times["a"]), len(ka), gs_a.describe()))
    print("  (c) three Net B=1 forwards + torch tail, graph : %s   %d device kernels, %s" % (fmt(times["c_graph"]), len(kc), gs_c.describe()))
    print("  (b) tripletnet, eager from Data objects        : %s   cache: %d graphs resident, %d structure uploads, %d hits"
          % (fmt(times["b"]), len(t_b.cache), t_b.cache.h2d, t_b.cache.hits))
    print("  (c) three Net B=1 forwards + torch tail, eager : %s" % fmt(times["c_eager"]))
    print("      (a) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in ka).most_common(40)))
    print("      losses after the run: (a) %.5f (c) %.5f" % (gs_a.loss_value(), gs_c.loss_value()))
    sys.stdout.flush()


if __name__ == "__main__":
    if len(sys.argv) >= 3:
        main_one(sys.argv[1], sys.argv[2])
    else:
        main_all()
