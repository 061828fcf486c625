#!/usr/bin/env python3
"""The GAT encoder in the two-stage scheme, measured (train_triplet.py --method=GAT: ONE triplet per optimiser step, then evaluate()):
DD-shaped synthetic graphs, Nmax 1000, DGATEncoderGraph 2 layers x 4 heads x 64, final_dim output_dim, margin loss (alpha 1.5) +
clip 2.0 + Adam under FlatTrainer.

  step  (a) gat_triplet.tripletnet on a resident triplet, replayed from one hipGraph (+ the device kernels of one replayed step)
        (b) what the package offered before gat_triplet, replayed the same way in the same process: three B = 1 calls of the module on
            resident dense tensors, F.pairwise_distance, torch.nn.MarginRankingLoss
        (c) both fed eagerly from ``.graph`` dicts drawn from a fixed set of objects
  eval  (d) two_stage.evaluate on 1,168 graphs (1,051 / 117) through gat_triplet.tripletnet (packed chunks) against the plain loop of
            B = 1 forwards (a bare model, chunk=None), and embed_dataset at 32 / 64 / 128 / 256 graphs per chunk

    python scripts/gat_triplet_step.py               both parts, each in a child process under its own time limit
    python scripts/gat_triplet_step.py step          one part in this process
    python scripts/gat_triplet_step.py eval [N]

Rows of a part are timed in alternating windows, REPS times; reported: median [min .. max] over the windows.  Replayed rows: device
events around 200 replays; eager rows and (d): host clock around calls that end in a synchronise."""
import os
import subprocess
import sys
import time

REPS, REPLAYS, EAGER_STEPS, POOL = 5, 200, 60, 48
LIMIT_S = {"step": 400, "eval": 500}


def main_all():
    for part in ("step", "eval"):
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S[part]), sys.executable, os.path.abspath(__file__), part])
        if r.returncode != 0:                                # (a fault or a time-out: nothing more is started on the device)
            print("part %s ended with status %d: stopping" % (part, r.returncode))
            sys.exit(r.returncode)


def _setup():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)


def _model(fin, dev):
    import torch
    from two_stage_gnn_amd import gat_encoders as G
    torch.manual_seed(5)
    return G.DGATEncoderGraph(fin, 64, 64, 2, None, num_layers=2, num_heads=[4, 4], final_dim="output_dim").to(dev)


def main_step():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    _setup()
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import gat_triplet as GT
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    dev = torch.device("cuda")
    pool, fin = dense_dataset(POOL)                            # a fixed set of graph objects, as the triplet sampler draws from a training set
    draws = np.random.default_rng(1).integers(0, POOL, size=(EAGER_STEPS, 3))
    fixed = [pool[0], pool[1], pool[2]]
    tgt = torch.full((1,), -1.0, device=dev)

    def make():
        m = _model(fin, dev).train()
        return m, FlatTrainer(m, lr=1e-3, clip=2.0)

    def dense_inputs(o):
        d = o.graph
        return (torch.as_tensor(np.asarray(d["feats"], dtype=np.float32)[None], device=dev),
                torch.as_tensor(np.asarray(d["adj"], dtype=np.float32)[None], device=dev), np.array([int(d["num_nodes"])]))

    def parent_loss(m, crit, inputs):
        e = [m(h0, adj, n)[1] for h0, adj, n in inputs]
        return crit(F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2), tgt)

    # (a)
    m_a, tr_a = make()
    t_a, crit_a = GT.tripletnet(m_a), GT.MarginRankingLoss(margin=1.5)
    batch_a = t_a.batch(*fixed)
    gs_a = GraphedStep(tr_a, lambda: crit_a(*t_a.embed(batch_a)[:2], tgt), warmup=3)
    # (b): the dense tensors stay on the device, so the module's own conversion is cached after the warm-up steps
    m_b, tr_b = make()
    crit_b = torch.nn.MarginRankingLoss(margin=1.5)
    fixed_b = [dense_inputs(o) for o in fixed]
    gs_b = GraphedStep(tr_b, lambda: parent_loss(m_b, crit_b, fixed_b), warmup=3)
    # (c)
    m_c, tr_c = make()
    t_c, crit_c = GT.tripletnet(m_c), GT.MarginRankingLoss(margin=1.5)
    m_e, tr_e = make()
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

    step_c = lambda trip: tr_c.step(lambda: crit_c(*t_c(*trip)[:2], tgt))
    step_e = lambda trip: tr_e.step(lambda: parent_loss(m_e, crit_e, [dense_inputs(o) for o in trip]))
    rows = {"a": lambda: replayed(gs_a), "b": lambda: replayed(gs_b), "c_new": lambda: eager(step_c), "c_old": lambda: eager(step_e)}
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

    ka, kb = kernels(gs_a), kernels(gs_b)
    fmt = lambda v: "%8.1f [%8.1f .. %8.1f] us/step" % (float(np.median(v)), min(v), max(v))
    every = lambda new, old: all(x < y for x, y in zip(times[new], times[old]))
    nodes = "/".join(str(int(o.graph["num_nodes"])) for o in fixed)
    sizes = [int(o.graph["num_nodes"]) for o in pool]
    print("DD-shaped, Nmax 1000, %d features, 2 layers x 4 heads x 64, final_dim output_dim; resident triplet of %s nodes; eager rows: %d draws "
          "from %d graphs (%d..%d nodes); median [min .. max] of %d alternating windows" % (fin, nodes, EAGER_STEPS, POOL, min(sizes), max(sizes), REPS))
    print("  (a) gat_triplet.tripletnet, resident triplet, one hipGraph : %s   %d device kernels, %s" % (fmt(times["a"]), len(ka), gs_a.describe()))
    print("  (b) three module B=1 calls + torch tail, one hipGraph      : %s   %d device kernels, %s" % (fmt(times["b"]), len(kb), gs_b.describe()))
    print("      (a) faster than (b) in every window: %s   (ratio of medians %.2fx)" % (every("a", "b"), np.median(times["b"]) / np.median(times["a"])))
    print("  (c) gat_triplet.tripletnet, eager from .graph dicts        : %s   cache: %d graphs resident, %d uploads, %d hits"
          % (fmt(times["c_new"]), len(t_c.cache), t_c.cache.h2d, t_c.cache.hits))
    print("  (c) three module B=1 calls + torch tail, eager from dicts  : %s" % fmt(times["c_old"]))
    print("      new faster than old in every window: %s   (ratio of medians %.2fx)"
          % (every("c_new", "c_old"), np.median(times["c_old"]) / np.median(times["c_new"])))
    print("      (a) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in ka).most_common(40)))
    print("      losses after the run: (a) %.5f (b) %.5f" % (gs_a.loss_value(), gs_b.loss_value()))
    sys.stdout.flush()


def main_eval(n_graphs=1168):
    import numpy as np
    import torch
    _setup()
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import gat_triplet as GT, two_stage as TS
    dev = torch.device("cuda")
    graphs, fin = dense_dataset(n_graphs)
    n_val = max(1, int(round(0.1 * n_graphs)))
    train, val = graphs[:n_graphs - n_val], graphs[n_graphs - n_val:]
    m = _model(fin, dev)
    tnet = GT.tripletnet(m)

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    chunked = lambda: TS.evaluate(train, val, tnet, n_neighbors=3)
    plain = lambda: TS.evaluate(train, val, m, n_neighbors=3)               # a bare model, chunk=None: the plain loop
    t_first, res_c = wall(chunked)                                          # first evaluation: the graphs become resident
    _, res_p = wall(plain)
    times = {"chunked": [], "plain": []}
    for _ in range(REPS):
        times["chunked"].append(wall(chunked)[0])
        times["plain"].append(wall(plain)[0])
    sweep = {}
    for c in (32, 64, 128, 256):
        TS.embed_dataset(tnet, graphs, chunk=c)
        sweep[c] = [wall(lambda: TS.embed_dataset(tnet, graphs, chunk=c))[0] for _ in range(REPS)]
    emb_c, emb_p = TS.embed_dataset(tnet, graphs), TS.embed_dataset(m, graphs)
    fmt = lambda v: "%9.2f [%9.2f .. %9.2f] ms" % (float(np.median(v)), min(v), max(v))
    print("DD-shaped, Nmax 1000: %d graphs (%d train / %d validation), 2 layers x 4 heads x 64, embedding width %d, k = 3; median [min .. max] of "
          "%d alternating windows" % (n_graphs, len(train), len(val), int(emb_c.size(1)), REPS))
    print("  (d) evaluate, gat_triplet.tripletnet (packed chunks of %d) : %s   (first call, graphs not yet resident: %.1f ms)"
          % (GT.DEFAULT_CHUNK, fmt(times["chunked"]), t_first))
    print("  (d) evaluate, bare model (plain loop of B = 1 forwards)     : %s" % fmt(times["plain"]))
    print("      chunked faster in every window: %s   (ratio of medians %.1fx)"
          % (all(a < b for a, b in zip(times["chunked"], times["plain"])), np.median(times["plain"]) / np.median(times["chunked"])))
    print("  embed_dataset by graphs per chunk: " + ", ".join("%d: %s" % (c, fmt(v)) for c, v in sweep.items()))
    best = min(sweep, key=lambda c: float(np.median(sweep[c])))
    print("      fastest: %d graphs per chunk (gat_triplet.DEFAULT_CHUNK = %d)" % (best, GT.DEFAULT_CHUNK))
    print("  largest |chunked - plain| embedding entry: %.3e (largest entry %.3e)" % (float((emb_c - emb_p).abs().max()), float(emb_p.abs().max())))
    print("  metrics, chunked:", {k: round(v, 4) for k, v in res_c.items()})
    print("  metrics, plain  :", {k: round(float(v), 4) for k, v in res_p.items()})
    sys.stdout.flush()


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "step":
        main_step()
    elif len(sys.argv) >= 2 and sys.argv[1] == "eval":
        main_eval(int(sys.argv[2]) if len(sys.argv) > 2 else 1168)
    else:
        main_all()
