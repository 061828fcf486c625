#!/usr/bin/env python3
"""The DiffPool encoder in the two-stage scheme, measured (train_triplet.py --method=soft-assign: ONE triplet per optimiser step, then
evaluate()): DD-shaped synthetic graphs, Nmax 1000, SoftPoolingGcnEncoder 3 layers, hidden = embedding = assignment-hidden width h,
assign_ratio 0.1 (K = 100), one pooling level, final_dim output_dim, margin loss (alpha 1.5) + clip 2.0 + Adam under FlatTrainer.

  step  (a) a resident triplet (triplet.assemble once, net._embed in the loss function), replayed from one hipGraph, on the per-graph
            routes: the level-0 stacks on the fused GraphSage node, the pooled level on csrc/dense_stack_pg.hip (+ the device kernels
            of one replayed step)
        (b) the same with dense_encoders.PER_GRAPH_STACK and PER_GRAPH_DENSE off — every stack op by op, the route before those
            flags existed —, replayed the same way in the same process (timed eagerly, and said so, if it does not capture)
        (c) both fed eagerly from ``.graph`` dicts drawn from a fixed set of objects
  eval  (d) two_stage.evaluate on 1,168 graphs (1,051 / 117), route (a) against route (b), and embed_dataset at 32 / 64 / 128 graphs
            per chunk

    python scripts/diffpool_triplet_step.py               both parts, each in a child process under its own time limit
    python scripts/diffpool_triplet_step.py step [h ...]  one part in this process (default h: 64 128)
    python scripts/diffpool_triplet_step.py eval [N]

On a checkout without dense_encoders.PER_GRAPH_DENSE the rows of route (a) are absent and route (b) is what the package runs.
Rows of a part are timed in alternating windows, REPS times; reported: median [min .. max] over the windows.  Replayed rows: device
events around 200 replays; eager rows and (d): host clock around calls that end in a synchronise."""
import os
import subprocess
import sys
import time

REPS, REPLAYS, EAGER_STEPS, POOL = 5, 200, 40, 32
LIMIT_S = {"step": 500, "eval": 500}


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


def _model(fin, h, dev):
    import torch
    from two_stage_gnn_amd import dense_encoders as E
    torch.manual_seed(5)
    return E.SoftPoolingGcnEncoder(1000, fin, h, h, 2, 3, h, assign_ratio=0.1, num_pooling=1, linkpred=False, final_dim="output_dim").to(dev)


def _routed(on, fn):
    """fn with the per-graph routes on (route a) or off (route b) while it runs: the flags are read when the forward builds its nodes"""
    from two_stage_gnn_amd import dense_encoders as E

    def f(*args):
        old = (E.PER_GRAPH_STACK, getattr(E, "PER_GRAPH_DENSE", None))
        E.PER_GRAPH_STACK = bool(on)
        if old[1] is not None:
            E.PER_GRAPH_DENSE = bool(on)
        try:
            return fn(*args)
        finally:
            E.PER_GRAPH_STACK = old[0]
            if old[1] is not None:
                E.PER_GRAPH_DENSE = old[1]
    return f


def _has_new():
    from two_stage_gnn_amd import dense_encoders as E
    return hasattr(E, "PER_GRAPH_DENSE")


def step_rows(h, pool, fin, dev):
    import numpy as np
    import torch
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    from two_stage_gnn_amd import triplet as T3
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    draws = np.random.default_rng(1).integers(0, POOL, size=(EAGER_STEPS, 3))
    fixed = [pool[0], pool[1], pool[2]]
    tgt = torch.full((1,), -1.0, device=dev)
    new = _has_new()

    def make():
        m = _model(fin, h, dev).train()
        return m, T3.tripletnet(m), FlatTrainer(m, lr=1e-3, clip=2.0), T3.MarginRankingLoss(margin=1.5)

    def resident_step(on):
        """(callable that runs REPLAYS steps and returns us/step, how it runs, the GraphedStep or None)"""
        m, net, tr, crit = make()
        g, x, xa, sizes = T3.assemble([T3.resident_graph(o, dev, net._resident) for o in fixed], dev)
        loss = _routed(on, lambda: crit(*net._embed(x, g, sizes, x if xa is None else xa)[:2], tgt))
        try:
            gs = GraphedStep(tr, loss, warmup=3)
            gs.step()
        except Exception as e:                                   # does not capture: timed eagerly
            print("    route %s did not capture (%s: %s): timed eagerly" % ("a" if on else "b", type(e).__name__, str(e)[:120]))
            m, net, tr, crit = make()
            loss = _routed(on, lambda: crit(*net._embed(x, g, sizes, x if xa is None else xa)[:2], tgt))

            def eager_resident():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(REPLAYS):
                    tr.step(loss)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / REPLAYS * 1e6
            return eager_resident, "eager", None

        def replayed():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(gs.stream)
            for _ in range(REPLAYS):
                gs.step()
            e1.record(gs.stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / REPLAYS * 1e3
        return replayed, gs.describe(), gs

    def eager_dicts(on):
        m, net, tr, crit = make()
        one = _routed(on, lambda trip: crit(*net(*trip)[:2], tgt))

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(EAGER_STEPS):
                trip = [pool[j] for j in draws[i]]
                tr.step(lambda: one(trip))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / EAGER_STEPS * 1e6
        return run

    rows, how, graphed = {}, {}, {}
    for key, on in (("a", True), ("b", False)):
        if on and not new:
            continue
        rows[key], how[key], graphed[key] = resident_step(on)
        rows["c_" + key] = eager_dicts(on)
    for f in rows.values():                                      # warm-up: every shape of the timed windows (all draws seen once)
        f()
    times = {k: [] for k in rows}
    for _ in range(REPS):
        for k, f in rows.items():
            times[k].append(f())

    def kernels(gs):
        best = []
        for _ in range(3):                                       # (the profiler's first cycles in a process may drop events: keep the fullest)
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

    fmt = lambda v: "%8.1f [%8.1f .. %8.1f] us/step" % (float(np.median(v)), min(v), max(v))
    every = lambda a, b: all(x < y for x, y in zip(times[a], times[b]))
    nodes = "/".join(str(int(o.graph["num_nodes"])) for o in fixed)
    print("hidden %d: resident triplet of %s nodes, K = 100, pooled input width %d; eager rows: %d draws from %d graphs; median [min .. max] "
          "of %d alternating windows" % (h, nodes, 3 * h, EAGER_STEPS, POOL, REPS))
    label = {"a": "(a) per-graph routes (fused level 0 + dense_stack_pg)", "b": "(b) both flags off, op by op                        "}
    kern = {}
    for key in ("a", "b"):
        if key not in rows:
            print("  %s: not in this checkout" % label[key])
            continue
        kern[key] = kernels(graphed[key]) if graphed[key] is not None else None
        print("  %s, resident, %s: %s   %s" % (label[key], "one hipGraph" if graphed[key] is not None else "EAGER", fmt(times[key]),
                                              ("%d device kernels, %s" % (len(kern[key]), how[key])) if kern[key] is not None else how[key]))
    if "a" in rows:
        print("      (a) faster than (b) in every window: %s   (ratio of medians %.2fx)" % (every("a", "b"), np.median(times["b"]) / np.median(times["a"])))
    for key in ("a", "b"):
        if "c_" + key in rows:
            print("  (c) route (%s), eager from .graph dicts: %s" % (key, fmt(times["c_" + key])))
    if "c_a" in rows:
        print("      (c) route (a) faster than route (b) in every window: %s   (ratio of medians %.2fx)"
              % (every("c_a", "c_b"), np.median(times["c_b"]) / np.median(times["c_a"])))
    for key in ("a", "b"):
        if kern.get(key) is not None:
            print("      (%s) kernels: %s" % (key, ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in kern[key]).most_common(40))))
            print("      (%s) loss after the run: %.5f" % (key, graphed[key].loss_value()))
    sys.stdout.flush()


def main_step(hs):
    import torch
    _setup()
    from two_stage_eval import dense_dataset
    dev = torch.device("cuda")
    pool, fin = dense_dataset(POOL)                              # a fixed set of graph objects, as the triplet sampler draws from a training set
    print("DD-shaped, Nmax 1000, %d features, SoftPoolingGcnEncoder 3 layers, assign_ratio 0.1, one pooling level, final_dim output_dim; "
          "margin 1.5 + clip 2.0 + Adam under FlatTrainer; per-graph flags in this checkout: %s" % (fin, _has_new()))
    for h in hs:
        step_rows(h, pool, fin, dev)


def main_eval(n_graphs=1168, h=64):
    import numpy as np
    import torch
    _setup()
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import two_stage as TS
    dev = torch.device("cuda")
    graphs, fin = dense_dataset(n_graphs)
    n_val = max(1, int(round(0.1 * n_graphs)))
    train, val = graphs[:n_graphs - n_val], graphs[n_graphs - n_val:]
    m = _model(fin, h, dev)
    new = _has_new()

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    routes = {k: _routed(on, lambda: TS.evaluate(train, val, m, n_neighbors=3)) for k, on in (("a", True), ("b", False)) if new or not on}
    first, res = {}, {}
    for k, f in routes.items():                                  # first evaluation: the graphs become resident
        first[k], res[k] = wall(f)
    times = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            times[k].append(wall(f)[0])
    fmt = lambda v: "%9.2f [%9.2f .. %9.2f] ms" % (float(np.median(v)), min(v), max(v))
    print("DD-shaped, Nmax 1000: %d graphs (%d train / %d validation), hidden %d, K = 100, k = 3; median [min .. max] of %d alternating windows"
          % (n_graphs, len(train), len(val), h, REPS))
    label = {"a": "(d) evaluate, per-graph routes (a)", "b": "(d) evaluate, both flags off (b) "}
    for k in ("a", "b"):
        if k in routes:
            print("  %s: %s   (first call: %.1f ms)" % (label[k], fmt(times[k]), first[k]))
        else:
            print("  %s: not in this checkout" % label[k])
    if "a" in routes:
        print("      (a) faster than (b) in every window: %s   (ratio of medians %.2fx)"
              % (all(x < y for x, y in zip(times["a"], times["b"])), np.median(times["b"]) / np.median(times["a"])))
    top = "a" if "a" in routes else "b"
    sweep = {}
    for c in (32, 64, 128):
        f = _routed(top == "a", lambda: TS.embed_dataset(m, graphs, chunk=c))
        f()
        sweep[c] = [wall(f)[0] for _ in range(REPS)]
    print("  embed_dataset, route (%s), by graphs per chunk: %s" % (top, ", ".join("%d: %s" % (c, fmt(v)) for c, v in sweep.items())))
    if "a" in routes:
        ea = _routed(True, lambda: TS.embed_dataset(m, graphs))()
        eb = _routed(False, lambda: TS.embed_dataset(m, graphs))()
        print("  largest |route a - route b| embedding entry: %.3e (largest entry %.3e)" % (float((ea - eb).abs().max()), float(eb.abs().max())))
    for k in routes:
        print("  metrics, route (%s): %s" % (k, {kk: round(float(v), 4) for kk, v in res[k].items()}))
    sys.stdout.flush()


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "step":
        main_step([int(v) for v in sys.argv[2:]] or [64, 128])
    elif len(sys.argv) >= 2 and sys.argv[1] == "eval":
        main_eval(int(sys.argv[2]) if len(sys.argv) > 2 else 1168)
    else:
        main_all()
