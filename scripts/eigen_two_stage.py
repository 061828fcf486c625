#!/usr/bin/env python3
"""EigenGCN's stage two measured (Code/eigengcn/train_triplet.py:30-268, run after every epoch at :326-354): ``two_stage.evaluate`` /
``evaluate_mlp`` on chunks assembled by csrc/eigen_assemble.hip, against what this code base could do without it, in ONE process.

Workload: 1,168 DD-shaped synthetic graphs (1,051 train / 117 validation; scripts/eigen_step.py's generator and chunked clusters), Nmax
1000, 89 features, WavePoolingGcnEncoder 3 layers h128, pool_sizes '10', J = 2, Jf = 1, con_final 1, pred_hidden_dims [50], label_dim 64.

    python scripts/eigen_two_stage.py [N] [--out FILE]      N graphs (default 1168); the report goes to FILE (default
                                                            profiles/r10/eigen_two_stage.txt) and to stdout

Rows (every comparison in alternating windows, median [min .. max] of REPS):
  sweep       ``embed_dataset`` at 32 / 64 / 128 / 256 graphs per chunk (device events)
  evaluate    end to end at the default chunk (host clock around a call that ends in a synchronise), against
              (a) the plain loop of B = 1 forwards on PREBUILT one-graph EigenBatches + the same HIP k-NN — the best the code base
                  could do before: no route of ``embed_dataset`` took this family
  evaluate_mlp end to end, chunked and on (a)'s embeddings
  assembler   one pass over all chunks of the default size, nothing else: the kernel against
              (b) ``eigen_pool.concat_batches`` + ``torch.cat`` of the same resident one-graph batches (host clock ending in a
                  synchronise: the cost is host work and launches; device events beside it); and ``embed_dataset`` with (b) inside
Results of the chunked way and of (a) are compared (largest difference of an embedding entry, both metric dictionaries).

A ``.graph`` dict of this size holds five dense [1000, 1000] arrays, 20 MB in float32, 23 GB for the dataset: every graph object gets
its dict, is made resident from it (``eigen_triplet.resident_graph``: packed on the host, one upload; timed) and then keeps only the
label.  That is this script saving host memory, not a property of the interface: objects are otherwise taken to be immutable."""
import os
import sys
import time

REPS = 5
NMAX, J, JF, LABEL_DIM = 1000, 2, 1, 64
CHUNKS = (32, 64, 128, 256)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Graph:
    pass


def dataset(n_graphs, dev, cache):
    """graph objects, resident; -> (objects, labels, feature width, seconds of host packing + upload per graph)"""
    import numpy as np
    import eigen_step
    from two_stage_gnn_amd import eigen_pool as ep, eigen_triplet as ET
    results, xp, labels = eigen_step.batch(7, B=n_graphs, nmax=NMAX)
    objs, spent = [], 0.0
    f32 = lambda t: np.ascontiguousarray(t[0].numpy().astype(np.float32))
    for b, r in enumerate(results):
        adj, pooled, n0, nl, pm = ep.dense_inputs([r], NMAX, J, JF)
        n = int(n0[0])
        feats = xp[b].copy()
        feats[:n] += 0.25 * float(labels[b])                 # (a class signal, so that the classifiers have something to find)
        g = Graph()
        g.graph = {"adj": f32(adj), "feats": feats, "num_nodes": n, "adj_pool_1": f32(pooled[0]), "num_nodes_1": int(nl[0][0]),
                   "label": int(labels[b])}
        for j in range(J):
            g.graph["pool_adj_0_%d" % j] = f32(pm[0][j])
        for j in range(JF):
            g.graph["pool_adj_1_%d" % j] = f32(pm[1][j])
        t0 = time.perf_counter()
        ET.resident_graph(g, dev, cache, 1, J, JF, check=True)
        spent += time.perf_counter() - t0
        g.graph = {"label": int(labels[b])}
        objs.append(g)
    return objs, np.asarray(labels[:n_graphs]), int(xp.shape[2]), spent / max(n_graphs, 1)


def main(n_graphs, out_path):
    import types
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from two_stage_gnn_amd import eigen_encoders as EE, eigen_pool as ep, eigen_triplet as ET, resident as R, two_stage as TS
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    args = types.SimpleNamespace(bias=True, con_final=1, pool_sizes="10", num_pool_matrix=J, num_pool_final_matrix=JF)
    torch.manual_seed(5)
    fin = 89
    model = EE.WavePoolingGcnEncoder(NMAX, fin, 128, 128, LABEL_DIM, 3, num_pool_matrix=J, num_pool_final_matrix=JF, pool_sizes=[10],
                                     pred_hidden_dims=[50], args=args)
    net = ET.tripletnet(model, args)
    cache = R.resident_cache(model)
    graphs, y, fin_data, t_resident = dataset(n_graphs, dev, cache)
    assert fin_data == fin
    n_val = max(1, int(round(0.1 * n_graphs)))
    train, val = graphs[:n_graphs - n_val], graphs[n_graphs - n_val:]
    y_tr, y_va = y[:n_graphs - n_val], y[n_graphs - n_val:]
    parts = [cache.lookup(g, dev.index) for g in graphs]
    singles = [(torch.cat([p.feats, R.ghost_zeros(NMAX, p.ldf, dev)]), p.eb) for p in parts]     # (a)'s prebuilt one-graph batches

    def sync_wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def events(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def windows(rows, timer):
        """every row once as warm-up, then REPS alternating windows -> {name: [ms]}, {name: last result}"""
        last = {}
        for k, f in rows.items():
            last[k] = f()
        times = {k: [] for k in rows}
        for _ in range(REPS):
            for k, f in rows.items():
                t, last[k] = timer(f)
                times[k].append(t)
        return times, last

    fmt = lambda v: "%9.2f [%9.2f .. %9.2f] ms" % (float(np.median(v)), min(v), max(v))
    med = lambda v: float(np.median(v))
    lines = []

    def say(s=""):
        print(s)
        sys.stdout.flush()
        lines.append(s)

    say("EigenGCN stage two: %d DD-shaped graphs (%d train / %d validation, %d..%d nodes), Nmax %d, %d features, 3 layers h128, "
        "pool_sizes '10', J %d, Jf %d, con_final 1, pred_hidden_dims [50], label_dim %d; median [min .. max] of %d alternating windows"
        % (n_graphs, len(train), len(val), min(p.n for p in parts), max(p.n for p in parts), NMAX, fin, J, JF, LABEL_DIM, REPS))
    say("  making a graph resident (pack_host on the dict + the piece's one upload): %.1f ms per graph, once" % (t_resident * 1e3))

    # ---- the sweep
    rows = {c: (lambda c=c: TS.embed_dataset(net, graphs, c)) for c in CHUNKS}
    sweep, _ = windows(rows, events)
    say("  embed_dataset by graphs per chunk (device events):")
    for c in CHUNKS:
        say("    %4d: %s" % (c, fmt(sweep[c])))
    best = min(CHUNKS, key=lambda c: med(sweep[c]))
    chunk = ET.DEFAULT_CHUNK
    say("    fastest: %d graphs per chunk (%.2f ms); this tree's eigen_triplet.DEFAULT_CHUNK = %d, used by the rows below" % (best, med(sweep[best]), chunk))
    say("    launch shape: the pieces' records by value, ceil(B / 32) launches per chunk.  One launch per chunk reading the records from a "
        "description table staged through pinned memory was measured beside it before it was removed "
        "(profiles/r10/eigen_two_stage_launch_shapes.txt): neither shape won, and this one uploads nothing")

    # ---- evaluate / evaluate_mlp end to end against (a)
    def loop_embed():
        model.eval()
        with R.per_graph_statistics(model), torch.no_grad():
            return torch.cat([model.pred_model(model(x, eb, readout_only=True)) for x, eb in singles])

    def evaluate_a():
        emb = TS._rows16(loop_embed())
        conf, _ = TS.knn_confusions(emb[:len(train)], y_tr, emb[len(train):], y_va, 3)
        res = TS.metrics_from_confusion(conf[0])
        res["train acc"] = int(np.trace(conf[1])) / max(int(conf[1].sum()), 1)
        return res

    def mlp_a():
        emb = TS._rows16(loop_embed())
        torch.manual_seed(9)
        return {"acc": TS.MLPProbe().fit(emb[:len(train)], y_tr).score(emb[len(train):], y_va)}

    def mlp_chunked():
        torch.manual_seed(9)
        return TS.evaluate_mlp(train, val, net, chunk=chunk)
    ev, res = windows({"chunked": lambda: TS.evaluate(train, val, net, chunk=chunk), "a": evaluate_a}, sync_wall)
    say("  evaluate, end to end (host clock, synchronised), %d graphs per chunk:" % chunk)
    say("    two_stage.evaluate, chunks assembled by the kernel            : %s" % fmt(ev["chunked"]))
    say("    (a) loop of B = 1 forwards on prebuilt EigenBatches + HIP k-NN : %s" % fmt(ev["a"]))
    say("    chunked faster in every window: %s   (ratio of medians %.1fx)"
        % (all(c < a for c, a in zip(ev["chunked"], ev["a"])), med(ev["a"]) / med(ev["chunked"])))
    say("    metrics, chunked: %s" % {k: round(v, 4) for k, v in res["chunked"].items()})
    say("    metrics, (a)    : %s" % {k: round(v, 4) for k, v in res["a"].items()})
    diff = float((TS.embed_dataset(net, graphs, chunk) - loop_embed()).abs().max())
    say("    largest difference of an embedding entry, chunked vs (a): %.3e (largest entry %.3e)" % (diff, float(loop_embed().abs().max())))
    mv, mres = windows({"chunked": mlp_chunked, "a": mlp_a}, sync_wall)
    say("  evaluate_mlp, end to end: chunked %s   on (a)'s embeddings %s   (ratio of medians %.1fx); acc %s / %s"
        % (fmt(mv["chunked"]), fmt(mv["a"]), med(mv["a"]) / med(mv["chunked"]), mres["chunked"], mres["a"]))

    # ---- the assembler alone, and embed_dataset with concat_batches inside: (b)
    groups = [parts[i:i + chunk] for i in range(0, len(parts), chunk)]

    def concat_chunk(grp):
        return torch.cat([q.feats for q in grp] + [R.ghost_zeros(NMAX, grp[0].ldf, dev)]), ep.concat_batches([q.eb for q in grp])

    def embed_b():
        model.eval()
        out = []
        with R.per_graph_statistics(model), torch.no_grad():
            for grp in groups:
                x, eb = concat_chunk(grp)
                out.append(model.pred_model(model(x, eb, readout_only=True)))
        return torch.cat(out)
    asm = {"kernel": lambda: [ET.assemble(g, dev) for g in groups], "b": lambda: [concat_chunk(g) for g in groups]}
    aw, _ = windows(asm, sync_wall)
    ae, _ = windows(asm, events)
    say("  assembling all %d chunks of %d graphs, nothing else (host clock, synchronised | device events):" % (len(groups), chunk))
    say("    kernel (csrc/eigen_assemble.hip)               : %s | %s" % (fmt(aw["kernel"]), fmt(ae["kernel"])))
    say("    (b) eigen_pool.concat_batches + torch.cat      : %s | %s" % (fmt(aw["b"]), fmt(ae["b"])))
    kern = "kernel"
    say("    kernel faster than (b) in every window: %s   (ratio of medians %.1fx)"
        % (all(k < b for k, b in zip(aw[kern], aw["b"])), med(aw["b"]) / med(aw[kern])))
    eb_t, _ = windows({"kernel": lambda: TS.embed_dataset(net, graphs, chunk), "b": embed_b}, sync_wall)
    say("  embed_dataset (host clock, synchronised): kernel-assembled chunks %s   (b) inside %s   (ratio of medians %.1fx)"
        % (fmt(eb_t["kernel"]), fmt(eb_t["b"]), med(eb_t["b"]) / med(eb_t["kernel"])))
    say("  verdicts: chunked evaluate beats (a): %s; the kernel assembler beats (b) at %d graphs per chunk: %s"
        % (med(ev["chunked"]) < med(ev["a"]), chunk, med(aw[kern]) < med(aw["b"])))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r10", "eigen_two_stage.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    main(int(argv[0]) if argv else 1168, out)
