#!/usr/bin/env python3
"""The SAGPool mini-batch stream, measured (Code/sag/train.py:181-198: ONE new mini-batch of 128 graphs per optimiser step): 1,000
IMDB-B-shaped and 512 DD-shaped synthetic graphs, sag_layers.Net(use_batch=True) nhid 128, ratio 0.5, 2 classes, dropout 0.5,
F.nll_loss + Adam (lr 5e-4, weight decay 1e-4, no clipping) under FlatTrainer + GraphedStep, a seeded schedule of 2,000 entries of
distinct graphs.  Per shape four step figures in ONE process, five alternating windows each:

  (a) streamed: sag_stream.MiniBatchStream at its default capacity (the 128 largest graphs, level by level)
  (b) streamed at sag_stream.schedule_capacity (the schedule's own maxima)
  (c) the schedule's mean-size entry as an exact resident batch replayed from one hipGraph (BASELINE config 4's step)
  (d) the eager loop: a host collate of the same objects in the same order, .to(device), Net(use_batch=True), nll_loss, FlatTrainer.step
      (a window = 40 entries)

plus the gather launch alone between two events.

    python scripts/sag_minibatch_step.py               both shapes, each in a child process under its own time limit
    python scripts/sag_minibatch_step.py DD            one shape in this process

Replayed rows: device events around the window's replays; the eager row: host clock around steps that end in a synchronise.
Reported: median [min .. max] over the windows."""
import os
import subprocess
import sys
import time

SHAPES = {"IMDB-BINARY": (1000, 136), "DD": (512, 1000)}      # shape: (graphs, Nmax of the generator)
BATCH, STEPS, REPS, EAGER_STEPS, SINGLE = 128, 2000, 5, 40, 50
LIMIT_S = 280


def main_all():
    for shape in SHAPES:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), shape])
        if r.returncode != 0:                                # (a fault or a time-out: nothing more is started on the device)
            print("shape %s ended with status %d: stopping" % (shape, r.returncode))
            sys.exit(r.returncode)


def main_one(shape):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from two_stage_gnn_amd import message_passing as mp, sag_layers as S, sag_stream as SS, sag_triplet as ST, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    dev = torch.device("cuda")
    per = STEPS // REPS
    GRAPHS, nmax = SHAPES[shape]

    class Data:
        pass

    hb = synthetic.host_batch(7, GRAPHS, shape, nmax)
    sizes = hb["sizes"]
    gp = np.concatenate([[0], np.cumsum(sizes)])
    rp, col, fin = hb["rowptr"], hb["col"], int(hb["x"].shape[1])
    labels = np.random.default_rng(3).integers(0, 2, GRAPHS)
    pool, host = [], []
    for b in range(GRAPHS):
        lo, hi = int(gp[b]), int(gp[b + 1])
        c = col[rp[lo]:rp[hi]].astype(np.int64) - lo
        t = np.repeat(np.arange(hi - lo), np.diff(rp[lo:hi + 1]))
        h = Data()                                           # what a DataLoader collates: host tensors
        h.x = torch.from_numpy(np.ascontiguousarray(hb["x"][lo:hi])).float()
        h.edge_index = torch.from_numpy(np.stack([c, t.astype(np.int64)]))
        h.y = torch.tensor([int(labels[b])])
        d = Data()
        d.x, d.edge_index, d.y = h.x.to(dev), h.edge_index.to(dev), h.y
        pool.append(d); host.append(h)
    rng = np.random.default_rng(1)
    sched = np.stack([rng.choice(GRAPHS, size=BATCH, replace=False) for _ in range(STEPS)]).astype(np.int64)
    rows = sizes[sched].sum(1)

    def make():
        torch.manual_seed(5)
        net = S.Net(fin, 128, 2, 0.5, 0.5, use_batch=True, conv="gcn").to(dev).train()
        return net, FlatTrainer(net, lr=5e-4, weight_decay=1e-4, clip=0)

    # (a), (b)
    m_a, tr_a = make()
    t0 = time.perf_counter()
    st_a = SS.MiniBatchStream(m_a, pool, BATCH, max_steps=STEPS)
    t_pack = time.perf_counter() - t0
    gs_a = GraphedStep(tr_a, st_a.loss(), warmup=3)
    m_b, tr_b = make()
    own = SS.schedule_capacity(st_a.arena.records, sched, 0.5)
    st_b = SS.MiniBatchStream(m_b, pool, BATCH, max_steps=STEPS, **own)
    gs_b = GraphedStep(tr_b, st_b.loss(), warmup=3)
    assert st_a.fits(sched).all() and st_b.fits(sched).all()
    # (c)
    m_c, tr_c = make()
    k_mean = int(np.argmin(np.abs(rows - rows.mean())))
    net_c = ST.tripletnet(m_c)
    batch_c = net_c.batch_of([pool[i] for i in sched[k_mean]])
    y_c = torch.from_numpy(labels[sched[k_mean]].astype(np.int64)).to(dev)
    gs_c = GraphedStep(tr_c, lambda: mp.nll_loss(mp.mlp3_log_softmax(net_c.readout(batch_c), m_c.lin1, m_c.lin2, m_c.lin3, 0.5, True), y_c),
                       warmup=3)
    # (d)
    m_d, tr_d = make()

    def collate(ids):
        b, off, eis, bv = Data(), 0, [], []
        for k, i in enumerate(ids):
            h = host[i]
            eis.append(h.edge_index + off)
            bv.append(torch.full((h.x.size(0),), k, dtype=torch.long))
            off += int(h.x.size(0))
        b.x = torch.cat([host[i].x for i in ids]).to(dev)
        b.edge_index, b.batch = torch.cat(eis, dim=1).to(dev), torch.cat(bv).to(dev)
        b.y = torch.cat([host[i].y for i in ids]).to(dev)
        return b

    def eager_step(ids):
        b = collate(ids)
        tr_d.step(lambda: mp.nll_loss(m_d(b), b.y))

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
            eager_step(ids)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / EAGER_STEPS * 1e6

    st_a.load(sched); st_b.load(sched)
    replayed(gs_a, 50); replayed(gs_b, 50); replayed(gs_c, 50)   # warm-up of every row
    for ids in sched[:5]:
        eager_step(ids)
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

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    single = {"a": [], "b": []}
    for key, st in (("a", st_a), ("b", st_b)):
        for _ in range(SINGLE):
            e0.record(); st.gather(); e1.record(); e1.synchronize()
            single[key].append(e0.elapsed_time(e1) * 1e3)

    fmt = lambda v, unit="us/step": "%8.1f [%8.1f .. %8.1f] %s" % (float(np.median(v)), min(v), max(v), unit)
    med = {k: float(np.median(v)) for k, v in times.items()}
    ratio = lambda p, q: "%.3f [%.3f .. %.3f]" % (med[p] / med[q], min(x / y for x, y in zip(times[p], times[q])),
                                                  max(x / y for x, y in zip(times[p], times[q])))
    ar = st_a.arena
    print("%s-shaped: %d graphs (%d..%d nodes, mean %.0f), %d features; sag_layers.Net(use_batch=True) conv=gcn, nhid 128, ratio 0.5, 2 classes, "
          "dropout 0.5; B %d; nll + Adam (lr 5e-4, weight decay 1e-4, no clipping) under FlatTrainer; schedule of %d seeded entries of distinct "
          "graphs (rows %d..%d, mean %.0f); median [min .. max] of %d alternating windows of %d steps"
          % (shape, GRAPHS, sizes.min(), sizes.max(), sizes.mean(), fin, BATCH, STEPS, rows.min(), rows.max(), rows.mean(), REPS, per))
    print("  arena: %.1f MB, packed + uploaded in %.2f s" % ((ar.buf.nbytes + ar.feats.nbytes + ar.records.nbytes) / 1e6, t_pack))
    for key, st, what in (("a", st_a, "default capacity   "), ("b", st_b, "schedule_capacity  ")):
        print("  (%s) streamed, %s (rows per level %s, %d entries): %s   %.0f graphs/s"
              % (key, what, "/".join(str(L.N) for L in st.plan.levels), st.nnz_cap, fmt(times[key]), BATCH / med[key] * 1e6))
    print("  (c) the mean-size entry (%d rows) as an exact resident batch, one hipGraph : %s   %.0f graphs/s"
          % (int(rows[k_mean]), fmt(times["c"]), BATCH / med["c"] * 1e6))
    print("  (d) eager: host collate + Net(use_batch=True), same objects, same order    : %s   %.0f graphs/s"
          % (fmt(times["d"]), BATCH / med["d"] * 1e6))
    print("      time (b) / time (c) = %s   time (a) / time (b) = %s   (median; range of the per-window ratios)" % (ratio("b", "c"), ratio("a", "b")))
    print("      time (d) / time (b) = %s   (b) faster than (d) in every window: %s   (a) faster than (d) in every window: %s"
          % (ratio("d", "b"), all(x < y for x, y in zip(times["b"], times["d"])), all(x < y for x, y in zip(times["a"], times["d"]))))
    for key, st in (("a", st_a), ("b", st_b)):
        print("  gather launch alone at (%s)'s capacity, %d workgroups: between two events %s"
              % (key, -(-st.row_cap // 32), fmt(single[key], "us")))
    print("      cursors after the windows: %s; loss of each window's last step: (a) %s  (b) %s"
          % (pos, " ".join("%.4f" % v for v in losses["a"]), " ".join("%.4f" % v for v in losses["b"])))
    sys.stdout.flush()


if __name__ == "__main__":
    if len(sys.argv) >= 2:
        main_one(sys.argv[1])
    else:
        main_all()
