#!/usr/bin/env python3
"""The fine-tuning step of 2stg+ for the SAGPool family, measured (Code/sag/train_triplet_pre_train.py:219-263: ONE graph per
optimiser step on F.nll_loss(model(data), data.y)): 256 IMDB-B-shaped and 256 DD-shaped synthetic labelled graphs, sag_layers.Net
nhid 128, ratio 0.5, final_dim 64 (= num_classes), dropout 0.5 active, Adam at lr 1e-3 without clipping under a new
FlatTrainer(clip=0), a seeded schedule of 2,000 anchors.  Three figures per shape in ONE process, five alternating windows each:

  (a) streamed: sag_stream.PostTrainStream, a NEW anchor per replay of one hipGraph (a window = 400 consecutive schedule entries)
  (b) the eager sag_stream.post_train_step on the resident structure, fed the same objects in the same order (a window = 40 entries)
  (c) the plain module call: mp.nll_loss(model(data), data.y), same objects and order

plus the device kernels of one streamed step.  ``measure3`` is shared with scripts/eigen_posttrain_step.py.

    python scripts/sag_posttrain_step.py [OUTPUT_FILE]       (appends to OUTPUT_FILE; one child process per shape, each under its own
                                                              time limit: after a fault or a time-out nothing more is started)

Replayed row: device events around the window's replays; the eager rows: host clock around steps that end in a synchronise.
Reported: median [min .. max] over the windows."""
import os
import subprocess
import sys
import time

GRAPHS, STEPS, REPS, EAGER_STEPS = 256, 2000, 5, 40
SHAPES = ("IMDB-BINARY", "DD")
LIMIT_S = 280


def measure3(title, pool, anchors, make, stream_of, eager_step, plain_step, out_path, note=""):
    """``make()`` -> (model, FlatTrainer); ``stream_of(model)`` -> a PostTrainStream; ``eager_step(model, obj)`` / ``plain_step(model, obj)``
    -> the loss of rows (b) / (c).  Prints the rows and appends them to ``out_path``"""
    import numpy as np
    import torch
    from collections import Counter
    from torch.profiler import profile, ProfilerActivity
    from two_stage_gnn_amd.data_parallel import GraphedStep
    per = STEPS // REPS
    m_a, tr_a = make()
    t0 = time.perf_counter()
    st = stream_of(m_a)
    t_pack = time.perf_counter() - t0
    gs_a = GraphedStep(tr_a, st.step_loss(), warmup=3)
    m_b, tr_b = make()
    m_c, tr_c = make()

    def replayed(gs, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(gs.stream)
        for _ in range(n):
            gs.step()
        e1.record(gs.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    def eager(tr, m, step, w):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in anchors[w * per:w * per + EAGER_STEPS]:
            tr.step(lambda: step(m, pool[i]))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / EAGER_STEPS * 1e6

    st.load(anchors)
    replayed(gs_a, 50)                                       # warm-up of every row (the eager rows: every window's objects once)
    for w in range(REPS):
        eager(tr_b, m_b, eager_step, w); eager(tr_c, m_c, plain_step, w)
    st.load(anchors)                                         # the epoch starts here: window w replays entries [w * per, (w + 1) * per)
    times = {"a": [], "b": [], "c": []}
    losses = []
    for w in range(REPS):
        times["a"].append(replayed(gs_a, per))
        times["b"].append(eager(tr_b, m_b, eager_step, w))
        times["c"].append(eager(tr_c, m_c, plain_step, w))
        losses.append(gs_a.loss_value())
    pos = st.position()
    best = []
    for _ in range(3):                                       # (the profiler's first cycles in a process may drop events: keep the fullest)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs_a.step()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type.name == "CUDA"]
        best = ev if len(ev) > len(best) else best

    def short(n):
        n = n.replace("void ", "").replace("(anonymous namespace)::", "").replace("at::native::", "")
        return n.split("(")[0].split("<")[0][:40] or n[:40]
    us = Counter()
    for e in best:
        us[short(e.name)] += e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
    fmt = lambda v: "%8.1f [%8.1f .. %8.1f] us/step" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = ["%s; schedule of %d seeded anchors; median [min .. max] of %d alternating windows" % (title, STEPS, REPS)]
    lines.append("  arena packed + uploaded in %.2f s%s" % (t_pack, note and "; " + note))
    lines.append("  (a) streamed, a new anchor per replay, one hipGraph        : %s   %d device kernels, %s; cursor after the windows: %d"
                 % (fmt(times["a"]), len(best), gs_a.describe(), pos))
    lines.append("  (b) eager post_train_step, same objects in the same order  : %s" % fmt(times["b"]))
    lines.append("  (c) the plain module call + the library's loss             : %s" % fmt(times["c"]))
    lines.append("      (a) faster than (b) in every window: %s   time (b) / time (a) = %.2fx;   (a) faster than (c) in every window: %s   time (c) / "
                 "time (a) = %.2fx" % (all(x < y for x, y in zip(times["a"], times["b"])), med["b"] / med["a"],
                                      all(x < y for x, y in zip(times["a"], times["c"])), med["c"] / med["a"]))
    lines.append("      (a) kernels: " + ", ".join("%s x%d" % kv for kv in Counter(short(e.name) for e in best).most_common(40)))
    lines.append("      (a) device us of one step, largest first: " + ", ".join("%s %.1f" % kv for kv in us.most_common(12)))
    lines.append("      loss of each window's last streamed step: " + " ".join("%.4f" % v for v in losses))
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")
    sys.stdout.flush()
    return med


def main_all(out_path):
    for shape in SHAPES:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--shape", shape] +
                           ([out_path] if out_path else []))
        if r.returncode != 0:                                # (a fault or a time-out: nothing more is started on the device)
            print("shape %s ended with status %d: stopping" % (shape, r.returncode))
            sys.exit(r.returncode)


def main_one(shape, out_path):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from two_stage_gnn_amd import message_passing as mp, sag_layers as S, sag_stream, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    dev = torch.device("cuda")

    class Data:
        pass

    hb = synthetic.host_batch(7, GRAPHS, shape, 1000 if shape == "DD" else 136)
    sizes = hb["sizes"]
    gp = np.concatenate([[0], np.cumsum(sizes)])
    rp, col, fin = hb["rowptr"], hb["col"], int(hb["x"].shape[1])
    labels = np.random.default_rng(3).integers(0, 64, size=GRAPHS)
    pool = []
    for b in range(GRAPHS):
        lo, hi = int(gp[b]), int(gp[b + 1])
        c = col[rp[lo]:rp[hi]].astype(np.int64) - lo
        t = np.repeat(np.arange(hi - lo), np.diff(rp[lo:hi + 1]))
        d = Data()
        d.x = torch.from_numpy(np.ascontiguousarray(hb["x"][lo:hi])).float().to(dev)
        d.edge_index = torch.from_numpy(np.stack([c, t.astype(np.int64)])).to(dev)
        d.y = torch.tensor([int(labels[b])], device=dev)
        pool.append(d)
    anchors = np.random.default_rng(1).integers(0, GRAPHS, size=STEPS)

    def make():
        torch.manual_seed(5)
        net = S.Net(fin, 128, 64, 0.5, 0.5, conv="gcn").to(dev).train()
        return net, FlatTrainer(net, lr=1e-3, clip=0)

    measure3("%s-shaped: %d labelled graphs (%d..%d nodes, mean %.0f), %d features; sag_layers.Net conv=gcn, nhid 128, ratio 0.5, final_dim 64, "
             "dropout 0.5 active; nll over 64 columns, Adam lr 1e-3, no clipping"
             % (shape, GRAPHS, sizes.min(), sizes.max(), sizes.mean(), fin), pool, anchors, make,
             lambda m: sag_stream.PostTrainStream(m, pool, max_steps=STEPS), lambda m, d: sag_stream.post_train_step(m, d)[0],
             lambda m, d: mp.nll_loss(m(d), d.y), out_path,
             note="the three-graph triplet step of profiles/r16/sag_stream.txt: %s us/step" % ("151" if shape == "IMDB-BINARY" else "251"))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--shape"]:
        main_one(args[1], args[2] if len(args) > 2 else None)
    else:
        main_all(args[0] if args else None)
