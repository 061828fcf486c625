#!/usr/bin/env python3
"""Hard / semi-hard negative mining, measured (mining.mine_negatives -> tsgnn_mine_negatives_f32, csrc/mine.hip).

DD-shaped: 1,051 graphs in two classes (612 / 439), a schedule of 1,051 triplets drained from a seeded TripletSampler-shaped object
(every graph the anchor once, the positive drawn from its class, the negative from the other), member lists in the sampler's shuffled
order.  ONE process, interleaved windows, median [min .. max]:

  1. the mine launch alone on standard-normal embeddings, E = 64, both modes: a burst of back-to-back launches between two device
     events (per launch), and the in-order time between two events around ONE launch
  2. host baselines on the same inputs, neither of which is the code under test, the device-to-host copy of the embeddings and the
     host-to-device copy of the mined column included: (v) tests/mining_ref.mine, one numpy expression per entry; (l) tests/mining_ref.
     mine_loop, one np.linalg.norm call per (anchor, candidate) pair as the reference's sampler spends them (fewer windows: seconds each)
     beside (d) the device path as a user calls it: mining.mine_negatives + a synchronise (host clock, like the baselines)
  3. the GraphSage stream (triplet_stream.TripletStream, GcnEncoderGraph 3 layers x 128 on 1,051 DD-shaped graphs, Nmax 1000): the
     epoch boundary embed_dataset + load + mine (host clock around work that ends in a synchronise) beside the epoch's 1,051 replays
     of one hipGraph (device events), and the replayed step with and without a mined schedule

    python scripts/mining_epoch.py [--no-stream]
"""
import os
import sys
import time

GRAPHS, SIZES, E, WINDOWS, LOOP_WINDOWS, BURST, SINGLES = 1051, (612, 439), 64, 5, 2, 200, 50
MARGIN = 1.0e6


class Sampler:
    """TripletSampler-shaped (shuffle / end / sampler, ``.graphs`` = {class: [objects]}), seeded"""

    def __init__(self, classes, seed):
        import numpy as np
        self.graphs, self.rng = classes, np.random.default_rng(seed)
        self.order, self.i = [], 0

    def shuffle(self):
        for k in self.graphs:
            self.rng.shuffle(self.graphs[k])
        self.order = [(k, j) for k in self.graphs for j in range(len(self.graphs[k]))]
        self.i = 0

    def end(self):
        return self.i >= len(self.order)

    def sampler(self):
        k, j = self.order[self.i]
        self.i += 1
        other = [c for c in self.graphs if c != k]
        kn = other[int(self.rng.integers(len(other)))]
        p = j
        while p == j:
            p = int(self.rng.integers(len(self.graphs[k])))
        return {"anchor": self.graphs[k][j], "pos": self.graphs[k][p], "neg": self.graphs[kn][int(self.rng.integers(len(self.graphs[kn])))]}


def main():
    import numpy as np
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    sys.path.insert(0, root)
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.join(root, "tests"))
    import mining_ref as MR
    from two_stage_gnn_amd import _native as nat, mining as M, triplet_stream as TS
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    dev = torch.device("cuda")
    fmt = lambda v, unit="us": "%9.1f [%9.1f .. %9.1f] %s" % (float(np.median(v)), min(v), max(v), unit)

    # ---- 1 + 2: the launch alone and the host baselines, on objects that stand for graphs
    objs = [object() for _ in range(GRAPHS)]
    label = np.repeat([0, 1], SIZES)
    sampler = Sampler({c: [o for o, y in zip(objs, label) if y == c] for c in (0, 1)}, seed=3)
    sched = TS.schedule_of(sampler, objs)
    index = M.class_index(sampler.graphs, objs)                # after the drain: the lists are in the epoch's order
    T = sched.shape[0]
    emb = torch.from_numpy(np.random.default_rng(4).standard_normal((GRAPHS, E)).astype(np.float32)).to(dev)
    drawn = torch.from_numpy(sched).to(dev)
    work = drawn.clone()
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def burst(h):
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(BURST):
            M.mine_negatives(emb, work, index, h)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / BURST * 1e3

    def single(h):
        out = []
        for _ in range(SINGLES):
            work.copy_(drawn)
            e0, e1 = ev(), ev()
            e0.record()
            M.mine_negatives(emb, work, index, h)
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(out))

    def device_path(h):
        work.copy_(drawn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M.mine_negatives(emb, work, index, h)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def host_path(fn, mode):
        work.copy_(drawn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = emb.cpu().numpy()                                  # the synchronising copy an epoch boundary would pay
        mined = fn(x, sched, index.class_of, index.class_ptr, index.members, mode)
        work[:, 2].copy_(torch.from_numpy(mined[:, 2].astype(np.int32)))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, mined

    nat.trace = []
    M.mine_negatives(emb, work, index, 1)
    kname = nat.trace[0][2]
    nat.trace = None
    res = {}
    for h, mode, name in ((0.5, MR.SEMI_HARD, "semi-hard"), (1, MR.HARDEST, "hardest")):
        burst(h); single(h); device_path(h)                     # warm-up
        r = res[name] = {"burst": [], "single": [], "dev": [], "vec": [], "loop": []}
        for w in range(WINDOWS):
            work.copy_(drawn)
            r["burst"].append(burst(h))
            r["single"].append(single(h))
            r["dev"].append(device_path(h))
            got = work.cpu().numpy()
            tv, mined = host_path(MR.mine, mode)
            r["vec"].append(tv)
            if w < LOOP_WINDOWS:
                r["loop"].append(host_path(MR.mine_loop, mode)[0])
            r["differ"] = MR.changed(mined, got)
            r["changed"] = MR.changed(sched, got)
    print("mining on %d graphs in two classes (%d / %d), E = %d, schedule of %d seeded triplets; kernel %s; median [min .. max] of %d interleaved windows"
          % (GRAPHS, SIZES[0], SIZES[1], E, T, kname.split("<")[0], WINDOWS))
    for name, r in res.items():
        print("  %s: %d of %d negatives changed; %d entries differ from the float64 host result" % (name, r["changed"], T, r["differ"]))
        print("    mine launch alone, burst of %d back-to-back launches   : %s per launch" % (BURST, fmt(r["burst"])))
        print("    mine launch alone, in order between two events (median of %d per window): %s" % (SINGLES, fmt(r["single"])))
        print("    (d) device path, mine_negatives + synchronise, host clock : %s" % fmt(r["dev"]))
        print("    (v) host, vectorised numpy per entry, copies included     : %s" % fmt(r["vec"]))
        print("    (l) host, one norm call per pair, copies included (%d windows): %s" % (LOOP_WINDOWS, fmt(r["loop"])))
        print("        (d) faster than (v) in every window: %s   (v) / (d) = %.0fx   (l) / (d) = %.0fx"
              % (all(a < b for a, b in zip(r["dev"], r["vec"])), np.median(r["vec"]) / np.median(r["dev"]), np.median(r["loop"]) / np.median(r["dev"])))
    sys.stdout.flush()
    if "--no-stream" in sys.argv:
        return

    # ---- 3: the epoch boundary beside the epoch, GraphSage stream
    from two_stage_eval import dense_dataset
    from two_stage_gnn_amd import dense_encoders as En, triplet, two_stage
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    pool, fin = dense_dataset(GRAPHS)
    classes = {}
    for o in pool:
        classes.setdefault(o.graph["label"], []).append(o)
    sampler = Sampler(classes, seed=5)

    class A:
        bias = True
    torch.manual_seed(5)
    m = En.GcnEncoderGraph(fin, 128, 128, 2, 3, bn=True, args=A(), final_dim="output_dim").to(dev).train()
    net = triplet.tripletnet(m)
    st = triplet.TripletStream(net, pool, max_steps=GRAPHS)
    tgt = torch.full((1,), -1.0, device=dev)
    gs = GraphedStep(FlatTrainer(m, lr=1e-3, clip=2.0), st.loss(triplet.MarginRankingLoss(margin=MARGIN), tgt), warmup=3)

    def epoch():
        e0, e1 = ev(), ev()
        e0.record(gs.stream)
        for _ in range(len(st)):
            gs.step()
        e1.record(gs.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    rows = {k: [] for k in ("sched", "embed", "load", "mine", "epoch_mined", "epoch_drawn")}
    changed = []
    for w in range(WINDOWS + 1):                                # (window 0: warm-up, dropped)
        for h in (1, 0):                                       # a mined epoch and a drawn one, alternately
            t_s, s = timed(lambda: TS.schedule_of(sampler, pool))
            idx = M.class_index(sampler.graphs, pool)
            t_e, x = timed(lambda: two_stage.embed_dataset(net, pool))
            t_l, _ = timed(lambda: st.load(s))
            t_m, c = timed(lambda: st.mine(x, idx, h, count=True))
            t_ep = epoch()
            if w:
                if h:
                    rows["sched"].append(t_s); rows["embed"].append(t_e); rows["load"].append(t_l); rows["mine"].append(t_m)
                    rows["epoch_mined"].append(t_ep); changed.append(int(c))
                else:
                    rows["epoch_drawn"].append(t_ep)
    T2 = len(st)
    print("GraphSage stream, %d DD-shaped graphs (classes %s), Nmax %d, 3 layers x 128, embeddings [%d, %d]; an epoch = %d replays of one hipGraph; %d windows"
          % (GRAPHS, "/".join(str(len(v)) for v in classes.values()), st.arena.nmax, x.shape[0], x.shape[1], T2, WINDOWS))
    print("  epoch boundary (host clock, each ends in a synchronise), hardest:")
    print("    schedule_of (host, the sampler's draws)   : %s" % fmt(rows["sched"], "ms"))
    print("    embed_dataset                            : %s" % fmt(rows["embed"], "ms"))
    print("    load                                     : %s" % fmt(rows["load"], "ms"))
    print("    mine (two synchronises + the launch)     : %s   negatives changed per epoch: %s" % (fmt(rows["mine"], "ms"), changed))
    print("  the epoch's %d replays, mined schedule      : %s  = %.1f us per step" % (T2, fmt(rows["epoch_mined"], "ms"), np.median(rows["epoch_mined"]) / T2 * 1e3))
    print("  the epoch's %d replays, drawn schedule      : %s  = %.1f us per step" % (T2, fmt(rows["epoch_drawn"], "ms"), np.median(rows["epoch_drawn"]) / T2 * 1e3))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
