#!/usr/bin/env python3
"""Golden vectors of hard / semi-hard negative mining (test infrastructure; never imported by the product path).

tests/golden/mining_dense.npz, mining_sag.npz — the reference's own ``TripletSampler.sampler(embed, hardness)`` (imported read-only at
run time from a checkout of the reference; none of its text is copied) drained three times under identical seeds of ``random`` and
``numpy.random``: with hardness 0, 0.5 and 1.  Hardness consumes no random numbers, so the first drain is the DRAWN schedule of the
other two (the script asserts that anchors and positives agree).  The files keep DATA only: the embeddings, the class lists as each
epoch's ``shuffle()`` left them, the drawn schedule and both mined schedules.

  dense   Code/sage+gat+diffpool/triplet_sampler.py over three classes of 5, 9 and 70 graphs: one epoch = 84 triplets; two epochs
  sag     Code/sag/triplet_sampler.py over two classes taken from ``.y`` (33 and 41 graphs).  Its epoch is TWO triplets (its
          ``attacker_list`` is [0, 1]), so the fixture concatenates 64 epochs, each with its own list order

Embeddings are multiples of 1/8 in [-4, 4], E = 24: every squared distance is exact in fp32 and fp64 in any summation order, and
distinct squared distances (multiples of 1/64 below 2^11) keep distinct fp32 square roots, so the reference's norm comparisons and
squared comparisons agree entry for entry.  Rows are drawn from a small pool of prototypes (shared across the classes), so several
graphs carry IDENTICAL rows and ties occur; the script prints how many entries rest on a tie rule and requires at least five of
each kind per fixture.

Usage:  python scripts/gen_golden_mining.py REFERENCE_ROOT
"""
import importlib.util
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mining_ref as MR  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden")
E = 24


def _load(root, sub):
    path = os.path.join(root, "Code", sub, "triplet_sampler.py")
    sys.dont_write_bytecode = True                             # (the checkout is read, never written)
    spec = importlib.util.spec_from_file_location("ref_sampler_" + sub.replace("+", "_"), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.TripletSampler


class Obj:
    """a graph as far as the samplers look: an identity, and ``.y`` for the SAGPool sampler"""

    def __init__(self, index, y):
        self.index, self.y = index, y


def embeddings(rng, sizes):
    """[sum(sizes), E] float32, multiples of 1/8 in [-4, 4]: every class draws its rows (with repetition) from 60% of its size in
    prototypes of its own plus six prototypes all classes share"""
    shared = np.clip(np.rint(8 * rng.normal(0.0, 1.0, size=(6, E))), -32, 32)
    rows = []
    for c, n in enumerate(sizes):
        own = np.clip(np.rint(8 * (rng.normal(0.0, 0.35, size=E) + rng.normal(0.0, 1.0, size=(max(2, (3 * n) // 5), E)))), -32, 32)
        pool = np.concatenate([own, shared])
        rows.append(pool[rng.integers(0, pool.shape[0], n)])
    return (np.concatenate(rows) / 8.0).astype(np.float32)


def drain(make, X, epochs, hardness, seed):
    """-> (schedule [T, 3], epoch_of [T], members [epochs, G]) of ``epochs`` epochs of a fresh sampler under the given seeds"""
    random.seed(seed)
    np.random.seed(seed)
    sampler, objs = make()
    where = {id(o): o.index for o in objs}
    rows, epoch_of, lists = [], [], []
    for ep in range(epochs):
        sampler.shuffle()
        keys = list(sampler.graphs.keys())
        lists.append(np.concatenate([[where[id(o)] for o in sampler.graphs[k]] for k in keys]))
        embed = {k: [X[where[id(o)]] for o in sampler.graphs[k]] for k in keys} if hardness > 0 else None
        while not sampler.end():
            s = sampler.sampler(embed, hardness)
            rows.append([where[id(s[k])] for k in ("anchor", "pos", "neg")])
            epoch_of.append(ep)
    return np.asarray(rows, dtype=np.int32), np.asarray(epoch_of, dtype=np.int32), np.asarray(lists, dtype=np.int32)


def fixture(name, Sampler, sizes, epochs, seed, by_y):
    rng = np.random.default_rng(seed)
    X = embeddings(rng, sizes)
    labels = np.repeat(np.arange(len(sizes)), sizes)

    def make():
        objs = [Obj(i, int(labels[i])) for i in range(labels.size)]
        if by_y:
            return Sampler(objs), objs
        return Sampler({"class%d" % c: [o for o in objs if o.y == c] for c in range(len(sizes))}), objs
    drawn, epoch_of, members = drain(make, X, epochs, 0, seed)
    semi, e1, m1 = drain(make, X, epochs, 0.5, seed)
    hard, e2, m2 = drain(make, X, epochs, 1, seed)
    assert np.array_equal(members, m1) and np.array_equal(members, m2) and np.array_equal(epoch_of, e1) and np.array_equal(epoch_of, e2)
    assert np.array_equal(drawn[:, :2], semi[:, :2]) and np.array_equal(drawn[:, :2], hard[:, :2]), "hardness moved anchors / positives"
    class_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    class_of = labels.astype(np.int32)
    ties_h = ties_s = 0
    for ep in range(epochs):
        sel = epoch_of == ep
        h, s = MR.tie_counts(X, drawn[sel], class_of, class_ptr, members[ep])
        ties_h, ties_s = ties_h + h, ties_s + s
        # the restatement on squared float64 distances gives what the reference's norms gave
        assert np.array_equal(MR.mine(X, drawn[sel], class_of, class_ptr, members[ep], MR.SEMI_HARD), semi[sel])
        assert np.array_equal(MR.mine(X, drawn[sel], class_of, class_ptr, members[ep], MR.HARDEST), hard[sel])
    print("%s: %d entries in %d epochs; changed: semi-hard %d, hardest %d; resting on a tie rule: hardest %d, semi-hard %d"
          % (name, drawn.shape[0], epochs, MR.changed(drawn, semi), MR.changed(drawn, hard), ties_h, ties_s))
    assert ties_h >= 5 and ties_s >= 5, "too few ties: pick another seed"
    assert np.array_equal(X * 8, np.rint(X * 8)) and np.abs(X).max() <= 4
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, emb=X, class_of=class_of, class_ptr=class_ptr, members=members, epoch_of=epoch_of, drawn=drawn,
                        semi=semi, hardest=hard, seed=seed, ties=np.array([ties_h, ties_s]))
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    fixture("mining_dense", _load(sys.argv[1], "sage+gat+diffpool"), [5, 9, 70], 2, 301, by_y=False)
    fixture("mining_sag", _load(sys.argv[1], "sag"), [33, 41], 64, 302, by_y=True)
