"""The integer-valued synthetic cases the mining tests share (tests/test_mining_host.py checks that they contain what they claim,
tests/test_gpu_mining.py runs the kernel on them).  Every squared distance is an integer far below 2^24, so fp32 in any summation
order, float64 and int64 agree exactly and the kernel must equal ``mining_ref.mine_int`` entry for entry.

A case = (dim, class sizes, T, kind).  The grid covers dim in {1, 3, 4, 5, 64, 130, 1024} (below / at / above a 16-byte column
group, two and a half LDS passes of nothing special, the widest row), class sizes in {1, 2, 63, 64, 65, 129} (below / at / above one
stride of 64 lanes, two strides and one), two and three classes, T in {1, 3, 4, 5, 257} (below / at / above one workgroup of four
entries, many workgroups with a ragged last one).  Every class's member list is a permutation that differs from index order
(classes of one graph excepted).

kind "random": rows of small integers in [-2, 2] — distances collide all the time, so ties of every sort occur by themselves.
kind "crafted": all rows share a random integer offset (it cancels in difference form only) and differ in the LAST column alone,
where the candidates of the last class sit at x = 100 except four "special" ones at x = 0, 10, 20, 30 placed at list positions
0, 63, 64 and last.  The first entries of the schedule are then, in this order:
  0..3  anchor at x = 0 / 10 / 20 / 30 (EQUAL to the special candidate: distance 0), positive 2 away: semi-hard finds its first
        qualifying candidate at list position 0 / 63 / 64 / last, hardest finds the same graph
  4     anchor at x = 50, positive at 52: no candidate qualifies for semi-hard (the drawn negative stays)
  5     anchor at x = 200, drawn negative one of the x = 100 group: hardest has the drawn negative TIED for the minimum (it stays)
  6     anchor at x = 200, drawn negative the special at x = 0: hardest has the whole x = 100 group tied, the earliest position wins
the rest of the schedule is random."""
import functools

import numpy as np

import mining_ref as MR

CASES = [
    (3, (1, 2), 1, "random"),
    (4, (63, 64), 3, "random"),
    (5, (2, 65, 1), 4, "random"),
    (64, (64, 129, 63), 5, "random"),
    (130, (65, 63), 257, "random"),
    (1024, (2, 129), 5, "random"),
    (1, (129, 64, 65), 257, "random"),
    (1, (12, 129), 257, "crafted"),
    (130, (12, 2, 129), 257, "crafted"),
    (1024, (12, 129), 257, "crafted"),
]
IDS = ["d%d-%s-T%d-%s" % (d, "x".join(map(str, s)), T, k) for d, s, T, k in CASES]
N_CRAFTED = 7


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def build(i):
    """-> Case(emb float32 [G, dim], class_of, class_ptr, members, sched int32 [T, 3], special: list positions of the four special
    candidates (crafted) or None); built once per process, treat as read-only"""
    dim, sizes, T, kind = CASES[i]
    rng = np.random.default_rng(1000 + i)
    G, C = int(sum(sizes)), len(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    class_of = np.repeat(np.arange(C), sizes).astype(np.int32)
    lists = []
    for c in range(C):
        idx = np.arange(first[c], first[c + 1])
        perm = rng.permutation(idx)
        while idx.size > 1 and np.array_equal(perm, idx):
            perm = rng.permutation(idx)
        lists.append(perm)
    special = None
    if kind == "random":
        emb = rng.integers(-2, 3, size=(G, dim)).astype(np.float32)
    else:
        last, n_last = C - 1, sizes[-1]
        assert sizes[0] >= 12 and n_last >= 66
        emb = np.tile(rng.integers(-3, 4, size=(1, dim)), (G, 1)).astype(np.float32)
        x = np.full(G, 100.0)
        special = [0, 63, 64, n_last - 1]
        for k, pos in enumerate(special):
            x[lists[last][pos]] = 10.0 * k
        # class 0 (index order): anchors 0..3 at the specials, positives 4..7 two away, 8 / 9 the x = 50 pair, 10 / 11 at x = 200
        x[0:4] = [0, 10, 20, 30]
        x[4:8] = [2, 12, 22, 32]
        x[8:12] = [50, 52, 200, 200]
        for c in range(1, C - 1):
            x[first[c]:first[c + 1]] = 300.0 + rng.integers(0, 5, size=sizes[c])
        emb[:, dim - 1] += x.astype(np.float32)
    sched = np.zeros((T, 3), dtype=np.int32)
    for t in range(T):
        a = int(rng.integers(0, G))
        ca = int(class_of[a])
        cn = int(rng.choice([c for c in range(C) if c != ca]))
        sched[t] = (a, int(rng.integers(first[ca], first[ca + 1])), int(rng.integers(first[cn], first[cn + 1])))
    if kind == "crafted":
        group = int(lists[-1][1])                                  # a member of the x = 100 group (position 1 is never special)
        rows = [(k, 4 + k, group) for k in range(4)] + [(8, 9, group), (10, 11, int(lists[-1][2])), (10, 11, int(lists[-1][0]))]
        assert len(rows) == N_CRAFTED <= T
        sched[:N_CRAFTED] = rows
    members = np.concatenate(lists).astype(np.int32)
    return Case(dim=dim, sizes=sizes, T=T, kind=kind, emb=emb, class_of=class_of, class_ptr=first.astype(np.int32), members=members,
                sched=sched, special=special, G=G, C=C)


@functools.lru_cache(maxsize=None)
def expected(i, mode):
    """``mining_ref.mine_int`` on case i, computed once; treat as read-only"""
    c = build(i)
    out = MR.mine_int(c.emb, c.sched, c.class_of, c.class_ptr, c.members, mode)
    out.setflags(write=False)
    return out


def scenarios(i):
    """what case i contains, by the reference's own arithmetic -> set of names"""
    c = build(i)
    X = c.emb.astype(np.int64)
    semi, hard = expected(i, MR.SEMI_HARD), expected(i, MR.HARDEST)
    found = set()
    for t, (a, p, n) in enumerate(c.sched.astype(np.int64)):
        cls = c.class_of[n]
        cand = c.members[c.class_ptr[cls]:c.class_ptr[cls + 1]].astype(np.int64)
        d = MR.d2(X, a, cand)
        dn, dp = MR.d2(X, a, n), MR.d2(X, a, p)
        if (d == 0).any():
            found.add("anchor equals a candidate")
        if dn == d.min() and (d == d.min()).sum() >= 2:
            found.add("hardest: drawn negative tied for the minimum")
            assert hard[t, 2] == n
        elif dn > d.min() and (d == d.min()).sum() >= 2:
            found.add("hardest: two other candidates tied")
            assert hard[t, 2] == cand[np.flatnonzero(d == d.min())[0]]
        hit = np.flatnonzero(d < dp)
        if hit.size == 0:
            found.add("semi-hard: no qualifying candidate")
            assert semi[t, 2] == n
        else:
            assert semi[t, 2] == cand[hit[0]]
            for name, pos in (("0", 0), ("63", 63), ("64", 64), ("last", cand.size - 1)):
                if hit[0] == pos and cand.size > 64:
                    found.add("semi-hard: first qualifying candidate at position " + name)
    return found


REQUIRED = {"anchor equals a candidate", "hardest: drawn negative tied for the minimum", "hardest: two other candidates tied",
            "semi-hard: no qualifying candidate"} | {"semi-hard: first qualifying candidate at position " + s for s in ("0", "63", "64", "last")}


# ---------------------------------------------------------------------------- real-valued embeddings (standard normal, E = 64)
REAL_E, REAL_SIZES, REAL_SEEDS = 64, (300, 300), (5, 6)


@functools.lru_cache(maxsize=None)
def real_case(seed):
    """two classes of 300 standard-normal rows, every graph the anchor once, member lists permuted"""
    rng = np.random.default_rng(seed)
    G = sum(REAL_SIZES)
    emb = rng.standard_normal((G, REAL_E)).astype(np.float32)
    class_of = np.repeat([0, 1], REAL_SIZES).astype(np.int32)
    members = np.concatenate([rng.permutation(300), 300 + rng.permutation(300)]).astype(np.int32)
    a = np.arange(G)
    p = np.where(a < 300, rng.integers(0, 300, G), rng.integers(300, 600, G))
    n = np.where(a < 300, rng.integers(300, 600, G), rng.integers(0, 300, G))
    return Case(dim=REAL_E, emb=emb, class_of=class_of, class_ptr=np.array([0, 300, 600], dtype=np.int32), members=members,
                sched=np.stack([a, p, n], 1).astype(np.int32), T=G, G=G, C=2)
