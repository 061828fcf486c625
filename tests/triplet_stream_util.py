"""The seeded dataset and schedule the triplet-stream tests share (tests/test_triplet_stream_host.py, tests/test_gpu_triplet_stream.py),
and a numpy restatement of the arena's layout.

7 graphs, nmax 48, fin 12; sizes cover a graph that fills every slot and a one-node graph; graph 0 is dense enough that rows have
more than 16 neighbours (a CSR tail), graph 3 has an isolated node."""
import numpy as np

NMAX, FIN, ELL_W = 48, 12, 16
SIZES = [48, 1, 33, 17, 40, 5, 29]
# largest first, then the smallest (everything the big triplet wrote must be overwritten); one object in two roles; one object three times
SCHEDULE = np.array([[0, 2, 4], [1, 5, 3], [0, 0, 6], [4, 2, 0], [1, 1, 1]], dtype=np.int64)
ISOLATED = (3, 2)          # (graph, node)


class G:                   # stand-in for the networkx graphs cross_val.split_train_val prepares (cross_val.py:158-184)
    def __init__(self, adj, feats, n):
        self.graph = {"adj": adj, "feats": feats, "num_nodes": n, "assign_feats": feats}


def dataset(seed=11, nmax=NMAX):
    """nmax > 48: the same graphs padded further, so that the largest graph leaves ghost slots (ghost_slots = 49 < nmax)"""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(SIZES):
        p = 0.55 if i == 0 else 0.15
        a = np.triu(rng.random((n, n)) < p, 1)
        a = (a | a.T).astype(np.float32)
        if i == ISOLATED[0]:
            a[ISOLATED[1], :] = 0
            a[:, ISOLATED[1]] = 0
        adj = np.zeros((nmax, nmax), dtype=np.float32)
        adj[:n, :n] = a
        feats = np.zeros((nmax, FIN), dtype=np.float32)
        feats[:n] = rng.standard_normal((n, FIN)).astype(np.float32)
        out.append(G(adj, feats, n))
    assert (out[0].graph["adj"].sum(1) > ELL_W).any() and all((g.graph["adj"].sum(1) <= ELL_W).all() for g in out[1:])
    return out


def restate(graphs, ell_w=ELL_W):
    """the arena's arrays graph by graph, row by row (plain python): records [G, 8], and per graph its local row pointers, columns,
    tail pointers, tail columns and feature rows"""
    rec, per = [], []
    row0 = ent0 = tail0 = 0
    for i, g in enumerate(graphs):
        d = g.graph
        n = int(d["num_nodes"])
        a = np.asarray(d["adj"])[:n, :n]
        rp, col, tp, tc = [0], [], [0], []
        for r in range(n):
            nb = [int(j) for j in range(n) if a[r, j] != 0]
            col += nb
            tc += nb[ell_w:]
            rp.append(len(col))
            tp.append(len(tc))
        rec.append([n, len(col), len(tc), row0, ent0, tail0, i, 0])
        per.append((np.array(rp), np.array(col, dtype=np.int64), np.array(tp), np.array(tc, dtype=np.int64),
                    np.asarray(d["feats"], dtype=np.float32)[:n]))
        row0 += n; ent0 += len(col); tail0 += len(tc)
    return np.array(rec, dtype=np.int64), per
