"""The seeded dataset and schedules the mini-batch-stream tests share (tests/test_minibatch_stream_host.py,
tests/test_gpu_minibatch_stream.py), the same graphs as a CSR-resident TU dataset, and a numpy restatement of the gather launch.

24 graphs, nmax 48 (graph 0 fills every slot) or 64 (ghost slots to spare), fin 9 (ld 12: three pad columns), three label classes;
graph 1 has one node, graph 2 is dense enough that its rows have more than 16 neighbours (a CSR tail), graph 3 has an isolated node.
The node-label variant (``onehot=True``) carries the one-hot rows of its 9 node labels as features."""
import numpy as np

NMAX, FIN, LD, ELL_W, N_CLASSES = 48, 9, 12, 16, 3
SIZES = [48, 1, 30, 17, 40, 5, 29, 3, 12, 45, 7, 22, 2, 36, 9, 14, 4, 27, 11, 6, 33, 8, 19, 10]
FULL, ONE_NODE, TAIL, ISOLATED = 0, 1, 2, (3, 2)          # graph ids; ISOLATED = (graph, node)
BATCHES = [1, 3, 8, 9, 32, 33, 64, 65, 128]


class G:                   # stand-in for the networkx graphs cross_val.split_train_val prepares (cross_val.py:158-184)
    def __init__(self, adj, feats, n, label, node_label):
        self.graph = {"adj": adj, "feats": feats, "num_nodes": n, "assign_feats": feats, "label": label, "node_label": node_label}


def dataset(seed=23, nmax=NMAX, onehot=False):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(SIZES):
        p = 0.8 if i == TAIL else 0.15
        a = np.triu(rng.random((n, n)) < p, 1)
        a = (a | a.T).astype(np.float32)
        if i == ISOLATED[0]:
            a[ISOLATED[1], :] = 0
            a[:, ISOLATED[1]] = 0
        adj = np.zeros((nmax, nmax), dtype=np.float32)
        adj[:n, :n] = a
        nl = rng.integers(0, FIN, size=n).astype(np.int64)
        dense = rng.standard_normal((n, FIN)).astype(np.float32)
        feats = np.zeros((nmax, FIN), dtype=np.float32)
        if onehot:
            feats[np.arange(n), nl] = 1.0
        else:
            feats[:n] = dense
        out.append(G(adj, feats, n, int(i % N_CLASSES), nl))
    deg = [g.graph["adj"].sum(1) for g in out]
    assert (deg[TAIL] > ELL_W).any() and all((d <= ELL_W).all() for i, d in enumerate(deg) if i != TAIL)
    return out


def tu_dataset(graphs):
    """the same graphs as a ``tu_data.TUDataset`` (one CSR over all nodes, sorted columns), straight from the dense adjacencies"""
    from two_stage_gnn_amd.tu_data import TUDataset
    gp, rowptr, col, nl, off = [0], [0], [], [], 0
    for g in graphs:
        d = g.graph
        n = int(d["num_nodes"])
        a = np.asarray(d["adj"])[:n, :n]
        for r in range(n):
            col += [int(j) + off for j in np.flatnonzero(a[r])]
            rowptr.append(len(col))
        nl += [int(v) for v in d["node_label"]]
        off += n
        gp.append(off)
    return TUDataset(np.asarray(gp, dtype=np.int64), np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64),
                     np.asarray([g.graph["label"] for g in graphs], dtype=np.int64), np.asarray(nl, dtype=np.int64), None, FIN)


def feature_table(graphs):
    """float32 [nodes, FIN]: the graphs' feature rows, graph after graph"""
    return np.concatenate([np.asarray(g.graph["feats"], dtype=np.float32)[:int(g.graph["num_nodes"])] for g in graphs])


def tail_counts(graphs, ell_w=ELL_W):
    return np.array([int(np.maximum(np.asarray(g.graph["adj"]).sum(1) - ell_w, 0).sum()) for g in graphs], dtype=np.int64)


def plan(B, graphs, seed=5):
    """-> (schedule int64 [T, B], row_cap, tail_cap): row_cap is EXACTLY the first entry's row count (no rounding) and tail_cap the
    largest tail sum of any entry rounded up to 4.  Entries: 0 the B largest graphs (B > 24: every graph, the rest drawn from the
    graphs of at most 12 nodes), 1 copies of the four smallest graphs (at least 40 rows below the capacity), 2 (B >= 2) entry 0 with
    its two largest places given to the one-node graph (duplicate ids), 3 entry 0 with its largest place given to the tail graph,
    4 (B >= 2) entry 0 in another order."""
    sizes = np.asarray(SIZES)
    rng = np.random.default_rng(seed + B)
    order = np.argsort(-sizes, kind="stable")
    if B <= len(sizes):
        full = order[:B].copy()
    else:
        small = np.flatnonzero(sizes <= 12)
        full = np.concatenate([order, rng.choice(small, B - len(sizes))])
    by_size = np.argsort(-sizes[full], kind="stable")             # places of `full`, the largest graph first
    entries = [full, np.resize(np.argsort(sizes, kind="stable")[:4], B)]
    if B >= 2:
        dup = full.copy()
        dup[by_size[:2]] = ONE_NODE
        entries.append(dup)
    tail = full.copy()
    tail[by_size[0]] = TAIL
    entries.append(tail)
    if B >= 2:
        entries.append(rng.permutation(full))
    sched = np.stack(entries).astype(np.int64)
    row_cap = int(sizes[full].sum())
    tail_cap = int(tail_counts(graphs)[sched].sum(1).max())
    return sched, row_cap, max((tail_cap + 3) // 4 * 4, 4)


def check_plan(B, sched, row_cap, graphs):
    """what every schedule of the gather test must contain (asserted on the host, in the test)"""
    sizes = np.asarray(SIZES)
    rows = sizes[sched].sum(1)
    assert sched.shape[1] == B and rows.max() == row_cap and (rows == row_cap).any(), rows
    assert rows.min() <= row_cap - 40, rows
    assert (sched == ONE_NODE).any() and (sched == TAIL).any()
    assert B == 1 or any(len(set(e.tolist())) < B for e in sched)
    assert max(SIZES) <= row_cap


def restate_launch(graphs, ids, nmax, row_cap, ell_w=ELL_W, onehot=False):
    """the gather launch of one entry in plain python: every output array as the launch must leave it (``tail_col`` / ``tail_slots``
    only up to the entry's tail).  Rows [0, n) real, [n, row_cap) padding of the dummy graph B, [row_cap, +nmax) ghost slots."""
    B, R = len(ids), row_cap + nmax
    n_of = [int(graphs[i].graph["num_nodes"]) for i in ids]
    n = sum(n_of)
    assert n <= row_cap
    out = {"graph_ptr": np.zeros(B + 2, dtype=np.int32), "slot_count": np.zeros(nmax, dtype=np.int32),
           "row_graph": np.full(row_cap, B, dtype=np.int32), "row_slot": np.full(row_cap, -1, dtype=np.int32),
           "ell": np.full(R * ell_w, -1, dtype=np.int32), "ell_slots": np.full(R * ell_w, -1, dtype=np.int32),
           "tail_ptr": np.zeros(R + 1, dtype=np.int32), "x": np.zeros((R, LD), dtype=np.float32),
           "ids": np.asarray(ids, dtype=np.int32), "label": np.asarray([graphs[i].graph["label"] for i in ids], dtype=np.int64)}
    tail_col, tail_slots = [], []
    g0 = 0
    for b, i in enumerate(ids):
        d = graphs[i].graph
        nb = n_of[b]
        out["graph_ptr"][b] = g0
        a = np.asarray(d["adj"])[:nb, :nb]
        for s in range(nb):
            r = g0 + s
            out["row_graph"][r], out["row_slot"][r] = b, s
            out["tail_ptr"][r] = len(tail_col)
            nbrs = [int(j) for j in np.flatnonzero(a[s])]
            for k, j in enumerate(nbrs):
                if k < ell_w:
                    out["ell"][r * ell_w + k] = j + g0
                    out["ell_slots"][r * ell_w + k] = (j << 20) | (j + g0)
                else:
                    tail_col.append(j + g0)
                    tail_slots.append((j << 20) | (j + g0))
            if onehot:
                out["x"][r, int(d["node_label"][s])] = 1.0
            else:
                out["x"][r, :FIN] = np.asarray(d["feats"], dtype=np.float32)[s]
        for s in range(min(nb, nmax)):
            out["slot_count"][s] += 1
        g0 += nb
    out["graph_ptr"][B], out["graph_ptr"][B + 1] = n, row_cap
    out["tail_ptr"][n:] = len(tail_col)
    out["tail_col"], out["tail_slots"] = np.asarray(tail_col, dtype=np.int32), np.asarray(tail_slots, dtype=np.int32)
    return out
