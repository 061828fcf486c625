"""What the SAGPool mini-batch stream's tests share (tests/test_sag_minibatch_host.py, tests/test_gpu_sag_minibatch.py): datasets with
labels, schedules, a numpy restatement of the gather launch (tsgnn_sag_batch_gather_f32, csrc/sag_batch_stream.hip) and the CPU oracle's
step on a mini-batch.

Datasets (parameters of test_gpu_sag_triplet.NET_SEED, conv="gcn", ratio 0.5, use_batch=True; the head's class count is this file's:
the fused head takes at most 16 classes):
  small12  sag_stream_util's small6 (n = 1, 7, 13, 9, 31, 17; graph 1 has no edges) + the extension: n = 2, 3, 32, 33, 64 and a graph
           of 4 nodes whose edge list is only self loops; fin 5, nhid 32, C 8
  dd3      sag_stream_util's dd3 (n = 150, 420, 290); fin 89, nhid 128, C 2
  fin1     four small graphs of ONE feature column (ld 4): the gather launch alone
  many40   40 graphs of n = 1..40 (fin 5, nhid 32, C 8): B = 128 with duplicates, and the epoch at B = 8
The extension's and many40's graph seeds were searched on the CPU so that no graph has an ambiguous pooling cut in the fp64 oracle
(test_sag_minibatch_host.test_no_graph_is_ambiguous): no entry of any schedule may be left out of a comparison."""
import numpy as np
import torch

import sag_stream_util as U0
from sag_stream_util import _D, _ambiguous, _net, _params, NET_SEED, RATIO  # noqa: F401
from test_gpu_sag_triplet import _graph

DEPTH = 3
EXT = [(2, 1.0, 605), (3, 1.0, 601), (32, 2.2, 4), (33, 2.2, 5), (64, 2.5, 6)]   # (n, edges per node, graph seed)
SELF_LOOPS_SEED = 7
# n -> seed, where 500 + n pools ambiguously (sparse random graphs pool into two-node components, whose GCN scores tie exactly)
MANY_SEEDS = {2: 621, 3: 610, 4: 604, 5: 615, 7: 600, 10: 602, 13: 601, 14: 603, 19: 600, 21: 601, 24: 600}
DIMS = {"small12": (5, 32, 8), "dd3": (89, 128, 2), "fin1": (1, 32, 8), "many40": (5, 32, 8)}
SIZES = {"small12": [1, 7, 13, 9, 31, 17, 2, 3, 32, 33, 64, 4], "dd3": [150, 420, 290], "fin1": [5, 1, 12, 8], "many40": list(range(1, 41))}
# the largest entry first, then the smallest; B copies of the n = 1 graph; an entry without any edge; permutations
SCHEDULES = {
    ("small12", 3): np.array([[10, 9, 8], [0, 6, 7], [0, 0, 0], [1, 0, 1], [4, 11, 5], [2, 2, 3]], dtype=np.int64),
    ("small12", 4): np.array([[10, 9, 8, 4], [0, 6, 7, 1], [0, 0, 0, 0], [1, 0, 1, 0], [11, 3, 2, 5]], dtype=np.int64),
    ("dd3", 3): np.array([[1, 2, 1], [0, 2, 0], [2, 0, 1]], dtype=np.int64),
    ("dd3", 2): np.array([[1, 2], [0, 0], [2, 1]], dtype=np.int64),
}
_CACHE = {}


def dataset(name):
    """-> fin, nhid, C, [(x, edge_index)] on the CPU, labels int64 [G]"""
    if name not in _CACHE:
        fin, nhid, C = DIMS[name]
        if name == "small12":
            graphs = list(U0.dataset("small6")[3]) + [_graph(seed, n, fin, e) for n, e, seed in EXT]
            loops = torch.tensor([[0, 1, 2, 3, 2], [0, 1, 2, 3, 2]])                  # (node 2's self loop twice: repeated edges stay)
            graphs.append((_graph(SELF_LOOPS_SEED, 4, fin, 0)[0], loops))
        elif name == "dd3":
            graphs = list(U0.dataset("dd3")[3])
        elif name == "fin1":
            graphs = [_graph(40 + i, n, fin, 1.5) for i, n in enumerate(SIZES[name])]
        else:
            graphs = [_graph(MANY_SEEDS.get(n, 500 + n), n, fin, 2.0) for n in SIZES[name]]
        assert [int(x.shape[0]) for x, _ in graphs] == SIZES[name]
        labels = (np.arange(len(graphs), dtype=np.int64) * 3 + 1) % C
        _CACHE[name] = (fin, nhid, C, graphs, labels)
    return _CACHE[name]


def datas(name, dev="cuda"):
    fin, nhid, C, graphs, labels = dataset(name)
    out = []
    for (x, ei), y in zip(graphs, labels):
        d = _D(x, ei, dev)
        d.y = torch.tensor([int(y)])
        out.append(d)
    return out


def net(name, mode="eval", p_drop=0.0, dev="cuda", use_batch=True, **kw):
    fin, nhid, C = DIMS[name]
    m = _net(fin, nhid, C, kw.pop("conv", "gcn"), use_batch, p_drop, seed=NET_SEED, dev=dev)
    for k, v in kw.items():
        setattr(m, k, v)
    return m.train(mode == "train")


def schedule(name, B):
    """the schedule of (name, B); where none is written down: the graphs in order, wrapping, with duplicates where B exceeds the
    dataset — the largest entry first, then the smallest, B copies of graph 0, and a rotation"""
    if (name, B) in SCHEDULES:
        return SCHEDULES[(name, B)]
    G = len(SIZES[name])
    order = np.argsort(SIZES[name])[::-1]
    big = order[np.arange(B) % G]
    small = order[::-1][np.arange(B) % G]
    rows = [big, small, np.zeros(B, dtype=np.int64), np.roll(np.arange(G), 5)[np.arange(B) % G]]
    if name == "small12":
        rows.insert(3, np.array([1, 0])[np.arange(B) % 2])                        # an entry without any edge
    return np.asarray(rows, dtype=np.int64)


def k_chain(n, ratio, depth=DEPTH):
    """the brute-force loop the vectorised helpers are held to"""
    out = [int(n)]
    for _ in range(depth):
        m = out[-1]
        out.append(min(m, int(np.ceil(np.float32(ratio) * np.float32(m)))))
    return out


_COEF = {}


def _coef(per, i):
    """(dinv, self_w) of graph i's rows, row by row: PyG's gcn_norm on unit weights — a row's entries, plus one where none of them is the
    row itself (add_remaining_self_loops keeps an existing self loop)"""
    key = (id(per), i)
    if key not in _COEF:
        rp, c, _ = per[i]
        n = rp.size - 1
        dinv, self_w = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        for r in range(n):
            lo, hi = int(rp[r]), int(rp[r + 1])
            has_self = bool((c[lo:hi] == r).any())
            d = np.float32(hi - lo) + np.float32(0.0 if has_self else 1.0)
            di = np.float32(1.0) / np.sqrt(d, dtype=np.float32)
            dinv[r], self_w[r] = di, np.float32(0.0) if has_self else di * di
        _COEF[key] = (per, dinv, self_w)                    # (``per`` stays referenced: its id() cannot be recycled)
    return _COEF[key][1:]


def launch_np(rec, per, labels, ids, ratio, depth, row_cap, nnz_cap, level_caps, ldg, ld, col_fill=-1):
    """the gather launch restated in numpy, graph by graph and row by row, for an entry that fits: every array it writes, padding
    included (``col`` past the batch's nnz keeps ``col_fill``: the launch does not touch it).  ``rec, per``: ``sag_stream_util.restate``"""
    ids = [int(i) for i in ids]
    B = len(ids)
    rowptr = np.zeros(row_cap + 1, dtype=np.int32)
    col = np.full(nnz_cap, col_fill, dtype=np.int32)
    x = np.zeros((row_cap, ld), dtype=np.float32)
    dinv, self_w = np.zeros(row_cap, dtype=np.float32), np.zeros(row_cap, dtype=np.float32)
    r0 = e0 = 0
    for i in ids:
        rp, c, feats = per[i]
        n = int(rec[i][0])
        di_g, sw_g = _coef(per, i)
        rowptr[r0:r0 + n] = rp[:n] + e0
        col[e0:e0 + int(rp[n])] = c + r0
        dinv[r0:r0 + n], self_w[r0:r0 + n] = di_g, sw_g
        x[r0:r0 + n, :feats.shape[1]] = feats
        r0 += n
        e0 += int(rp[n])
    assert r0 <= row_cap and e0 <= nnz_cap
    rowptr[r0:] = e0
    gp = np.zeros((depth + 1, ldg), dtype=np.int32)
    chains = np.array([k_chain(int(rec[i][0]), ratio, depth) for i in ids], dtype=np.int64)
    for l in range(depth + 1):
        pre = np.cumsum(chains[:, l])
        assert pre[-1] <= level_caps[l]
        gp[l, 1:B + 1] = pre
        gp[l, B + 1:] = pre[-1]
    return {"rowptr": rowptr, "col": col, "x": x, "dinv": dinv, "self_w": self_w, "gp": gp, "ids": np.asarray(ids, dtype=np.int32),
            "label": np.asarray([labels[i] for i in ids], dtype=np.int64)}


def collate_np(graphs, ids):
    """``sag_triplet.pack_host``-style collation of the same graphs (an independent route: edge lists, not the arena)"""
    from two_stage_gnn_amd import sag_triplet as ST

    class _H:
        def __init__(self, x, ei):
            self.x, self.edge_index = x, ei
    rowptr, col, batch, sizes, sym = ST.pack_host([_H(*graphs[int(i)]) for i in ids])
    x = np.concatenate([graphs[int(i)][0].numpy().astype(np.float32) for i in ids])
    return rowptr, col, batch, sizes, x


_ORACLE = {}


def oracle(name, ids):
    """the fp64 and fp32 CPU oracle's step on the mini-batch ``ids`` (``pyg_ref.sag_net`` WITH the batch vector, ``F.nll_loss``,
    backward), computed once: {dtype: (logp, loss, {parameter: grad})}"""
    from oracle import pyg_ref as P
    key = (name, tuple(int(i) for i in ids))
    if key not in _ORACLE:
        fin, nhid, C, graphs, labels = dataset(name)
        m = net(name, dev="cpu")
        xs, eis, bv, off = [], [], [], 0
        for b, i in enumerate(key[1]):
            x, ei = graphs[i]
            xs.append(x); eis.append(ei + off); bv.append(torch.full((x.shape[0],), b, dtype=torch.long))
            off += int(x.shape[0])
        x, ei, bv = torch.cat(xs), torch.cat(eis, dim=1), torch.cat(bv)
        y = torch.as_tensor(labels[list(key[1])])
        out = {}
        for dt in (torch.float64, torch.float32):
            p = _params(m, dt)
            logp = P.sag_net(p, x.to(dt), ei, RATIO, batch=bv, conv="gcn")
            loss = torch.nn.functional.nll_loss(logp, y)
            loss.backward()
            out[dt] = (logp.detach(), float(loss.detach()), {k: v.grad for k, v in p.items()})
        _ORACLE[key] = out
    return _ORACLE[key]
