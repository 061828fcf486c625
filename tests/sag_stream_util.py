"""The datasets, schedules and references the SAGPool triplet-stream tests share (tests/test_sag_stream_host.py,
tests/test_gpu_sag_stream.py), and a plain-python restatement of the arena's layout.

Datasets are built from the graphs of tests/test_gpu_sag_triplet.py's CASES with the parameters of NET_SEED, conv="gcn", ratio 0.5:
  small6   the six graphs of "n1_noedges" + "odd" (n = 1, 7, 13, 9, 31, 17; graph 1 has no edges); fin 5, nhid 32, C 8: level 0 takes the
           narrow gcn_propagate_affine route
  dd3      the three graphs of "dd" (n = 150, 420, 290); fin 89, nhid 128, C 64: propagate + MFMA product, the merged weight-gradient
           launch
Schedules follow triplet_stream_util.SCHEDULE's pattern: the largest triplet first, then the smallest (everything the big one wrote must
be overwritten or be padding), one object in two roles, a permutation, one object three times."""
import numpy as np
import torch

from test_gpu_sag_triplet import CASES, NET_SEED, RATIO, _D, _ambiguous, _net, _oracle_step, _params, _triplet  # noqa: F401

MARGIN = 1.5           # test_gpu_sag_triplet._oracle_step's
DATASETS = {"small6": ("n1_noedges", "odd"), "dd3": ("dd",)}
SCHEDULES = {
    "small6": np.array([[4, 5, 2], [0, 1, 3], [2, 2, 5], [2, 5, 4], [3, 3, 3]], dtype=np.int64),
    # (the last entry fills the capacity: no padding row at any level)
    "dd3": np.array([[1, 2, 1], [0, 2, 0], [1, 2, 0], [2, 0, 1], [1, 1, 1]], dtype=np.int64),
}
SIZES = {"small6": [1, 7, 13, 9, 31, 17], "dd3": [150, 420, 290]}


def dataset(name):
    """-> fin, nhid, C, [(x, edge_index)] on the CPU"""
    graphs, dims = [], None
    for case in DATASETS[name]:
        fin, nhid, C, g = _triplet(case)
        assert dims in (None, (fin, nhid, C))
        dims = (fin, nhid, C)
        graphs += g
    assert [int(x.shape[0]) for x, _ in graphs] == SIZES[name]
    return dims + (graphs,)


def datas(graphs, dev="cuda"):
    return [_D(x, ei, dev) for x, ei in graphs]


def net(name, mode="eval", p_drop=0.0, dev="cuda", **kw):
    fin, nhid, C, _ = dataset(name)
    m = _net(fin, nhid, C, kw.pop("conv", "gcn"), False, p_drop, seed=NET_SEED, dev=dev)
    for k, v in kw.items():
        setattr(m, k, v)
    return m.train(mode == "train")


def restate(graphs):
    """the arena graph by graph, row by row (plain python): records [G, 8], and per graph its local row pointers, its columns (rows are
    targets, sources ascending, repeated edges kept) and its feature rows"""
    rec, per = [], []
    row0 = ent0 = 0
    for i, (x, ei) in enumerate(graphs):
        n = int(x.shape[0])
        src, dst = ei[0].tolist(), ei[1].tolist()
        rp, col = [0], []
        for r in range(n):
            col += sorted(s for s, d in zip(src, dst) if d == r)
            rp.append(len(col))
        rec.append([n, len(col), row0, ent0, i, 0, 0, 0])
        per.append((np.array(rp, dtype=np.int64), np.array(col, dtype=np.int64), x.numpy().astype(np.float32)))
        row0 += n; ent0 += len(col)
    return np.array(rec, dtype=np.int64), per


_ORACLE = {}


def oracle(name, ids):
    """the fp64 and fp32 CPU oracle's step on schedule entry ``ids`` (three B = 1 forwards, margin loss, backward), computed once:
    {dtype: (dp, dn, [embeds], loss, {parameter: grad})}"""
    key = (name, tuple(int(i) for i in ids))
    if key not in _ORACLE:
        fin, nhid, C, graphs = dataset(name)
        m = _net(fin, nhid, C, "gcn", False, 0.0, seed=NET_SEED, dev="cpu")
        out = {}
        for dt in (torch.float64, torch.float32):
            p = _params(m, dt)
            dp, dn, e, loss = _oracle_step(p, [graphs[i] for i in key[1]], "gcn")
            out[dt] = (dp, dn, e, loss, {k: v.grad for k, v in p.items()})
        _ORACLE[key] = out
    return _ORACLE[key]
