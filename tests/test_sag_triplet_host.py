"""Host half of sag_triplet.tripletnet (the drop-in for Code/sag/tripletnet.py), no GPU needed:
  - pack_host: the block-diagonal CSR / batch vector / symmetry flags of three graphs against an independent construction;
  - the claim the design rests on — sag_layers.Net has no cross-graph coupling — on the fp64 oracle: three graphs in one batch give the
    embeddings of three B = 1 calls;
  - the resident cache answers only for the object an entry was built from (a recycled id() must miss);
  - CPU tensors raise the package's "GPU only" error."""
import gc
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pyg_ref as P


def _sym_graph(seed, n, e):
    g = torch.Generator().manual_seed(seed)
    s, t = torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    keep = s != t
    s, t = s[keep], t[keep]
    code = torch.unique(torch.cat([s * n + t, t * n + s]))
    return torch.stack([code // n, code % n])


class _Data:
    """stands for torch_geometric.data.Data: an ordinary object with .x and .edge_index (anything else on it is ignored)"""

    def __init__(self, x, ei):
        self.x, self.edge_index, self.y = x, ei, torch.tensor([1])


_data = _Data


def _three(fin=5, dtype=torch.float32):
    """n = 1 without edges, 7 nodes without edges, 13 nodes with a DIRECTED edge list (unsorted, one repeated edge)"""
    g = torch.Generator().manual_seed(3)
    ei13 = torch.tensor([[4, 0, 12, 3, 3, 7, 9, 1, 4, 11, 2], [0, 4, 3, 12, 5, 7, 1, 9, 0, 2, 6]])
    xs = [torch.randn(n, fin, generator=g).to(dtype) for n in (1, 7, 13)]
    return [_data(xs[0], torch.zeros(2, 0, dtype=torch.long)), _data(xs[1], torch.zeros(2, 0, dtype=torch.long)), _data(xs[2], ei13)]


def _independent(datas):
    """concatenate the offset edge lists, then build the rows target by target"""
    off, eis = 0, []
    for d in datas:
        eis.append(d.edge_index.numpy() + off)
        off += d.x.shape[0]
    ei = np.concatenate(eis, axis=1)
    want_rp, want_col = [0], []
    for t in range(off):
        want_col += sorted(int(s) for s, tt in zip(ei[0], ei[1]) if tt == t)
        want_rp.append(len(want_col))
    sizes = [d.x.shape[0] for d in datas]
    return np.asarray(want_rp, dtype=np.int32), np.asarray(want_col, dtype=np.int32), np.repeat(np.arange(len(sizes)), sizes), sizes


def test_pack_host_equals_an_independent_csr():
    from two_stage_gnn_amd import sag_triplet as ST
    three = _three()                                                       # n = 1, no edges, directed
    four = three[:2] + [_data(three[1].x, _sym_graph(5, 7, 9)), three[2]]  # ... and a symmetric graph with edges among them
    for datas, want_sym in ((three, (True, True, False)), (four, (True, True, True, False))):
        rowptr, col, batch, sizes, sym = ST.pack_host(datas)
        assert rowptr.dtype == np.int32 and col.dtype == np.int32 and batch.dtype == np.int64 and sizes.dtype == np.int64
        want_rp, want_col, want_batch, want_sizes = _independent(datas)
        assert np.array_equal(rowptr, want_rp) and np.array_equal(col, want_col)
        assert np.array_equal(sizes, want_sizes) and np.array_equal(batch, want_batch)
        assert sym == want_sym
    # one graph at a time (what the device cache stores) concatenates to the same batch
    r0 = e0 = 0
    for i, d in enumerate(datas):
        rp1, c1, _, s1, sy1 = ST.pack_host([d])
        n = int(s1[0])
        assert np.array_equal(rp1 + e0, rowptr[r0: r0 + n + 1]) and np.array_equal(c1 + r0, col[e0: e0 + c1.size]) and sy1 == (sym[i],)
        r0, e0 = r0 + n, e0 + c1.size
    with pytest.raises(IndexError):
        ST.pack_host([_data(torch.zeros(3, 2), torch.tensor([[0, 3], [1, 0]]))])


@pytest.mark.parametrize("conv", ["gcn", "sage"])
def test_three_graphs_in_one_batch_equal_three_single_graph_calls_fp64(conv):
    """eval mode, nhid 16, ratio 0.5, graphs of 1, 7 (no edges) and 13 nodes; the edge list / batch vector are pack_host's"""
    from two_stage_gnn_amd import sag_triplet as ST
    fin, nhid, C = 5, 16, 8
    datas = _three(fin, torch.float64)
    datas[2] = _data(datas[2].x, _sym_graph(7, 13, 20))
    rowptr, col, batch, sizes, _ = ST.pack_host(datas)
    tgt = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    ei = torch.from_numpy(np.stack([col.astype(np.int64), tgt.astype(np.int64)]))
    x = torch.cat([d.x for d in datas])
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.4
    p = {}
    for i, k in ((1, fin), (2, nhid), (3, nhid)):
        if conv == "gcn":
            p["conv%d.weight" % i], p["conv%d.bias" % i] = r(k, nhid), r(nhid)
        else:
            p["conv%d.lin_l.weight" % i], p["conv%d.lin_l.bias" % i], p["conv%d.lin_r.weight" % i] = r(nhid, k), r(nhid), r(nhid, k)
        p["pool%d.score_layer.weight" % i], p["pool%d.score_layer.bias" % i] = r(nhid, 1), r(1)
    p["lin1.weight"], p["lin1.bias"] = r(nhid, 2 * nhid), r(nhid)
    p["lin2.weight"], p["lin2.bias"] = r(nhid // 2, nhid), r(nhid // 2)
    p["lin3.weight"], p["lin3.bias"] = r(C, nhid // 2), r(C)
    together = P.sag_net(p, x, ei, 0.5, batch=torch.from_numpy(batch), conv=conv)
    alone = torch.cat([P.sag_net(p, d.x, d.edge_index, 0.5, batch=torch.zeros(d.x.size(0), dtype=torch.long), conv=conv) for d in datas])
    err = float((together - alone).abs().max())
    print("max |batched - single| = %.3g" % err)
    assert err <= 1e-13, err


def test_cache_misses_on_a_recycled_id():
    from two_stage_gnn_amd import sag_triplet as ST
    cache = ST.ResidentCache()
    a = _three()[2]
    ea = cache.store(a, ST._Graph())
    assert cache.lookup(a) is ea and (cache.hits, cache.misses) == (1, 0)
    # an entry filed under another object's id (what a recycled id() amounts to) does not answer for that object
    b = _three()[1]
    cache._entries[(id(b), None)] = ea
    assert cache.lookup(b) is None and cache.misses == 1
    del cache._entries[(id(b), None)]
    # the real thing: the object dies, its entry goes with it, and whatever is allocated at its address next misses
    key = (id(a), None)
    del a
    gc.collect()
    assert key not in cache._entries and len(cache) == 0
    keep = []
    for _ in range(2000):
        c = _three()[2]
        if (id(c), None) == key:
            assert cache.lookup(c) is None
            break
        keep.append(c)
    # an object that cannot be weakly referenced is kept alive by its entry instead (its id cannot be recycled)
    s = types.SimpleNamespace(x=None, edge_index=None)
    with pytest.raises(TypeError):
        import weakref
        weakref.ref(s)
    es = cache.store(s, ST._Graph())
    assert cache.lookup(s) is es and es.ref() is s


def test_forward_on_cpu_tensors_raises_gpu_only():
    from two_stage_gnn_amd import sag_layers as S, sag_triplet as ST
    net = ST.tripletnet(S.Net(5, 16, 8, 0.5, 0.0))
    a, p, n = _three()
    with pytest.raises(RuntimeError, match="GPU only"):
        net(a, p, n)
    assert len(net.cache) == 0
