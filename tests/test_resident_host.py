"""``resident.py`` without a GPU: the block-diagonal CSR concatenation against an independent construction (the dense block-diagonal
matrix through ``dense_csr_host``), both of its routes, its edge rules (no edges, mixed weights), the host conversions, the dense
family's cache entry that dies with its array, the one ``RESIDENT`` switch and ``per_graph_statistics``."""
import gc
import types

import numpy as np
import pytest
import torch

from two_stage_gnn_amd import resident as RS

NMAX = 16
SIZES = [1, 7, 13, 2, 16, 5, 16, 3, 9, 1, 11, 4, 16, 8, 2, 6, 10, 12, 15, 14]


def _adjacencies(count):
    """[NMAX, NMAX] arrays, real part [:n, :n]: graph 0 is one node without an edge, graph 1 seven nodes without any edge, the others
    random with non-unit weights, every second one symmetric"""
    rng = np.random.default_rng(11)
    out = []
    for i, n in enumerate(SIZES[:count]):
        a = np.zeros((NMAX, NMAX), dtype=np.float32)
        if i >= 2:
            w = (rng.random((n, n)) < 0.3) * rng.uniform(0.5, 2.0, (n, n))
            a[:n, :n] = np.maximum(w, w.T) if i % 2 else w
        out.append(a)
    return out


def _piece(a, n, weighted=True):
    rp, col, val, sym = RS.dense_csr_host(a, n)
    return (torch.from_numpy(rp), torch.from_numpy(col), torch.from_numpy(val) if weighted else None, n, int(col.size), sym)


@pytest.mark.parametrize("closing", [1, NMAX + 1])
@pytest.mark.parametrize("count", [1, 3, 8, 9, 20])
def test_concat_csr_equals_the_csr_of_the_block_diagonal_matrix(count, closing):
    assert RS._PER_PIECE_MAX == 8                                            # (8 and 9 pieces straddle the two routes)
    sizes = SIZES[:count]
    adjs = _adjacencies(count)
    N = sum(sizes)
    block = np.zeros((N, N), dtype=np.float32)
    r0 = 0
    for a, n in zip(adjs, sizes):
        block[r0:r0 + n, r0:r0 + n] = a[:n, :n]
        r0 += n
    rp, col, val, sym = RS.dense_csr_host(block, N)
    want_rp = np.concatenate([rp[:-1], np.full(closing, col.size, dtype=np.int32)])
    pieces = [_piece(a, n) for a, n in zip(adjs, sizes)]
    assert count < 3 or {p[5] for p in pieces} == {True, False}
    routes = [RS.concat_csr(pieces, closing, per_piece=pp) for pp in (None, True, False)]
    for got_rp, got_col, got_val, nnz, got_sym in routes:
        assert nnz == col.size and got_sym == sym
        assert got_rp.dtype == torch.int32 and got_col.dtype == torch.int32 and got_val.dtype == torch.float32
        assert np.array_equal(got_rp.numpy(), want_rp)
        if nnz:
            assert np.array_equal(got_col.numpy(), col) and np.array_equal(got_val.numpy(), val)
        else:                                                                # no edges: one zero, so the kernels get a valid pointer
            assert got_col.tolist() == [0] and got_val.tolist() == [0.0]
    for other in routes[1:]:
        assert all(torch.equal(a, b) for a, b in zip(routes[0][:3], other[:3]))


@pytest.mark.parametrize("per_piece", [True, False])
def test_concat_csr_of_empty_pieces(per_piece):
    pieces = [_piece(np.zeros((NMAX, NMAX), np.float32), n, weighted=False) for n in (1, 7, 4)]
    for closing in (1, NMAX + 1):
        rp, col, val, nnz, sym = RS.concat_csr(pieces, closing, per_piece=per_piece)
        assert nnz == 0 and val is None and sym and col.dtype == torch.int32 and col.tolist() == [0]
        assert rp.dtype == torch.int32 and rp.tolist() == [0] * (12 + closing)


@pytest.mark.parametrize("per_piece", [True, False])
def test_concat_csr_fills_missing_weights_with_ones(per_piece):
    a, b = _adjacencies(4)[2:]
    unit = (a != 0).astype(np.float32)
    pa, pb, pu = _piece(a, 13), _piece(b, 2), _piece(unit, 13, weighted=False)
    assert pu[2] is None and pu[4] == pa[4] > 0 and pb[4] > 0
    _, col, val, nnz, _ = RS.concat_csr([pu, pb], 1, per_piece=per_piece)
    assert torch.equal(val, torch.cat([torch.ones(pu[4]), pb[2]])) and nnz == col.numel() == val.numel()
    _, _, val, _, _ = RS.concat_csr([pb, pu, pa], NMAX + 1, per_piece=per_piece)
    assert torch.equal(val, torch.cat([pb[2], torch.ones(pu[4]), pa[2]]))
    assert RS.concat_csr([pu, pu], 1, per_piece=per_piece)[2] is None        # nobody weighted: no val at all


def test_dense_csr_host():
    a = np.full((6, 6), 9.0, dtype=np.float32)                               # rubbish in the padding
    a[:4, :4] = [[0, 2, 0, 0.5], [2, 0, 0, 0], [0, 0, 0, 0], [0.5, 0, 0, 3]]
    rp, col, val, sym = RS.dense_csr_host(a, 4)
    assert (rp.dtype, col.dtype, val.dtype) == (np.int32, np.int32, np.float32)
    assert rp.tolist() == [0, 2, 3, 3, 5] and col.tolist() == [1, 3, 0, 0, 3] and val.tolist() == [2.0, 0.5, 2.0, 0.5, 3.0] and sym
    a[2, 0] = 1.0                                                            # an edge without its reverse
    rp, col, val, sym = RS.dense_csr_host(a, 4)
    assert not sym and rp.tolist() == [0, 2, 3, 4, 6] and col.tolist() == [1, 3, 0, 0, 0, 3]
    rp, col, val, sym = RS.dense_csr_host(a, 0)
    assert rp.tolist() == [0] and col.size == 0 and val.size == 0 and sym


@pytest.mark.parametrize("width,stride", [(1, 4), (4, 4), (6, 8)])
def test_padded_rows(width, stride):
    f = np.arange(5 * width, dtype=np.float64).reshape(5, width) + 1.0
    out = RS.padded_rows(f, 3, torch.device("cpu"))
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, stride) and out.stride() == (stride, 1)
    assert np.array_equal(out[:, :width].numpy(), f[:3].astype(np.float32)) and not out[:, width:].any()


class _G:
    def __init__(self, adj, feats, n, assign=None):
        self.graph = {"adj": adj, "feats": feats, "num_nodes": n, "assign_feats": feats if assign is None else assign}


def test_dense_entry_counts_its_uploads_and_dies_with_its_array():
    from two_stage_gnn_amd import triplet as T
    cpu = torch.device("cpu")
    cache = RS.ResidentCache()
    rng = np.random.default_rng(3)
    feats = rng.normal(size=(NMAX, 6)).astype(np.float32)
    unit = (_adjacencies(3)[2] != 0).astype(np.float32)
    g = _G(unit, feats, 13)
    e = T.resident_graph(g, cpu, cache)
    assert (cache.hits, cache.misses, cache.h2d, len(cache)) == (0, 1, 3, 1)          # rowptr, col, feats: unit weights, no val
    assert e.val is None and e.assign is None and (e.n, e.nmax, e.nnz) == (13, NMAX, int(unit.sum())) and e.feats.shape == (13, 8)
    assert T.resident_graph(g, cpu, cache) is e and (cache.hits, cache.misses, cache.h2d) == (1, 1, 3)
    assert [(k, v) for k, v in cache] == cache.items() == [((id(unit), None), e)]
    w = _G(_adjacencies(3)[2], feats, 13, assign=feats[:, :3].copy())
    ew = T.resident_graph(w, cpu, cache)
    assert ew.val is not None and ew.assign.shape == (13, 4) and (cache.misses, cache.h2d, len(cache)) == (2, 8, 2)
    del g, unit
    gc.collect()
    assert len(cache) == 1 and cache.items()[0][1] is ew                     # the entry went with its array
    del w
    gc.collect()
    assert len(cache) == 0


def test_triplet_resident_is_the_one_switch(monkeypatch):
    from two_stage_gnn_amd import sag_layers as S, sag_triplet as ST, triplet as T
    monkeypatch.setattr(RS, "RESIDENT", True)                                # (whatever TSGNN_TRIPLET_CACHE says here)
    assert T.RESIDENT is True
    model = S.Net(5, 16, 8, 0.5, 0.0)
    assert ST.tripletnet(model).cache is RS.resident_cache(model)
    monkeypatch.setattr(T, "RESIDENT", False)
    assert RS.RESIDENT is False and T.RESIDENT is False
    own = ST.tripletnet(model).cache
    assert own is not RS.resident_cache(model) and isinstance(own, RS.ResidentCache)
    T.RESIDENT = True
    assert RS.RESIDENT is True and ST.tripletnet(model).cache is RS.resident_cache(model)


def test_per_graph_statistics_restores_and_creates_nothing():
    m = types.SimpleNamespace(per_graph_bn=False)
    with RS.per_graph_statistics(m):
        assert m.per_graph_bn is True
    assert m.per_graph_bn is False
    m.per_graph_bn = "before"
    with pytest.raises(RuntimeError, match="inside"):
        with RS.per_graph_statistics(m):
            assert m.per_graph_bn is True
            raise RuntimeError("inside")
    assert m.per_graph_bn == "before"
    bare = types.SimpleNamespace()
    with RS.per_graph_statistics(bare):
        assert not hasattr(bare, "per_graph_bn")
    assert not hasattr(bare, "per_graph_bn")


def test_torch_distances():
    e = torch.randn(3, 5, generator=torch.Generator().manual_seed(0))
    dp, dn, a, p, n = RS.torch_distances(e)
    assert torch.equal(dp, torch.nn.functional.pairwise_distance(e[0:1], e[1:2], 2)) and dp.shape == (1,)
    assert torch.equal(dn, torch.nn.functional.pairwise_distance(e[0:1], e[2:3], 2))
    assert torch.equal(a, e[0:1]) and torch.equal(p, e[1:2]) and torch.equal(n, e[2:3])
