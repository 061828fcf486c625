"""gat_triplet without a GPU: ``pack_host`` against a plain numpy construction and its defining properties, the reference fixtures
tests/golden/triplet_gat_*.npz against the CPU oracle, and the assembler's host-side validator."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, params_of
from oracle import dense_ref as R

NMAX = 8
FIXTURES = ["triplet_gat_output_dim", "triplet_gat_classes"]


class GraphObj:
    """stands for the networkx graph object whose ``.graph`` dict the drop-ins read"""

    def __init__(self, adj, feats, n, label=0):
        self.graph = {"adj": adj, "feats": feats, "num_nodes": n, "assign_feats": feats, "label": label}


def make_obj(seed, n, nmax=NMAX, fin=3, kind="sym", pad_value=0.0):
    rng = np.random.default_rng(seed)
    a = np.zeros((nmax, nmax), dtype=np.float64)
    if kind != "empty" and n > 1:
        u = (rng.random((n, n)) < 0.35).astype(np.float64)
        np.fill_diagonal(u, 0.0)
        if kind == "sym":
            u = np.maximum(np.triu(u, 1), np.triu(u, 1).T)
        elif kind == "weighted":
            u = np.maximum(np.triu(u, 1), np.triu(u, 1).T) * (0.25 + rng.random((n, n)))
        a[:n, :n] = u                                                  # "directed": u as drawn, asymmetric
    f = np.full((nmax, fin), pad_value, dtype=np.float32)
    f[:n] = rng.standard_normal((n, fin)).astype(np.float32)
    return GraphObj(a, f, n)


def plain(obj):
    """the piece written out entry by entry: lists of (row, col) in CSR order and in transposed order"""
    a, n = np.asarray(obj.graph["adj"]), int(obj.graph["num_nodes"])
    nmax = a.shape[0]
    nr = n + (n < nmax)
    ent = [(i, j) for i in range(n) for j in range(n) if a[i, j] > 0]
    ent_t = sorted(range(len(ent)), key=lambda e: (ent[e][1], ent[e][0]))
    rowptr = [0] + [sum(1 for (i, _) in ent if i <= r) for r in range(nr)]
    rowptr_t = [0] + [sum(1 for (_, j) in ent if j <= c) for c in range(nr)]
    iso = [c for c in range(nr) if not any(j == c for (_, j) in ent)]
    return nr, ent, ent_t, rowptr, rowptr_t, iso


CASES = [(0, "sym"), (1, "sym"), (5, "sym"), (NMAX, "sym"), (5, "directed"), (6, "empty"), (5, "weighted"), (NMAX, "directed")]


@pytest.mark.parametrize("n,kind", CASES)
def test_pack_host_against_a_plain_construction(n, kind):
    from two_stage_gnn_amd import gat_triplet as GT
    obj = make_obj(10 * n + len(kind), n, kind=kind)
    p = GT.pack_host(obj)
    nr, ent, ent_t, rowptr, rowptr_t, iso = plain(obj)
    nnz = len(ent)
    assert (p["n"], p["nmax"], p["nr"], p["nnz"], p["mult"], p["k"]) == (n, NMAX, nr, nnz, NMAX - n, len(iso))
    assert p["rowptr"].dtype == np.int32 and p["rowptr"].tolist() == rowptr
    assert p["col"].tolist() == [j for (_, j) in ent]
    assert p["rowptr_t"].tolist() == rowptr_t
    assert p["col_t"].tolist() == [ent[e][0] for e in ent_t] and p["src_e_t"].tolist() == ent_t
    # the defining properties, stated on the arrays themselves
    src = p["src_e_t"]
    assert sorted(src.tolist()) == list(range(nnz))                                            # a permutation
    row_of_t = np.repeat(np.arange(nr), np.diff(p["rowptr_t"]))
    assert np.array_equal(p["col"][src], row_of_t)                                             # col[src_e_t[q]] = the transposed row of q
    row_of = np.repeat(np.arange(nr), np.diff(p["rowptr"]))
    assert np.array_equal(p["col_t"], row_of[src])                                             # its column there = the source row
    for c in range(nr):
        seg = p["col_t"][p["rowptr_t"][c]:p["rowptr_t"][c + 1]]
        assert (np.diff(seg) > 0).all()                                                        # ascending by source row
    assert np.array_equal(p["inv_e_t"][src], np.arange(nnz)) and np.array_equal(src[p["inv_e_t"]], np.arange(nnz))
    assert p["iso_rows"].tolist() == iso
    assert p["iso_w"].tolist() == [float(NMAX - n) if c == n else 1.0 for c in iso]             # 1 for real columns, Nmax - n for the representative
    if n < NMAX:
        assert p["rowptr"][n] == p["rowptr"][n + 1] == nnz and iso[-1] == n                    # the representative: no edges, listed
    f = np.asarray(obj.graph["feats"])
    assert p["feats"].shape == (nr, 4) and p["fin"] == 3 and p["feats"].dtype == np.float32
    assert np.array_equal(p["feats"][:, :3], f[:nr]) and (p["feats"][:, 3:] == 0).all()
    assert p["exact"]


def test_weights_are_a_mask():
    """weighted entries count as present, entries <= 0 as absent (encoders_GAT.py:40: ``adj > 0``)"""
    from two_stage_gnn_amd import gat_triplet as GT
    obj = make_obj(3, 5, kind="weighted")
    a = obj.graph["adj"].copy()
    a[0, 1], a[1, 0] = -2.0, 0.5
    ones = GraphObj((a > 0).astype(np.float64), obj.graph["feats"], 5)
    p, q = GT.pack_host(GraphObj(a, obj.graph["feats"], 5)), GT.pack_host(ones)
    for k in ("rowptr", "col", "rowptr_t", "col_t", "src_e_t", "inv_e_t", "iso_rows", "iso_w"):
        assert np.array_equal(p[k], q[k]), k
    assert (0, 1) not in list(zip(np.repeat(np.arange(6), np.diff(p["rowptr"])).tolist(), p["col"].tolist()))


def test_padded_rows_that_differ_take_the_fallback():
    from two_stage_gnn_amd import gat_triplet as GT
    obj = make_obj(4, 5)
    assert GT.pack_host(obj)["exact"]
    same = make_obj(4, 5, pad_value=0.75)                      # identical non-zero padded rows: one representative stands for them
    p = GT.pack_host(same)
    assert p["exact"] and (p["feats"][5, :3] == 0.75).all()
    obj.graph["feats"][7, 1] = 0.5
    assert not GT.pack_host(obj)["exact"]
    last = make_obj(5, NMAX - 1)
    last.graph["feats"][NMAX - 1, 0] = 3.0                     # a single padded row is its own representative
    assert GT.pack_host(last)["exact"]
    edge = make_obj(4, 5)
    edge.graph["adj"][6, 2] = 1.0                              # an edge of a padded row: the dense reference would use it
    assert not GT.pack_host(edge)["exact"]
    edge.graph["adj"][6, 2] = -1.0                             # (not an edge: ``adj > 0``)
    assert GT.pack_host(edge)["exact"]


def test_pack_host_rejects_bad_graphs():
    from two_stage_gnn_amd import gat_triplet as GT
    f = np.zeros((NMAX, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        GT.pack_host(GraphObj(np.zeros((NMAX, NMAX + 1)), f, 3))
    with pytest.raises(ValueError):
        GT.pack_host(GraphObj(np.zeros((NMAX, NMAX)), f, NMAX + 1))
    with pytest.raises(ValueError):
        GT.pack_host(GraphObj(np.zeros((NMAX, NMAX)), f, -1))


def test_piece_buffer_sections_start_on_16_bytes():
    from two_stage_gnn_amd import _native as nat, gat_triplet as GT
    p = GT.pack_host(make_obj(7, 5))
    buf = GT.piece_buffer(p)
    off = np.zeros(10, dtype=np.int64)
    assert nat.lib().tsgnn_gat_assemble_layout(p["nr"], p["nnz"], p["k"], 4, off.ctypes.data) == 0
    assert all(int(o) % 4 == 0 for o in off) and buf.size == off[9] and buf.dtype == np.int32
    parts = [p["rowptr"], p["rowptr_t"], p["col"], p["col_t"], p["src_e_t"], p["inv_e_t"], p["iso_rows"], p["iso_w"].view(np.int32),
             p["feats"].reshape(-1).view(np.int32)]
    for k, part in enumerate(parts):
        assert off[k] + part.size <= off[k + 1] and np.array_equal(buf[off[k]:off[k] + part.size], part)


# ------------------------------------------------------------------------------------------------ the fixtures, on the CPU
def triplets(g):
    """[(three (adj, feats, n)), ...] of a fixture"""
    return [[(g["t%d.g%d.adj" % (t, j)], g["t%d.g%d.feats" % (t, j)], int(g["t%d.g%d.num_nodes" % (t, j)])) for j in range(3)]
            for t in range(int(g["n_triplets"]))]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_hold_together_on_the_cpu(name):
    """oracle.dense_ref.gat_encoder at B = 1 per graph + F.pairwise_distance + the margin loss reproduce the stored outputs and
    gradients at the tolerances of tests/test_oracle_golden.py::test_gat_encoder, and every stored hinge is active"""
    g = load_golden(name)
    assert int(g["n_triplets"]) == 4 and int(g["nmax"]) == 16 and g["heads"].tolist() == [2, 2]
    sizes = [n for trip in triplets(g) for (_, _, n) in trip]
    assert 16 in sizes                                                                        # a graph without a padded row
    assert any(n > 1 and ((a[:n, :n] > 0).sum(0) == 0).any() for trip in triplets(g) for (a, _, n) in trip)    # an isolated real node
    for t, trip in enumerate(triplets(g)):
        p = params_of(g, requires_grad=True)
        e = [R.gat_encoder(p, torch.tensor(f)[None], torch.tensor(a)[None], final_dim=str(g["final_dim"]))[1] for (a, f, _) in trip]
        dp, dn = F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2)
        loss = torch.nn.MarginRankingLoss(margin=float(g["margin"]))(dp, dn, torch.full_like(dp, -1.0))
        assert float(g["t%d.loss" % t]) > 0
        np.testing.assert_allclose(dp.detach().numpy(), g["t%d.dist_p" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(dn.detach().numpy(), g["t%d.dist_n" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(torch.cat(e).detach().numpy(), g["t%d.embed" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(float(loss.detach()), float(g["t%d.loss" % t]), rtol=1e-4, atol=1e-5)
        loss.backward()
        for k, q in p.items():
            ref = g["t%d.g.%s" % (t, k)]
            got = q.grad.numpy() if q.grad is not None else np.zeros_like(ref)
            np.testing.assert_allclose(got, ref, err_msg="%d %s" % (t, k), rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------------------ the assembler's validator
def _desc(K=1, R=6, E=10, I=2, B=1, ldf=4, pieces=None):
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    hw, pw = L.tsgnn_gat_assemble_header_words(), L.tsgnn_gat_assemble_piece_words()
    P = 1 << 20                                                                               # (pointers are only tested here, never followed)
    d = np.zeros(hw + pw * 8, dtype=np.int64)
    d[0:7] = (K, R, E, I, B, ldf, 1)
    d[7] = 2
    d[11:25] = P
    d[25] = P
    if pieces is None:                                                                        # (buffer, n, nr, nnz, k, mult, row0, e0, i0, graph, last)
        pieces = [(P, 5, 6, 10, 2, 3, 0, 0, 0, 0, 1)]
    for j, q in enumerate(pieces):
        d[hw + pw * j:hw + pw * (j + 1)] = q
    return d


def test_assemble_rejects_bad_descriptions_without_a_gpu():
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    assert L.tsgnn_gat_assemble_max_pieces() == 8
    P = 1 << 20
    call = lambda d: L.tsgnn_gat_assemble_f32(d.ctypes.data, None)
    assert L.tsgnn_gat_assemble_f32(None, None) == -1
    assert call(_desc(K=0)) == -1 and call(_desc(K=9)) == -1                                   # K outside 1..8
    assert call(_desc(pieces=[(P, 5, 6, -1, 2, 3, 0, 0, 0, 0, 1)])) == -1                      # a negative size
    assert call(_desc(pieces=[(P, -5, 6, 10, 2, 3, 0, 0, 0, 0, 1)])) == -1
    assert call(_desc(R=-1)) == -1 and call(_desc(E=-1)) == -1
    big = 1 << 31
    assert call(_desc(R=big + 6, pieces=[(P, 5, 6, 10, 2, 3, big, 0, 0, 0, 1)])) == -1         # a row offset past 2^31
    assert call(_desc(E=big + 10, pieces=[(P, 5, 6, 10, 2, 3, 0, big, 0, 0, 1)])) == -1        # an entry offset past 2^31
    assert call(_desc(pieces=[(P, 5, 6, 10, 2, 3, 1, 0, 0, 0, 0)])) == -1                      # a piece that leaves the batch's rows
    assert call(_desc(pieces=[(P, 5, 6, 10, 2, 3, 0, 1, 0, 0, 0)])) == -1                      # ... its entries
    assert call(_desc(pieces=[(P, 5, 6, 10, 2, 3, 0, 0, 1, 0, 0)])) == -1                      # ... its listed columns
    assert call(_desc(pieces=[(P, 5, 6, 10, 2, 3, 0, 0, 0, 1, 0)])) == -1                      # ... its graphs
    assert call(_desc(pieces=[(0, 5, 6, 10, 2, 3, 0, 0, 0, 0, 1)])) == -1                      # no buffer
    assert call(_desc(pieces=[(P + 4, 5, 6, 10, 2, 3, 0, 0, 0, 0, 1)])) == -1                  # a buffer off 16 bytes
    assert call(_desc(pieces=[(P, 5, 7, 10, 2, 3, 0, 0, 0, 0, 1)])) == -1                      # more than one representative
    assert call(_desc(ldf=6)) == -1                                                            # rows off 16 bytes
    d = _desc()
    d[13] = 0
    assert call(d) == -1                                                                       # a missing output
    off = np.zeros(10, dtype=np.int64)
    assert L.tsgnn_gat_assemble_layout(-1, 0, 0, 4, off.ctypes.data) == -1 and L.tsgnn_gat_assemble_layout(3, 2, 1, 4, None) == -1
    assert L.tsgnn_gat_assemble_layout(3, 2, 1, 6, off.ctypes.data) == -1
