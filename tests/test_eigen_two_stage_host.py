"""EigenGCN in stage two, without a GPU:

  1. the piece buffer: every section starts on 16 bytes, and ``pack_host`` -> ``piece_buffer`` -> ``unpack_piece`` returns every array,
     also for four pooling levels (more than the assembler's launch takes: the layout has no bound);
  2. the chunk assembler restated in numpy (tests/eigen_two_stage_util.py::assemble_numpy) on 1, 3 and 9 piece buffers gives the arrays
     ``eigen_pool.collate`` builds on the host for the same graphs (collate's only launch, ``row_maps``, is restated for CPU tensors);
  3. the library refuses bad descriptions before any launch; ``check_dict`` / ``chunk_shape`` raise ValueError for a dict prepared for
     another L / J / Jf, mixed Nmax, mixed feature widths;
  4. ``two_stage.embed_dataset`` unwraps an ``eigen_triplet.tripletnet`` and hands EigenGCN graphs to the EigenGCN call, never to the
     GraphSage call shape.
"""
import numpy as np
import pytest
import torch

import eigen_two_stage_util as U
import test_eigen_triplet_host as H


def _pieces(name, count, fin=6):
    from two_stage_gnn_amd import eigen_triplet as ET
    pool_sizes, J, Jf = U.config(name)
    results, dicts = U.graph_set(name, fin)
    out = []
    for d in dicts[:count]:
        packed = ET.pack_host(d, len(pool_sizes), J, Jf)
        rows = ET.padded_rows_host(d["feats"], packed["n"][0])
        buf, off = ET.piece_buffer(packed, rows, J)
        out.append((buf, off, packed, rows))
    return results[:count], out


# ------------------------------------------------------------------------------------------------ 1. the piece buffer
@pytest.mark.parametrize("name", sorted(U.CONFIGS) + sorted(U.DEEP))
def test_piece_sections_start_on_16_bytes_and_round_trip(name):
    from two_stage_gnn_amd import eigen_triplet as ET
    pool_sizes, J, Jf = U.config(name)
    L = len(pool_sizes)
    _, pieces = _pieces(name, 5)
    for buf, off, packed, rows in pieces:
        n, nnz = packed["n"], [int(c[1].size) for c in packed["graphs"]]
        assert buf.dtype == np.int32 and buf.size == off[-1] and off.size == 7 * (L + 1) - 1
        assert all(int(o) % 4 == 0 for o in off) and np.all(np.diff(off) >= 0)
        u = ET.unpack_piece(buf, n, nnz, J, Jf, rows.shape[1])
        for (rp, col, val), (rp0, col0, val0, _) in zip(u["graphs"], packed["graphs"]):
            assert np.array_equal(rp, rp0) and np.array_equal(col, col0) and np.array_equal(val, val0) and val.dtype == np.float32
        assert len(u["levels"]) == L
        for lv, lv0 in zip(u["levels"], packed["levels"]):
            for k in ("cluster_of", "coef", "bptr", "members"):
                assert np.array_equal(lv[k], lv0[k]) and lv[k].dtype == lv0[k].dtype, k
        assert (u["final"] is None) == (Jf == 0) and (Jf == 0 or np.array_equal(u["final"], packed["final"]))
        assert np.array_equal(u["feats"], rows) and rows.shape[1] % 4 == 0
    # the graph set holds what the assembler's tests need
    results, _ = U.graph_set(name)
    assert results[0]["graphs"][0].shape[0] == U.NMAX
    assert (pieces[U.UNASSIGNED][2]["levels"][0]["cluster_of"] == -1).sum() == 3 and pieces[U.UNASSIGNED][2]["levels"][0]["bptr"][1] == 3
    one = pieces[U.ONE_CLUSTER][2]
    assert one["n"][1] == 1 and one["graphs"][1][1].size == 0


def test_a_four_level_piece_becomes_a_one_graph_batch(monkeypatch):
    """more pooling levels than the assembler's launch takes: the piece buffer, its upload and the views the triplet step and the
    per-graph call read (``device_piece`` / ``to_device``) have no bound on L (on CPU tensors here, ``row_maps`` restated)"""
    from two_stage_gnn_amd import eigen_triplet as ET
    _row_maps_on_the_host(monkeypatch)
    (name, (pool_sizes, J, Jf)), = U.DEEP.items()
    L = len(pool_sizes)
    assert L > ET.max_levels()
    _, dicts = U.graph_set(name)
    for d in dicts[:4]:
        packed = ET.pack_host(d, L, J, Jf)
        eb, feats, copies = ET.to_device(packed, d["feats"], torch.device("cpu"))
        assert copies == 1 and len(eb.levels) == L and eb.final_coef.shape == (packed["n"][L], Jf)
        gs = [eb.g0] + [lv.g for lv in eb.levels]
        for g, (rp, col, val, _), n in zip(gs, packed["graphs"], packed["n"]):
            assert g.n_rows == n and g.nnz == col.size and np.array_equal(g.rowptr[:n + 1].numpy(), rp) and bool((g.rowptr[n:] == rp[-1]).all())
            assert g.rowptr.numel() == n + U.NMAX + 1 and np.array_equal(g.col[:g.nnz].numpy(), col) and np.array_equal(g.val[:g.nnz].numpy(), val)
        for lv, h in zip(eb.levels, packed["levels"]):
            for k in ("cluster_of", "coef", "bptr", "members"):
                assert np.array_equal(getattr(lv, k).numpy(), h[k]), k
        assert np.array_equal(feats.numpy(), ET.padded_rows_host(d["feats"], packed["n"][0]))


def test_layout_rejects_bad_sizes():
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    n, z, off = np.array([5, 2], np.int64), np.array([8, 2], np.int64), np.zeros(13, np.int64)
    call = lambda nlev, J, Jf, ldf, n_=n, z_=z: L.tsgnn_eigen_assemble_layout(nlev, J, Jf, ldf, n_.ctypes.data, z_.ctypes.data, off.ctypes.data)
    assert call(2, 2, 1, 8) == 0
    # rowptr 6 -> 8, col 8, val 8 | rowptr 3 -> 4, col 2 -> 4, val 4 | cluster_of 5 -> 8, coef 10 -> 12, bptr 4, members 5 -> 8 | final 2 -> 4 | x 40
    assert off.tolist() == [0, 8, 16, 24, 28, 32, 36, 44, 56, 60, 68, 72, 112]
    assert call(0, 2, 1, 8) == -1 and call(2, 0, 1, 8) == -1 and call(2, 6, 1, 8) == -1
    n5, z5, off5 = np.array([9, 5, 4, 3, 2], np.int64), np.array([20, 8, 6, 4, 2], np.int64), np.zeros(34, np.int64)
    assert L.tsgnn_eigen_assemble_layout(5, 1, 0, 8, n5.ctypes.data, z5.ctypes.data, off5.ctypes.data) == 0      # any number of levels
    assert off5[0] == 0 and np.all(np.diff(off5[:33]) >= 0) and off5[-1] == off5[-2] + 9 * 8 and all(int(o) % 4 == 0 for o in off5)
    assert call(2, 2, 5, 8) == -1 and call(2, 2, 1, 6) == -1 and call(2, 2, 1, 8, n_=np.array([5, -1], np.int64)) == -1
    assert L.tsgnn_eigen_assemble_layout(2, 2, 1, 8, None, z.ctypes.data, off.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------ 2. the assembler, restated
def _row_maps_on_the_host(monkeypatch):
    from two_stage_gnn_amd import graph as G

    def call(name, *args):
        assert name == "row_maps", name
        gp, B, R, row_graph, row_slot = args
        g = gp.numpy()
        for b in range(B):
            row_graph[g[b]:g[b + 1]] = b
            row_slot[g[b]:g[b + 1]] = torch.arange(int(g[b + 1] - g[b]), dtype=torch.int32)
    monkeypatch.setattr(G.nat, "call", call)


@pytest.mark.parametrize("count", [1, 3, 9])
@pytest.mark.parametrize("name", sorted(U.CONFIGS))
def test_numpy_assembler_equals_collate(name, count, monkeypatch):
    from two_stage_gnn_amd import eigen_pool as ep
    _row_maps_on_the_host(monkeypatch)
    pool_sizes, J, Jf = U.CONFIGS[name]
    results, pieces = _pieces(name, count)
    ldf = pieces[0][3].shape[1]
    got = U.assemble_numpy([(buf, packed["n"], [int(c[1].size) for c in packed["graphs"]]) for buf, _, packed, _ in pieces], U.NMAX, J, Jf, ldf)
    want = U.batch_arrays(ep.collate(results, U.NMAX, J, Jf, device=torch.device("cpu")))
    for k, w in want.items():
        if w is None:
            assert got[k] is None, k
            continue
        w = w.numpy()
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (k, got[k].dtype, w.dtype, got[k].shape, w.shape)
        assert np.array_equal(got[k], w), k
    x = got["x"]
    rows = np.concatenate([p[3] for p in pieces])
    assert np.array_equal(x[:rows.shape[0]], rows) and not x[rows.shape[0]:].any() and x.shape[0] == rows.shape[0] + U.NMAX


@pytest.mark.parametrize("name", sorted(U.CONFIGS))
def test_graph_set_reaches_every_destination_residue(name):
    """where the pieces' rowptr / col / members / bptr land in the chunk's arrays takes all four residues mod 4: every head / body /
    tail split of the assembler's copies occurs (the GPU test asserts the same on the pieces it assembles)"""
    for count in (32, 33):
        results, pieces = _pieces(name, count)
        nnz = np.array([[int(c[1].size) for c in p[2]["graphs"]] for p in pieces], dtype=np.int64)
        res = U.destination_residues(U.level_sizes(results), nnz)
        assert all(v == {0, 1, 2, 3} for v in res.values()), res


# ------------------------------------------------------------------------------------------------ 3. what is refused
def _desc(K=1, B=1, nlev=2, J=2, Jf=1, ldf=8, nmax=10, first=1, R=(6, 2), E=(10, 2), pieces=None):
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    hw, pw = L.tsgnn_eigen_assemble_header_words(), L.tsgnn_eigen_assemble_piece_words()
    P = 1 << 20                                                             # (pointers are only tested here, never followed)
    pieces = [(P, 0, 1, 6, 10, 0, 0, 2, 2, 0, 0)] if pieces is None else pieces
    d = np.zeros(hw + pw * max(len(pieces), 1), dtype=np.int64)
    d[0:8] = (K, B, nlev, J, Jf, ldf, nmax, first)
    d[9], d[10] = P, P
    for i in range(nlev):
        d[12 + 2 * i], d[13 + 2 * i] = R[i], E[i]
        d[20 + 7 * i:27 + 7 * i] = P
    for i in range(nlev - 1):
        d[48 + 4 * i:52 + 4 * i] = P
    for t, p in enumerate(pieces):
        d[hw + pw * t:hw + pw * t + len(p)] = p
    return d


def test_assemble_rejects_bad_descriptions_without_a_gpu():
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    assert (L.tsgnn_eigen_assemble_max_pieces(), L.tsgnn_eigen_assemble_max_levels()) == (32, 3)
    assert (L.tsgnn_eigen_assemble_header_words(), L.tsgnn_eigen_assemble_piece_words()) == (60, 19)
    P = 1 << 20
    call = lambda d: L.tsgnn_eigen_assemble_f32(d.ctypes.data, None)
    assert L.tsgnn_eigen_assemble_f32(None, None) == -1
    bad = [_desc(K=0), _desc(K=2), _desc(K=33, B=40), _desc(nlev=0), _desc(nlev=5, R=(6, 2, 2, 2, 2), E=(10, 2, 2, 2, 2)), _desc(J=0), _desc(J=6),
           _desc(Jf=5), _desc(ldf=6), _desc(ldf=0), _desc(nmax=0), _desc(first=2), _desc(R=(-1, 2)), _desc(E=(10, -2)),
           _desc(pieces=[(0, 0, 1, 6, 10, 0, 0, 2, 2, 0, 0)]),             # no buffer
           _desc(pieces=[(P + 4, 0, 1, 6, 10, 0, 0, 2, 2, 0, 0)]),         # a misaligned buffer
           _desc(pieces=[(P, 1, 1, 6, 10, 0, 0, 2, 2, 0, 0)]),             # graph number outside the batch
           _desc(pieces=[(P, 0, 2, 6, 10, 0, 0, 2, 2, 0, 0)]),             # last is a flag
           _desc(pieces=[(P, 0, 1, -6, 10, 0, 0, 2, 2, 0, 0)]),            # a negative size
           _desc(pieces=[(P, 0, 1, 11, 10, 0, 0, 2, 2, 0, 0)], R=(11, 2)), # more rows than Nmax
           _desc(pieces=[(P, 0, 1, 6, 10, 1, 0, 2, 2, 0, 0)]),             # leaves the rows of level 0
           _desc(pieces=[(P, 0, 1, 6, 10, 0, 0, 2, 2, 0, 1)]),             # leaves the entries of level 1
           _desc(pieces=[(P, 0, 1, 5, 10, 0, 0, 2, 2, 0, 0)]),             # closes the batch before its end
           _desc(pieces=[(P, 0, 0, 6, 10, 0, 0, 2, 3, 0, 0)])]
    for d in bad:
        assert call(d) == -1, d[:12]
    for at in (9, 10, 20, 23, 26, 27, 33, 48, 51):                         # a missing, then a misaligned output
        for v in (0, P + 8):
            d = _desc()
            d[at] = v
            assert call(d) == -1, at
    d = _desc(Jf=0)
    d[10], d[9] = 0, 0                                                      # (no final matrices: the final array may be absent; x may not)
    assert call(d) == -1


def test_dicts_and_chunks_that_disagree_raise():
    from two_stage_gnn_amd import eigen_triplet as ET
    _, dicts = U.graph_set("l1_j2_f1")
    d = dicts[3]
    ET.check_dict(d, 1, 2, 1)
    for L, J, Jf in ((2, 2, 1), (0, 2, 1), (1, 1, 1), (1, 3, 1), (1, 2, 0), (1, 2, 2)):
        with pytest.raises(ValueError):
            ET.check_dict(d, L, J, Jf)
    with pytest.raises(ValueError):
        ET.check_dict({k: v for k, v in d.items() if k != "num_nodes_1"}, 1, 2, 1)

    def part(**kw):
        e = ET._Graph()
        e.nmax, e.ldf, e.fin, e.L, e.J, e.Jf = 19, 8, 6, 1, 2, 1
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    assert ET.chunk_shape([part(), part()]) == (19, 8, 1, 2, 1)
    for kw in (dict(nmax=20), dict(fin=7), dict(ldf=12, fin=9), dict(L=2), dict(J=1), dict(Jf=0)):
        with pytest.raises(ValueError):
            ET.chunk_shape([part(), part(**kw)])


# ------------------------------------------------------------------------------------------------ 4. the route
def test_embed_dataset_unwraps_the_tripletnet_and_takes_the_eigen_call(monkeypatch):
    from two_stage_gnn_amd import eigen_encoders as EE, eigen_triplet as ET, two_stage as TS
    c = dict(J=2, Jf=1, con_final=1, mask=1, nmax=U.NMAX, num_layers=3, hidden=8, emb=8, label_dim=4, pred_hidden=[6], pool_sizes=[4])
    m = EE.WavePoolingGcnEncoder(c["nmax"], 6, c["hidden"], c["emb"], c["label_dim"], c["num_layers"], num_pool_matrix=2,
                                 num_pool_final_matrix=1, pool_sizes=[4], pred_hidden_dims=[6], args=H.args_of(c)).cpu()
    net = ET.tripletnet(m, H.args_of(c))
    _, dicts = U.graph_set("l1_j2_f1")
    objs = [U.GraphObj(d) for d in dicts[:4]]
    seen = []

    def fake(model, g, dev):
        seen.append((model, g))
        assert not model.training and model.per_graph_bn and not torch.is_grad_enabled()
        return torch.full((1, 4), float(len(seen)))
    monkeypatch.setattr(ET, "embed_one", fake)
    m.train()
    for model in (net, m):
        del seen[:]
        out = TS.embed_dataset(model, objs)                      # (a model on the CPU: one call per graph)
        assert [s[0] for s in seen] == [m] * 4 and [s[1] for s in seen] == objs
        assert out.shape == (4, 4) and out[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0] and m.training
    out = TS.embed_dataset(m, dicts[:2] + objs[:1])              # bare dicts are taken too
    assert out.shape == (3, 4) and seen[-3][1] is dicts[0]
    assert TS._labels(dicts[:4]).tolist() == [0, 1, 2, 0] and TS._labels(objs).tolist() == [0, 1, 2, 0]
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="GPU only"):           # the real call refuses a model on the CPU: no CPU path
        TS.embed_dataset(m, objs[:1])
