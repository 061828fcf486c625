"""EigenGCN in stage two, on the GPU (eigen_triplet.assemble / embed_chunk, csrc/eigen_assemble.hip, the route in two_stage):

  1. the assembler against ``eigen_pool.concat_batches`` of the same one-graph batches (and ``eigen_pool.collate`` of the same graphs):
     every array word for word, 1 / 3 / kmax / kmax + 1 pieces (the last crosses a launch group), four configurations, GUARD words behind every
     array intact; the graph set (tests/eigen_two_stage_util.py) has a full graph, unassigned rows, a one-node edge-less pooled graph
     and destination offsets of every residue mod 4;
  2. ``embed_dataset`` rows at chunk 1, 5 and the default against the per-graph call of the same model through the dense
     reference-signature forward and against the fp64 restatement (tests/eigen_ref.py), mask on / off, con_final 0 / 1, two levels;
  3. the reference's own ``evaluate()`` (tests/golden/two_stage_eval_eigen_*.npz, scripts/gen_golden_eigen_two_stage.py): embeddings,
     predictions for both sets, all five metrics; no query is undecided in these fixtures, none is skipped;
  4. the resident cache is shared with the triplet step in both directions, and a second call uploads nothing;
  5. ``evaluate_mlp`` through the family equals ``MLPProbe`` on ``embed_dataset``'s rows;
  6. four pooling levels, more than the assembler's launch takes: the triplet step and ``embed_dataset`` (one call per graph) give the
     B = 1 rows.

Bounds of 2 and 3: the rule of tests/test_gpu_eigen_triplet.py (``_check``): 1e-5 of the tensor's largest entry, or 10 x what the same
computation in fp32 on the CPU itself misses fp64 by; both figures are printed."""
import os

import numpy as np
import pytest
import torch

import eigen_ref as ER
import eigen_two_stage_util as U
import test_eigen_triplet_host as H
import test_gpu_eigen_triplet as G

pytestmark = pytest.mark.gpu

FIN = 6


def _cfg(name, mask=1, con_final=1):
    pool_sizes, J, Jf = U.config(name)
    return dict(J=J, Jf=Jf, con_final=con_final, mask=mask, nmax=U.NMAX, num_layers=3, hidden=12, emb=12, label_dim=5, pred_hidden=[7],
                pool_sizes=list(pool_sizes))


def _seeded_model(c, fin=FIN, seed=23):
    m = G._model(c, fin)
    m.load_state_dict(G.seeded_state(m, seed))
    return m


# ------------------------------------------------------------------------------------------------ 1. the assembler
def _kmax():
    from two_stage_gnn_amd import _native as nat
    return int(nat.lib().tsgnn_eigen_assemble_max_pieces())


@pytest.mark.parametrize("count", ["1", "3", "kmax", "kmax+1"])
@pytest.mark.parametrize("name", sorted(U.CONFIGS))
def test_assembler_equals_concat_batches(name, count):
    from two_stage_gnn_amd import eigen_pool as ep, eigen_triplet as ET, resident as R
    dev = torch.device("cuda", torch.cuda.current_device())
    pool_sizes, J, Jf = U.CONFIGS[name]
    L = len(pool_sizes)
    count = {"1": 1, "3": 3, "kmax": _kmax(), "kmax+1": _kmax() + 1}[count]
    results, dicts = U.graph_set(name, FIN)
    assert count <= len(dicts)
    cache = R.ResidentCache()
    parts = [ET.resident_graph(U.GraphObj(d), dev, cache, L, J, Jf, check=True) for d in dicts[:count]]
    if count >= 9:                                    # the set the copies' head / body / tail splits are exercised on
        n, nnz = np.array([p.sizes for p in parts]), np.array([p.nnz for p in parts])
        assert n[0, 0] == U.NMAX and n[U.ONE_CLUSTER, 1] == 1 and nnz[U.ONE_CLUSTER, 1] == 0
        res = U.destination_residues(n, nnz)
        assert all(v == {0, 1, 2, 3} for v in res.values()), res
    x, eb = ET.assemble(parts, dev, guard=8)
    got = U.batch_arrays(eb, x)
    ref = ep.concat_batches([p.eb for p in parts])
    want = U.batch_arrays(ref, torch.cat([p.feats for p in parts] + [torch.zeros(U.NMAX, parts[0].ldf, device=dev)]))
    coll = U.batch_arrays(ep.collate(results[:count], U.NMAX, J, Jf, device=dev))
    if count > U.UNASSIGNED:
        c = got["cluster_of_0"][int(eb.g0.graph_ptr[U.UNASSIGNED]):int(eb.g0.graph_ptr[U.UNASSIGNED + 1])]
        assert int((c == -1).sum()) == 3                                       # unassigned rows keep their -1
    for k, w in want.items():
        if w is None:
            assert got[k] is None and coll[k] is None, k
            continue
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (k, got[k].dtype, w.dtype, tuple(got[k].shape), tuple(w.shape))
        assert torch.equal(got[k], w), k
        if k in coll:
            assert torch.equal(got[k], coll[k]), k + " (collate)"
    gs_got, gs_ref = [eb.g0] + [lv.g for lv in eb.levels], [ref.g0] + [lv.g for lv in ref.levels]
    for a, b in zip(gs_got, gs_ref):
        assert (a.B, a.nmax, a.n_rows, a.n_ghost, a.nnz, a.symmetric, a.layout) == (b.B, b.nmax, b.n_rows, b.n_ghost, b.nnz, b.symmetric, b.layout)
        assert np.array_equal(np.asarray(a.sizes), np.asarray(b.sizes))
    # every word behind every array (the guard and the padding up to the next array) is untouched
    ibuf, fbuf, ioff, isz, foff, fsz = eb._raw
    for buf, off, sz in ((ibuf, ioff, isz), (fbuf.view(torch.int32), foff, fsz)):
        for j, s in enumerate(sz):
            tail = buf[int(off[j]) + s:int(off[j + 1])]
            assert tail.numel() >= 8 and bool((tail == ET.GUARD).all()), (j, s)


# ------------------------------------------------------------------------------------------------ 2. embeddings vs per-graph calls
_refs = {}


def _restatements(key, m, dicts, c):
    """fp64 and fp32 CPU restatement rows of every graph at B = 1: computed once per case, shared, never written"""
    if key not in _refs:
        out = []
        for dt in (torch.float64, torch.float32):
            p = H._ref_params({k: v.detach().cpu().to(dt) for k, v in m.state_dict().items()})
            rows = []
            with torch.no_grad():
                for d in dicts:
                    x, adj, pooled, n0, nl, pm = H.dense_inputs(d, c, dt)
                    rows.append(ER.wave_pooling_forward(p, x, adj, pooled, n0, nl, pm, c["num_layers"], c["pool_sizes"], c["J"], c["Jf"],
                                                        concat=True, mask=c["mask"], con_final=c["con_final"],
                                                        n_linear=len(c["pred_hidden"]) + 1))
            out.append(torch.cat(rows))
        _refs[key] = out
    return _refs[key]


def _dense_rows(m, dicts, c):
    """the per-graph call of the same model through the dense reference-signature forward (``batch_from_dense`` at B = 1), eval mode"""
    rows = []
    f = lambda t: t.cuda()
    training = m.training
    m.eval()
    with torch.no_grad():
        for d in dicts:
            x, adj, pooled, n0, nl, pm = H.dense_inputs(d, c, torch.float32)
            rows.append(m(f(x), f(adj), [f(a) for a in pooled], n0, nl, {i: [f(t) for t in v] for i, v in pm.items()}))
    m.train(training)
    return torch.cat(rows)


EMBED_CASES = [("l1_j2_f1", 1, 1), ("l1_j2_f1", 0, 1), ("l1_j2_f1", 1, 0), ("l1_j2_f1", 0, 0), ("l2_j1", 1, 1), ("l1_j2_f2", 0, 1), ("l1_j1", 1, 1)]


@pytest.mark.parametrize("name,mask,con_final", EMBED_CASES)
def test_embed_dataset_rows_are_the_single_graph_forwards(name, mask, con_final):
    from two_stage_gnn_amd import eigen_triplet as ET, two_stage as TS
    c = _cfg(name, mask, con_final)
    m = _seeded_model(c)
    _, dicts = U.graph_set(name, FIN)
    dicts = dicts[:11]                               # the full graph, the unassigned rows and the one-node pooled graph are among them
    objs = [U.GraphObj(d) for d in dicts]
    r64, r32 = _restatements((name, mask, con_final), m, dicts, c)
    dense = _dense_rows(m, dicts, c)
    tag = "%s mask=%d con_final=%d " % (name, mask, con_final)
    G._check(tag + "dense B=1 rows", dense, r64, r32, 1e-5)
    net = ET.tripletnet(m, H.args_of(c))
    m.train()
    for chunk, model in ((1, m), (5, net), (None, net)):
        rows = TS.embed_dataset(model, objs, chunk)
        assert rows.shape == (len(objs), c["label_dim"]) and rows.dtype == torch.float32 and not rows.requires_grad and m.training
        G._check(tag + "chunk=%s vs fp64" % chunk, rows, r64, r32, 1e-5)
        G._check(tag + "chunk=%s vs dense" % chunk, rows, r64, r32, 1e-5, against=dense)
    assert ET.DEFAULT_CHUNK >= len(objs)             # (the default took all eleven graphs as one chunk)
    bare = TS.embed_dataset(m, dicts, 4)             # bare dicts: packed at every call, same rows
    assert torch.equal(bare, TS.embed_dataset(m, objs, 4))


def test_cache_off_takes_the_per_graph_call(monkeypatch):
    from two_stage_gnn_amd import eigen_triplet as ET, resident as R, two_stage as TS
    c = _cfg("l1_j2_f1")
    m = _seeded_model(c)
    _, dicts = U.graph_set("l1_j2_f1", FIN)
    objs = [U.GraphObj(d) for d in dicts[:6]]
    r64, r32 = _restatements(("l1_j2_f1", 1, 1), m, dicts[:11], c)
    on = TS.embed_dataset(m, objs)
    monkeypatch.setattr(R, "RESIDENT", False)
    calls = []
    real = ET.embed_one
    monkeypatch.setattr(ET, "embed_one", lambda *a: calls.append(1) or real(*a))
    before = len(R.resident_cache(m))
    off = TS.embed_dataset(m, objs)
    assert len(calls) == len(objs) and len(R.resident_cache(m)) == before
    G._check("cache off vs fp64", off, r64[:6], r32[:6], 1e-5)
    G._check("cache off vs chunked", off, r64[:6], r32[:6], 1e-5, against=on)


def test_chunks_that_disagree_raise():
    from two_stage_gnn_amd import two_stage as TS
    c = _cfg("l1_j2_f1")
    m = _seeded_model(c)
    _, dicts = U.graph_set("l1_j2_f1", FIN)
    _, wider = U.graph_set("l1_j2_f1", FIN + 1)
    _, bigger = U.graph_set("l1_j2_f1", FIN, sizes=U.SIZES[:4], nmax=U.NMAX + 1)
    _, other = U.graph_set("l1_j2_f2", FIN)
    for bad in (wider[1], bigger[1], other[1], {k: v for k, v in dicts[1].items() if k != "pool_adj_0_1"}):
        with pytest.raises(ValueError):
            TS.embed_dataset(m, [U.GraphObj(dicts[0]), U.GraphObj(bad)])


# ------------------------------------------------------------------------------------------------ 3. the reference's evaluate()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EVAL_NAMES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("two_stage_eval_eigen_") and f.endswith(".npz"))


def _eval_fixture(name):
    g = H.load(name)
    c = dict(J=int(g["J"]), Jf=int(g["Jf"]), con_final=int(g["con_final"]), mask=int(g["mask"]), nmax=int(g["nmax"]),
             num_layers=int(g["num_layers"]), hidden=int(g["hidden"]), emb=int(g["emb"]), label_dim=int(g["label_dim"]),
             pred_hidden=[int(v) for v in g["pred_hidden"]], pool_sizes=[int(v) for v in g["pool_sizes"]])
    keys = [k[2:] for k in g if k.startswith("d.")]
    dicts = [{k: (int(g["d." + k][b]) if g["d." + k].ndim == 1 else np.asarray(g["d." + k][b], dtype=np.float32)) for k in keys}
             for b in range(g["d.adj"].shape[0])]
    return g, c, dicts


def test_fixture_list():
    assert len(EVAL_NAMES) >= 2
    cs = [_eval_fixture(n)[1] for n in EVAL_NAMES]
    assert any(len(c["pool_sizes"]) == 2 for c in cs) and any(c["Jf"] > 0 for c in cs)


@pytest.mark.parametrize("name", EVAL_NAMES)
def test_evaluate_matches_the_reference(name):
    from two_stage_gnn_amd import eigen_triplet as ET, two_stage as TS
    g, c, dicts = _eval_fixture(name)
    fin = dicts[0]["feats"].shape[1]
    m = G._model(c, fin)
    m.load_state_dict({k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    n_train, k = int(g["n_train"]), int(g["k"])
    objs = [U.GraphObj(d) for d in dicts]
    net = ET.tripletnet(m, H.args_of(c))
    r64, r32 = _restatements(name, m, dicts, c)
    ref = torch.tensor(g["embed"])
    G._check(name + " restatement vs the reference", ref, r64, r32, 1e-5)
    emb = TS.embed_dataset(net, objs)
    G._check(name + " embeddings vs fp64", emb, r64, r32, 1e-5)
    G._check(name + " embeddings vs the reference", emb, r64, r32, 1e-5, against=ref)
    y = np.array([d["label"] for d in dicts])
    knn = TS.KNeighborsClassifier(k).fit(emb[:n_train], y[:n_train])
    assert np.array_equal(knn.predict(emb[n_train:].cpu().numpy()), g["pred_val"])           # no query skipped: none is undecided
    assert np.array_equal(knn.predict(emb[:n_train].cpu().numpy()), g["pred_train"])
    result = TS.evaluate(objs[:n_train], objs[n_train:], net, n_neighbors=k)
    want = dict(zip([str(s) for s in g["metric_names"]], g["metrics"].tolist()))
    assert sorted(result) == sorted(want) == ["F1", "acc", "prec", "recall", "train acc"]
    for key, v in want.items():
        assert abs(result[key] - v) <= 1e-12, (key, result[key], v)


# ------------------------------------------------------------------------------------------------ 4. the cache
def test_cache_is_shared_with_the_triplet_step_both_ways():
    from two_stage_gnn_amd import eigen_triplet as ET, two_stage as TS
    c = _cfg("l1_j2_f1")
    m = _seeded_model(c).eval()
    _, dicts = U.graph_set("l1_j2_f1", FIN)
    objs = [U.GraphObj(d) for d in dicts[:9]]
    net = ET.tripletnet(m, H.args_of(c))
    cc = net.cache
    with torch.no_grad():
        first = net(objs[0], objs[4], objs[7])
    assert cc.h2d == 3 and len(cc) == 3
    rows = TS.embed_dataset(net, objs)
    assert cc.h2d == 3 + 6 and len(cc) == 9           # the triplet's three graphs were not uploaded again, the other six once
    again = TS.embed_dataset(m, objs, 4)
    assert cc.h2d == 9 and len(cc) == 9               # a second call uploads nothing at all
    with torch.no_grad():
        step = net(objs[1], objs[2], objs[3])         # graphs only stage two has seen: the triplet step uploads nothing
        same = net(objs[0], objs[4], objs[7])
    assert cc.h2d == 9 and len(cc) == 9
    assert all(torch.equal(a, b) for a, b in zip(first, same))
    r64, r32 = _restatements(("l1_j2_f1", 1, 1), m, dicts[:11], c)
    G._check("rows after a triplet step", rows, r64[:9], r32[:9], 1e-5)
    G._check("rows, second call", again, r64[:9], r32[:9], 1e-5, against=rows)
    for b, e in ((1, step[2]), (2, step[3]), (3, step[4]), (0, first[2])):
        G._check("triplet embedding of graph %d" % b, e, r64[b:b + 1], r32[b:b + 1], 1e-5, against=rows[b:b + 1])


# ------------------------------------------------------------------------------------------------ 5. the MLP probe
def test_evaluate_mlp_through_the_family():
    from two_stage_gnn_amd import eigen_triplet as ET, two_stage as TS
    c = _cfg("l1_j2_f1")
    m = _seeded_model(c)
    _, dicts = U.graph_set("l1_j2_f1", FIN)
    objs = [U.GraphObj(d) for d in dicts]
    train, val = objs[:22], objs[22:]
    net = ET.tripletnet(m, H.args_of(c))
    torch.manual_seed(5)
    got = TS.evaluate_mlp(train, val, net, hidden=(16, 8))
    emb = TS.embed_dataset(net, objs)
    y = np.array([d["label"] for d in dicts])
    torch.manual_seed(5)
    probe = TS.MLPProbe((16, 8)).fit(emb[:22], y[:22])
    assert got == {"acc": probe.score(emb[22:], y[22:])} and 0.0 <= got["acc"] <= 1.0
    kept = TS.MLPProbe((16, 8))
    torch.manual_seed(5)
    TS.evaluate_mlp(train, val, m, hidden=(16, 8), probe=kept)           # the bare encoder, the probe handed in
    assert torch.equal(kept._flat, probe._flat) and torch.equal(kept.losses_, probe.losses_)


# ------------------------------------------------------------------------------------------------ 6. more levels than the launch takes
def test_four_pooling_levels_take_the_per_graph_route(monkeypatch):
    from two_stage_gnn_amd import eigen_triplet as ET, two_stage as TS
    (name, (pool_sizes, J, Jf)), = U.DEEP.items()
    assert len(pool_sizes) > ET.max_levels()
    c = _cfg(name)
    m = _seeded_model(c)
    _, dicts = U.graph_set(name, FIN)
    dicts = dicts[:6]
    objs = [U.GraphObj(d) for d in dicts]
    r64, r32 = _restatements((name, 1, 1), m, dicts, c)
    dense = _dense_rows(m, dicts, c)
    G._check(name + " dense B=1 rows", dense, r64, r32, 1e-5)
    net = ET.tripletnet(m, H.args_of(c))
    calls = []
    real = ET.embed_one
    monkeypatch.setattr(ET, "embed_one", lambda *a: calls.append(1) or real(*a))
    for model, graphs in ((net, objs), (m, dicts)):
        del calls[:]
        rows = TS.embed_dataset(model, graphs)
        assert len(calls) == len(graphs) and rows.shape == (len(graphs), c["label_dim"])
        G._check(name + " embed_dataset vs fp64", rows, r64, r32, 1e-5)
        G._check(name + " embed_dataset vs dense", rows, r64, r32, 1e-5, against=dense)
    m.eval()
    with torch.no_grad():
        dp, dn, ea, e_p, en = net(objs[0], objs[1], objs[3])                 # the triplet step: concat_batches of views of the pieces
    assert net.cache.h2d == 3
    for b, e in ((0, ea), (1, e_p), (3, en)):
        G._check(name + " triplet embedding of graph %d" % b, e, r64[b:b + 1], r32[b:b + 1], 1e-5, against=dense[b:b + 1])
    dev = next(m.parameters()).device
    with pytest.raises(ValueError):                                          # the assembler itself says no, before any launch
        ET.assemble([ET.resident_graph(o, dev, net.cache, len(pool_sizes), J, Jf) for o in objs[:2]], dev)
