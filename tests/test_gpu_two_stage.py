"""Stage two on the GPU: the k-nearest-neighbour kernel (csrc/knn.hip) against the fp64 brute force of tests/knn_oracle.py (pinned to
sklearn by tests/test_two_stage_host.py), ``two_stage.embed_dataset`` against per-graph B = 1 eval forwards of the fp64 oracles, and
``two_stage.evaluate`` against the reference's own evaluate() (tests/golden/two_stage_eval_*.npz, scripts/gen_golden_knn.py).

The undecided rule (every prediction check below): a query is undecided when the training rows whose fp64 distance lies within a band
of the k-th distance d_k carry more than one label — swapping rows inside the band could change the vote.  The band is tau(D) d_k,
tau(D) = (D + 2) 2^-22 (twice the worst-case rounding of a sequential fp32 sum of D squared differences and a square root).  Every
other query must get the oracle's prediction exactly and the oracle's neighbour set; undecided queries may be at most 2 % of a case
(asserted, never skipped)."""
import numpy as np
import pytest
import torch

import knn_oracle as KO
from conftest import load_golden
from oracle import dense_ref as R
from oracle import pyg_ref as P
from util_graphs import dense_batch

pytestmark = pytest.mark.gpu

CASES = [(0, 1051, 117, 64, 2, 0), (1, 1051, 117, 20, 2, 0), (2, 1000, 168, 128, 6, 0), (3, 1051, 117, 64, 2, 100), (4, 37, 5, 8, 3, 0),
         (5, 1051, 117, 384, 2, 0), (6, 4096, 512, 512, 4, 0)]
KS = (1, 3, 5, 16)
CAP = 0.02


def _check_against_oracle(X, y, Q, k, d, pred, idx, dist, band, tag):
    """pred / idx / dist of the code under test (numpy: class labels, [nq, k], [nq, k]) against the fp64 oracle under the undecided
    rule; d = fp64 distances [nq, n_train].  Prints its figures before it asserts"""
    want, want_idx, want_dist = KO.brute_force(X, y, Q, k, d=d)
    und = KO.undecided(d, y, k, band)
    rel = np.abs(np.sort(dist.astype(np.float64), axis=1) - want_dist) / np.maximum(want_dist, 1e-300)
    rel = np.where(want_dist == 0, np.abs(dist), rel)
    same_set = (np.sort(idx, axis=1) == np.sort(want_idx, axis=1)).all(axis=1)
    print("%s: undecided %d / %d, max rel distance error %.3g (tau %.3g), wrong pred %d, wrong set %d (decided only: %d, %d)"
          % (tag, und.sum(), und.size, rel.max(), KO.tau(X.shape[1]), (pred != want).sum(), (~same_set).sum(),
             ((pred != want) & ~und).sum(), (~same_set & ~und).sum()))
    assert und.mean() <= CAP, (tag, und.sum(), und.size)
    assert (np.diff(dist, axis=1) >= 0).all(), tag                            # neighbours ascend
    assert ((pred == want) | und).all(), tag
    assert (same_set | und).all(), tag
    return rel.max(), und


@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%d_n%d_q%d_D%d_C%d_off%d" % c)
def test_knn_kernel_against_fp64_brute_force(case):
    from two_stage_gnn_amd import _native as nat, two_stage as TS
    seed, n_train, n_query, D, C, offset = case
    X, y, Q, yq = KO.synthetic(seed, n_train, n_query, D, C, offset)
    Xd = torch.from_numpy(X).cuda()
    for qname, Qh, yqh in (("val", Q, yq), ("train", X, y)):
        d = KO.distances(X, Qh)
        Qd = torch.from_numpy(Qh).cuda()
        for k in KS:
            knn = TS.KNeighborsClassifier(k).fit(Xd, y)
            assert knn.kernel_ok()
            conf = torch.zeros(len(knn.classes_), len(knn.classes_), dtype=torch.int32, device="cuda")
            pred, idx, dist = knn.classify(Qd, knn.class_index(yqh), conf, neighbours=True)
            assert nat.last_kernel().startswith("knn_classify_kernel")
            pred_h, idx_h, dist_h = knn.classes_[pred.cpu().numpy()], idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()
            dk = np.sort(d, axis=1)[:, k - 1]
            err, _ = _check_against_oracle(X, y, Qh, k, d, pred_h, idx_h, dist_h, KO.tau(D) * dk, "case %d %s k=%d" % (seed, qname, k))
            assert err <= KO.tau(D), (case, qname, k, err)
            if qname == "train":
                assert (dist_h[:, 0] == 0).all() and (idx_h[:, 0] == np.arange(n_train)).all()       # a training row finds itself first
            # the confusion matrix is the one of pred, and a second call accumulates
            cm = TS.confusion_matrix(yqh, pred_h, knn.classes_)
            assert (conf.cpu().numpy() == cm).all()
            pred2 = knn.classify(Qd, knn.class_index(yqh), conf)[0]
            assert torch.equal(pred2, pred) and (conf.cpu().numpy() == 2 * cm).all()
            assert (knn.predict(Qd).cpu().numpy() == pred_h).all() and (knn.predict(Qh) == pred_h).all()


def test_knn_exact_duplicates_go_to_the_lowest_indices():
    """8 copies of one row with alternating labels, k = 3: the neighbours are the three lowest indices, at distance 0; rows further
    away do not matter.  Also rows whose stride is padded (dim 6 in rows of 8 floats, rubbish in the padding)"""
    from two_stage_gnn_amd import two_stage as TS
    rng = np.random.default_rng(0)
    row = rng.normal(size=(1, 6)).astype(np.float32)
    X = np.concatenate([row + 3.0, np.repeat(row, 8, axis=0), row - 2.0])
    y = np.array([5, 0, 1, 0, 1, 0, 1, 0, 1, 5])
    buf = torch.full((10, 8), 1e30, device="cuda")
    buf[:, :6] = torch.from_numpy(X).cuda()
    knn = TS.KNeighborsClassifier(3).fit(buf[:, :6], y)
    assert knn.kernel_ok() and knn._X.data_ptr() == buf.data_ptr()                 # read in place, padding and all
    qbuf = torch.full((2, 8), -1e30, device="cuda")
    qbuf[:, :6] = torch.from_numpy(np.concatenate([row, row + 3.0])).cuda()
    pred, idx, dist = knn.classify(qbuf[:, :6], neighbours=True)
    assert idx[0].tolist() == [1, 2, 3] and dist[0].tolist() == [0.0, 0.0, 0.0] and int(knn.classes_[pred[0]]) == 0
    assert idx[1].tolist()[0] == 0 and float(dist[1, 0]) == 0.0


@pytest.mark.parametrize("k,D", [(17, 8), (3, 1028)])
def test_shapes_outside_the_kernel_fall_back_with_the_same_semantics(k, D):
    """k = 17 or D = 1028: ``tsgnn_knn_supported`` says no and the torch composition answers; same predictions as the oracle on
    case 4 (D = 1028: its rows zero-extended, which changes no distance)"""
    from two_stage_gnn_amd import two_stage as TS
    X, y, Q, yq = KO.synthetic(4, 37, 5, 8, 3, 0)
    if D > 8:
        X, Q = (np.concatenate([a, np.zeros((a.shape[0], D - 8), np.float32)], axis=1) for a in (X, Q))
    knn = TS.KNeighborsClassifier(k).fit(torch.from_numpy(X).cuda(), y)
    assert not knn.kernel_ok()
    for Qh in (Q, X):
        pred, idx, dist = knn.classify(torch.from_numpy(Qh).cuda(), neighbours=True)
        d = KO.distances(X, Qh)
        _check_against_oracle(X, y, Qh, k, d, knn.classes_[pred.cpu().numpy()], idx.cpu().numpy().astype(np.int64), dist.cpu().numpy(),
                              KO.tau(D) * np.sort(d, axis=1)[:, k - 1], "fallback k=%d D=%d" % (k, D))
    ref = TS.KNeighborsClassifier(min(k, 16)).fit(torch.from_numpy(X[:, :8].copy()).cuda(), y)       # the kernel on the same case
    if k <= 16:
        assert ref.kernel_ok() and torch.equal(ref.classify(torch.from_numpy(Q[:, :8].copy()).cuda())[0], knn.classify(torch.from_numpy(Q).cuda())[0])


# ----------------------------------------------------------------------------- embed_dataset
class _G:                       # stand-in for the networkx graphs cross_val.split_train_val prepares (cross_val.py:158-184)
    def __init__(self, adj, feats, n, label=0, assign=None):
        self.graph = {"adj": adj, "feats": feats, "num_nodes": n, "assign_feats": feats if assign is None else assign, "label": label}


class _A:
    bias = True


def _dense_model(kind, final_dim, nmax, fin, seed=4):
    from two_stage_gnn_amd import dense_encoders as E
    torch.manual_seed(seed)
    if kind == "base":
        m = E.GcnEncoderGraph(fin, 8, 8, 2, 3, bn=True, args=_A(), final_dim=final_dim)
    else:
        m = E.SoftPoolingGcnEncoder(nmax, fin, 8, 8, 2, 3, 8, assign_ratio=0.25, num_pooling=1, bn=True, linkpred=False, args=_A(),
                                    assign_input_dim=fin, final_dim=final_dim)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "conv" in k and k.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)
    return m.cuda()


def _dense_oracle_rows(kind, final_dim, m, x, adj, sizes):
    """fp64, one graph at a time: the second value of the B = 1 forward"""
    p = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    rows = []
    for b in range(x.size(0)):
        xb, ab = x[b:b + 1].double(), adj[b:b + 1].double()
        if kind == "base":
            _, e = R.gcn_encoder(p, xb, ab, bn=True, final_dim=final_dim)
        else:
            _, e = R.diffpool_encoder(p, xb, ab, sizes[b:b + 1], 1, assign_x=xb, final_dim=final_dim)
        rows.append(e[0])
    return torch.stack(rows)


@pytest.mark.parametrize("kind,final_dim", [("base", "output_dim"), ("base", "pretrain"), ("diffpool", "output_dim"), ("diffpool", "pretrain")])
def test_embed_dataset_dense_equals_b1_forwards(kind, final_dim):
    """GraphSage / DiffPool: rows of embed_dataset == the fp64 oracle's per-graph eval forwards at the triplet tests' tolerance, whatever
    the chunk (the kernels promise no bitwise independence of the batch around a graph: equal at the same tolerance is what is
    asserted; whether the bits agreed is printed), a short last chunk included; model state restored; a graph a tripletnet step has
    used is not uploaded again"""
    from two_stage_gnn_amd import triplet as T3, two_stage as TS
    nmax, fin, n_graphs = 24, 6, 44
    gen = torch.Generator().manual_seed(7)
    sizes = [24, 1, 2, 24] + torch.randint(3, nmax + 1, (n_graphs - 4,), generator=gen).tolist()
    x, adj, sizes = dense_batch(43, n_graphs, nmax, fin, sizes=sizes, p_edge=0.2)
    m = _dense_model(kind, final_dim, nmax, fin)
    m.train()
    want = _dense_oracle_rows(kind, final_dim, m, x, adj, sizes).float()
    graphs = [_G(adj[b].numpy(), x[b].numpy(), int(sizes[b]), label=b % 3) for b in range(n_graphs)]
    net = T3.tripletnet(m)
    net(graphs[0], graphs[5], graphs[9])                                   # a training step first: three graphs become resident
    cache = T3.resident_cache(m)
    assert net._resident is cache
    before = {k: id(v) for k, v in cache.items()}
    assert len(before) == 3 and cache.h2d == 3 * 3                         # rowptr, col, feats of each of the step's graphs
    full = TS.embed_dataset(m, graphs)
    assert m.training and m.per_graph_bn is False and full.shape == (n_graphs, 8) and not full.requires_grad
    entries = {k: id(v) for k, v in cache.items()}
    assert all(entries[k] == v for k, v in before.items())                 # the step's entries were reused, not rebuilt
    assert len(cache) == n_graphs and cache.h2d == 3 * n_graphs            # one entry per graph object, each uploaded once
    err = (full.cpu() - want).abs().max().item()
    print("%s %s: max |embed_dataset - fp64 B=1| = %.3g (scale %.3g)" % (kind, final_dim, err, want.abs().max().item()))
    torch.testing.assert_close(full.cpu(), want, rtol=1e-4, atol=1e-4)
    for chunk in (1, 7, 16, n_graphs):                                     # 44 = 6 * 7 + 2 = 2 * 16 + 12: short last chunks
        got = TS.embed_dataset(m, graphs, chunk=chunk)
        print("  chunk %d: bitwise equal to one chunk: %s" % (chunk, torch.equal(got, full)))
        torch.testing.assert_close(got.cpu(), want, rtol=1e-4, atol=1e-4)
    assert {k: id(v) for k, v in cache.items()} == entries and cache.h2d == 3 * n_graphs     # nothing uploaded again
    dp, dn = net(graphs[20], graphs[21], graphs[22])[:2]                   # ... and the reverse: a step on graphs an evaluation made resident
    assert {k: id(v) for k, v in cache.items()} == entries and cache.h2d == 3 * n_graphs
    assert torch.isfinite(dp).all() and torch.isfinite(dn).all()
    as_dict = {}
    for g in graphs:
        as_dict.setdefault(g.graph["label"], []).append(g)
    order = [b for c in (0, 1, 2) for b in range(n_graphs) if b % 3 == c]
    torch.testing.assert_close(TS.embed_dataset(m, as_dict).cpu(), want[order], rtol=1e-4, atol=1e-4)


def test_dense_chunk_limit_is_read_from_the_library():
    from two_stage_gnn_amd import _native as nat, two_stage as TS
    m = _dense_model("base", "output_dim", 24, 6)
    lim = TS.dense_chunk_limit(m)
    L = nat.lib()
    assert lim >= 3 and L.tsgnn_slot_fused_supported(lim, 8) == 1 and L.tsgnn_slot_fused_supported(lim + 1, 8) == 0


@pytest.mark.parametrize("conv", ["gcn", "sage"])
def test_embed_dataset_net_equals_b1_forwards(conv):
    """sag_layers.Net: rows == the fp64 oracle's model(data)[0] of every graph alone (graphs whose pooling cut is ambiguous in fp64
    are not used: the rule of tests/test_gpu_sag_triplet.py); chunks as above; no second upload of graph structure either way"""
    from test_gpu_sag_triplet import NET_SEED, RATIO, _D, _ambiguous, _graph, _net
    from two_stage_gnn_amd import sag_triplet as ST, two_stage as TS
    fin, nhid, C = 5, 32, 8
    net = _net(fin, nhid, C, conv, False, 0.5, seed=NET_SEED)
    net.train()
    p64 = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    graphs, seed = [], 0
    sizes = [1, 2, 64] + [3 + (7 * i) % 60 for i in range(60)]
    for n in sizes[:43]:
        for _ in range(50):                                                # (two nodes joined by an edge score alike: no edge there)
            seed += 1
            x, ei = _graph(5000 + seed, n, fin, 2.2 if n > 2 else 0)
            if not _ambiguous(p64, x, ei, conv):
                graphs.append((x, ei))
                break
    assert len(graphs) == 43 and [g[0].size(0) for g in graphs[:3]] == [1, 2, 64]
    with torch.no_grad():
        want = torch.cat([P.sag_net(p64, x.double(), ei, RATIO, batch=None, conv=conv)[0:1] for x, ei in graphs]).float()
    datas = [_D(x, ei) for x, ei in graphs]
    for i, d in enumerate(datas):
        d.y = torch.tensor([i % 2])
    tnet = ST.tripletnet(net)
    with torch.no_grad():
        tnet(datas[3], datas[4], datas[5])
    c = tnet.cache
    assert c is ST.resident_cache(net) and c.h2d == 6
    full = TS.embed_dataset(net, datas)
    assert net.training and full.shape == (43, C) and c.h2d == 6 + 2 * 40
    err = (full.cpu() - want).abs().max().item()
    print("Net %s: max |embed_dataset - fp64 B=1| = %.3g" % (conv, err))
    torch.testing.assert_close(full.cpu(), want, rtol=1e-4, atol=1e-4)
    for chunk in (1, 5, 16, 43):
        got = TS.embed_dataset(net, datas, chunk=chunk)
        print("  chunk %d: bitwise equal to one chunk: %s" % (chunk, torch.equal(got, full)))
        torch.testing.assert_close(got.cpu(), want, rtol=1e-4, atol=1e-4)
    with torch.no_grad():
        tnet(datas[30], datas[31], datas[32])
    assert c.h2d == 6 + 2 * 40                                             # no graph structure uploaded again, either way


def test_other_models_take_the_plain_loop():
    """the GAT encoder has no chunked path: one B = 1 forward per graph, rows kept on the device, the same rows as calling it"""
    from two_stage_gnn_amd import gat_encoders as G, two_stage as TS
    fin, nmax = 6, 12
    x, adj, sizes = dense_batch(5, 4, nmax, fin, sizes=[12, 5, 9, 3])
    torch.manual_seed(3)
    m = G.DGATEncoderGraph(fin, 8, 8, 2, None, num_layers=2, num_heads=[2, 2], final_dim="output_dim", per_graph_features=True).cuda().eval()
    graphs = [_G(adj[b].numpy(), x[b].numpy(), int(sizes[b])) for b in range(4)]
    got = TS.embed_dataset(m, graphs)
    with torch.no_grad():
        want = torch.cat([m(x[b:b + 1].cuda(), adj[b:b + 1].cuda(), sizes[b:b + 1])[1] for b in range(4)])
    assert got.is_cuda
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)


# ----------------------------------------------------------------------------- evaluate against the reference's own evaluate()
@pytest.mark.parametrize("kind", ["base", "diffpool"])
def test_evaluate_against_the_reference_fixture(kind):
    """tests/golden/two_stage_eval_*.npz: the reference's encoders, eval-mode B = 1 forwards, sklearn's classifier and metrics.
    Embeddings at rtol = atol = 1e-4; predictions under the undecided rule with the band widened to tau(D) d_k + 2 max_i |e_hip,i -
    e_ref,i| (each distance moves by at most the two rows' own errors); the fixture was chosen so that no query is undecided, so the
    metrics dictionary equals the reference's exactly"""
    from two_stage_gnn_amd import two_stage as TS
    g = load_golden("two_stage_eval_" + kind)
    nt, k = int(g["n_train"]), int(g["k"])
    nmax, fin = g["adj"].shape[1], g["feats"].shape[2]
    m = _dense_model(kind, "output_dim", nmax, fin)
    m.load_state_dict({n[2:]: torch.from_numpy(v) for n, v in g.items() if n.startswith("p.")})
    graphs = [_G(g["adj"][i].astype(np.float32), g["feats"][i], int(g["num_nodes"][i]), int(g["label"][i])) for i in range(len(g["label"]))]
    train, val = graphs[:nt], graphs[nt:]
    emb = TS.embed_dataset(m, graphs).cpu().numpy()
    E = g["embed"]
    e_max = float(np.sqrt(((emb.astype(np.float64) - E) ** 2).sum(1)).max())
    print("%s: max |e_hip - e_ref| = %.3g (2-norm of a row; scale %.3g)" % (kind, e_max, np.abs(E).max()))
    np.testing.assert_allclose(emb, E, rtol=1e-4, atol=1e-4)
    y = g["label"]
    knn = TS.KNeighborsClassifier(k).fit(torch.from_numpy(emb[:nt]).cuda(), y[:nt])
    n_und = 0
    for Qh, Q_hip, want_pred in ((E[nt:], emb[nt:], g["pred_val"]), (E[:nt], emb[:nt], g["pred_train"])):
        d = KO.distances(E[:nt], Qh)
        band = KO.tau(E.shape[1]) * np.sort(d, axis=1)[:, k - 1] + 2 * e_max
        und = KO.undecided(d, y[:nt], k, band)
        pred = knn.predict(torch.from_numpy(Q_hip).cuda()).cpu().numpy()
        print("  undecided %d / %d, predictions that differ from sklearn's %d" % (und.sum(), und.size, (pred != want_pred).sum()))
        assert und.mean() <= CAP
        assert ((pred == want_pred) | und).all()
        n_und += int(und.sum())
    res = TS.evaluate(train, val, m, n_neighbors=k)
    want = dict(zip(("prec", "recall", "acc", "F1"), g["metrics"].tolist()))
    want["train acc"] = float(g["train_acc"])
    print("  evaluate:", res, "reference:", want)
    assert n_und == 0                                                      # (the generator chose the dataset so)
    assert res == want
    by_class = lambda gs: {c: [q for q in gs if q.graph["label"] == c] for c in sorted({q.graph["label"] for q in gs}, reverse=True)}
    assert TS.evaluate(by_class(train), by_class(val), m, n_neighbors=k) == want


def test_evaluate_copies_to_the_host_once():
    """after the embeddings exist: fit, both predictions and both confusion matrices without a host synchronisation
    (``set_sync_debug_mode('error')`` raises at any); the ONE copy is that of the two matrices"""
    from two_stage_gnn_amd import two_stage as TS
    X, y, Q, yq = KO.synthetic(0, 1051, 117, 64, 2, 0)
    Xd, Qd = torch.from_numpy(X).cuda(), torch.from_numpy(Q).cuda()
    TS.knn_confusions_device(Xd, y, Qd, yq, 3)                             # (first use: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        conf, labels = TS.knn_confusions_device(Xd, y, Qd, yq, 3)
        with pytest.raises(RuntimeError):
            conf.cpu()                                                     # (the mode is live: a copy to the host IS flagged)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    conf = conf.cpu().numpy()
    assert conf[0].sum() == 117 and conf[1].sum() == 1051
    pred, pred_t = KO.brute_force(X, y, Q, 3)[0], KO.brute_force(X, y, X, 3)[0]
    d, dt = KO.distances(X, Q), KO.distances(X, X)
    if not (KO.undecided(d, y, 3, KO.tau(64) * np.sort(d, axis=1)[:, 2]).any() or KO.undecided(dt, y, 3, KO.tau(64) * np.sort(dt, axis=1)[:, 2]).any()):
        assert (conf[0] == TS.confusion_matrix(yq, pred, labels)).all() and (conf[1] == TS.confusion_matrix(y, pred_t, labels)).all()
    res = TS.metrics_from_confusion(conf[0])
    assert 0.0 <= res["prec"] <= 1.0 and res["acc"] == np.trace(conf[0]) / 117
