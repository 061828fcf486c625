"""Stage two without a GPU: the fp64 brute-force oracle and the numpy metrics pinned to sklearn's recorded results
(tests/golden/knn_*.npz, scripts/gen_golden_knn.py), the declared C ABI of csrc/knn.hip, and the host logic of
``two_stage.embed_dataset`` / ``evaluate`` on the plain-loop path with a stub model."""
import glob
import os

import numpy as np
import pytest
import torch

import knn_oracle as KO
from conftest import GOLDEN, load_golden

KNN_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "knn_*.npz")))


def test_fixture_list_covers_the_cases():
    assert len(KNN_FIXTURES) >= 4
    ks, absent, labels = set(), False, set()
    for name in KNN_FIXTURES:
        g = load_golden(name)
        ks.add(int(g["k"]))
        labels |= set(g["y"].tolist())
        absent |= bool(set(g["y"].tolist()) - set(g["y_q"].tolist()))
    assert ks >= {1, 3, 5} and absent and labels == {3, 7, 11, 12, 40, 41}


@pytest.mark.parametrize("name", KNN_FIXTURES)
def test_brute_force_oracle_is_sklearn(name):
    """the ten-line fp64 brute force (tests/knn_oracle.py) gives sklearn's predictions, neighbours and distances: it is the oracle of
    every larger case"""
    g = load_golden(name)
    k = int(g["k"])
    pred, idx, dist = KO.brute_force(g["X"], g["y"], g["Q"], k)
    assert pred.dtype == g["y"].dtype and (pred == g["pred"]).all()
    assert (idx == g["nbr_index"]).all()
    np.testing.assert_allclose(dist, g["nbr_dist"], rtol=1e-12, atol=0)
    assert (KO.brute_force(g["X"], g["y"], g["X"], k)[0] == g["pred_train"]).all()
    assert not KO.undecided(KO.distances(g["X"], g["Q"]), g["y"], k, np.zeros(g["Q"].shape[0])).any()      # (no exact ties at the k-th place)


@pytest.mark.parametrize("name", KNN_FIXTURES)
def test_numpy_metrics_are_sklearns(name):
    from two_stage_gnn_amd import two_stage as TS
    g = load_golden(name)
    labels = np.unique(np.concatenate([g["y"], g["y_q"]]))                  # evaluate()'s table: classes nobody is or predicts drop out
    res = TS.metrics_from_confusion(TS.confusion_matrix(g["y_q"], g["pred"], labels))
    assert [res["prec"], res["recall"], res["acc"], res["F1"]] == g["metrics"].tolist()
    cm = TS.confusion_matrix(g["y"], g["pred_train"], labels)
    assert np.trace(cm) / cm.sum() == float(g["train_acc"])


def test_metrics_with_a_class_that_is_never_true():
    """sklearn's label set is the union of true and predicted labels: a predicted class without true samples has recall 0 and counts in
    the macro mean; a class that is neither true nor predicted does not (values: sklearn.metrics 1.7.2 on these vectors)"""
    from two_stage_gnn_amd import two_stage as TS
    y_true, y_pred = np.array([0, 0, 1, 1, 1, 0]), np.array([0, 2, 1, 1, 0, 0])
    res = TS.metrics_from_confusion(TS.confusion_matrix(y_true, y_pred, np.array([0, 1, 2, 5])))
    assert res["prec"] == (2 / 3 + 1.0 + 0.0) / 3 and res["recall"] == (2 / 3 + 2 / 3 + 0.0) / 3
    assert res["acc"] == 4 / 6 and res["F1"] == 4 / 6


@pytest.mark.parametrize("name", KNN_FIXTURES)
def test_classifier_torch_composition_matches_sklearn_on_the_cpu(name):
    """``KNeighborsClassifier`` on CPU tensors runs the torch composition (the path of shapes the kernel does not take): sklearn's
    predictions and neighbours, labels back in the dtype of y, containers as given"""
    from two_stage_gnn_amd import two_stage as TS
    g = load_golden(name)
    knn = TS.KNeighborsClassifier(int(g["k"])).fit(torch.from_numpy(g["X"]), g["y"])
    assert (knn.classes_ == np.unique(g["y"])).all() and not knn.kernel_ok()
    pred = knn.predict(torch.from_numpy(g["Q"]))
    assert isinstance(pred, torch.Tensor) and pred.dtype == torch.int64 and (pred.numpy() == g["pred"]).all()
    dist, idx = knn.kneighbors(torch.from_numpy(g["Q"]))
    assert (idx.numpy() == g["nbr_index"]).all()
    np.testing.assert_allclose(dist.numpy(), g["nbr_dist"], rtol=1e-5)
    conf, labels = TS.knn_confusions(torch.from_numpy(g["X"]), g["y"], torch.from_numpy(g["Q"]), g["y_q"], int(g["k"]))
    assert (conf[0] == TS.confusion_matrix(g["y_q"], g["pred"], labels)).all()
    assert (conf[1] == TS.confusion_matrix(g["y"], g["pred_train"], labels)).all()


def test_abi_declares_the_knn_entry_points():
    """include/tsgnn.h declares both entry points (tests/test_abi.py then checks them against the built library) and the limits the
    issue asks for are taken; bad arguments are refused before any launch"""
    from two_stage_gnn_amd import _native as nat
    decls = nat.parse_header()
    assert "tsgnn_knn_supported" in decls and "tsgnn_knn_classify_f32" in decls
    assert [n for _, n in decls["tsgnn_knn_classify_f32"][1]] == [
        "train", "ld_train", "train_class", "n_train", "query", "ld_query", "n_query", "dim", "k", "n_classes", "query_class", "confusion",
        "pred", "nbr_index", "nbr_dist", "stream"]
    L = nat.lib()
    assert L.tsgnn_knn_supported(1024, 16, 64) == 1 and L.tsgnn_knn_supported(1, 1, 1) == 1
    assert L.tsgnn_knn_supported(1028, 3, 2) == 0 and L.tsgnn_knn_supported(64, 17, 2) == 0 and L.tsgnn_knn_supported(64, 3, 65) == 0
    assert L.tsgnn_knn_supported(0, 3, 2) == 0 and L.tsgnn_knn_supported(64, 0, 2) == 0
    P = 1 << 20
    assert L.tsgnn_knn_classify_f32(None, 64, P, 10, P, 64, 5, 64, 3, 2, None, None, P, None, None, None) == -1
    assert L.tsgnn_knn_classify_f32(P, 64, P, 2, P, 64, 5, 64, 3, 2, None, None, P, None, None, None) == -1       # k > n_train
    assert L.tsgnn_knn_classify_f32(P, 64, P, 10, P, 64, 0, 64, 3, 2, None, None, P, None, None, None) == -1      # no queries
    assert L.tsgnn_knn_classify_f32(P, 32, P, 10, P, 64, 5, 64, 3, 2, None, None, P, None, None, None) == -1      # rows shorter than dim
    assert L.tsgnn_knn_classify_f32(P, 66, P, 10, P, 64, 5, 64, 3, 2, None, None, P, None, None, None) == -3      # stride not 16-byte rows
    assert L.tsgnn_knn_classify_f32(P + 4, 64, P, 10, P, 64, 5, 64, 3, 2, None, None, P, None, None, None) == -3  # misaligned rows
    assert L.tsgnn_knn_classify_f32(P, 64, P, 10, P, 64, 5, 64, 17, 2, None, None, P, None, None, None) == -1     # k > n_train first
    assert L.tsgnn_knn_classify_f32(P, 64, P, 100, P, 64, 5, 64, 17, 2, None, None, P, None, None, None) == -3    # k beyond the kernel's bound


# ----------------------------------------------------------------------------- embed_dataset / evaluate: host logic, stub model
class _G:
    def __init__(self, rng, label, nmax=6, fin=3):
        n = int(rng.integers(1, nmax + 1))
        feats = np.zeros((nmax, fin), dtype=np.float32)
        feats[:n] = rng.normal(size=(n, fin)) + label
        self.graph = {"adj": np.zeros((nmax, nmax), dtype=np.float32), "feats": feats, "num_nodes": n, "assign_feats": feats,
                      "label": label}


class _D:
    def __init__(self, rng, label):
        self.x = torch.from_numpy(rng.normal(size=(int(rng.integers(1, 6)), 3)).astype(np.float32) + label)
        self.edge_index = torch.zeros(2, 0, dtype=torch.long)
        self.y = torch.tensor([label])


class _Stub(torch.nn.Module):
    """a user's module on the CPU: takes both call shapes of the reference, counts its calls, can be told to fail"""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 5)
        self.per_graph_bn = False
        self.calls, self.fail_at, self.seen_training = 0, None, []

    def forward(self, x, adj=None, batch_num_nodes=None, assign_x=None):
        self.calls += 1
        self.seen_training.append((self.training, torch.is_grad_enabled()))
        if self.fail_at is not None and self.calls >= self.fail_at:
            raise RuntimeError("stub failure")
        if adj is None:                                              # Data-like: model(data)[0] is the embedding row
            return self.lin(x.x).sum(0, keepdim=True)
        assert x.dim() == 3 and x.size(0) == 1 and adj.shape[:2] == (1, x.size(1)) and len(batch_num_nodes) == 1
        assert assign_x is not None
        n = int(batch_num_nodes[0])
        return None, self.lin(x[:, :n]).sum(1)                       # (out, feat): feat[0] is the embedding row


def _sets(kind, seed=0):
    rng = np.random.default_rng(seed)
    make = _G if kind == "dense" else _D
    labels = [4, 9, 9, 4, 17, 4, 9, 17, 17, 4, 9, 4]
    graphs = [make(rng, c) for c in labels]
    return graphs[:8], graphs[8:]


@pytest.mark.parametrize("kind", ["dense", "data"])
def test_embed_dataset_and_evaluate_accept_both_container_shapes(kind):
    from two_stage_gnn_amd import two_stage as TS
    train, val = _sets(kind)
    m = _Stub()
    m.train()
    emb = TS.embed_dataset(m, train)
    assert emb.shape == (8, 5) and emb.dtype == torch.float32 and not emb.requires_grad and m.calls == 8
    assert m.training and all(s == (False, False) for s in m.seen_training)          # eval mode, no grad inside; restored outside
    assert emb.stride(0) % 4 == 0 and emb.data_ptr() % 16 == 0                       # 16-byte rows for the classifier kernel
    label_of = (lambda g: g.graph["label"]) if kind == "dense" else (lambda g: int(g.y))

    def by_class(graphs):
        d = {}
        for g in graphs:
            d.setdefault(label_of(g), []).append(g)
        return d
    as_dict = TS.embed_dataset(m, by_class(train))                                   # {class: [graphs]}: iteration order kept
    order = [g for c in by_class(train).values() for g in c]
    assert torch.equal(as_dict, TS.embed_dataset(m, order)) and not torch.equal(as_dict, emb)
    res = TS.evaluate(train, val, m, n_neighbors=3)
    res_d = TS.evaluate(by_class(train), by_class(val), m, n_neighbors=3)
    assert list(res) == ["prec", "recall", "acc", "F1", "train acc"]
    # the same numbers as the oracle on the stub's embeddings (a dictionary only reorders the rows)
    E, Ev = emb.numpy(), TS.embed_dataset(m, val).numpy()
    y, yv = np.array([label_of(g) for g in train]), np.array([label_of(g) for g in val])
    pred, pred_t = KO.brute_force(E, y, Ev, 3)[0], KO.brute_force(E, y, E, 3)[0]
    want = TS.metrics_from_confusion(TS.confusion_matrix(yv, pred, np.unique(np.concatenate([y, yv, pred]))))
    want["train acc"] = float((pred_t == y).mean())
    assert res == want and res_d == want


@pytest.mark.parametrize("kind", ["dense", "data"])
def test_state_is_restored_after_a_forward_that_raises(kind):
    from two_stage_gnn_amd import two_stage as TS
    train, val = _sets(kind)
    for training, per_graph in ((True, False), (False, True), (True, True)):
        m = _Stub()
        m.train(training)
        m.per_graph_bn = per_graph
        m.fail_at = 3
        with pytest.raises(RuntimeError, match="stub failure"):
            TS.embed_dataset(m, train)
        assert m.training is training and m.per_graph_bn is per_graph and torch.is_grad_enabled()
        m.calls = 0
        with pytest.raises(RuntimeError, match="stub failure"):
            TS.evaluate(train, val, m)
        assert m.training is training and m.per_graph_bn is per_graph and torch.is_grad_enabled()


def test_chunk_and_neighbour_arguments_are_checked():
    from two_stage_gnn_amd import two_stage as TS
    train, _ = _sets("dense")
    with pytest.raises(ValueError):
        TS.embed_dataset(_Stub(), train, chunk=0)
    with pytest.raises(ValueError):
        TS.KNeighborsClassifier(0)
    with pytest.raises(ValueError):
        TS.KNeighborsClassifier(5).fit(torch.zeros(3, 4), [0, 1, 0])
    assert TS.embed_dataset(_Stub(), []).shape[0] == 0


def test_shared_resident_caches_are_per_model():
    """a tripletnet and embed_dataset around the same model see one cache (no second upload of a graph); another model has its own;
    one registry serves the three families"""
    import types
    from two_stage_gnn_amd import eigen_triplet as ET, resident as RS, sag_triplet as ST, triplet as T
    a, b = _Stub(), _Stub()
    assert T.resident_cache(a) is T.resident_cache(a) and T.resident_cache(a) is not T.resident_cache(b)
    assert T.resident_cache is RS.resident_cache and ST.resident_cache is RS.resident_cache and ST.ResidentCache is RS.ResidentCache
    assert T.tripletnet(a)._resident is T.resident_cache(a) and isinstance(T.tripletnet(a)._resident, RS.ResidentCache)
    assert ST.tripletnet(a).cache is ST.resident_cache(a) and ST.tripletnet(b).cache is not ST.tripletnet(a).cache
    args = types.SimpleNamespace(pool_sizes="3_2", num_pool_matrix=2, num_pool_final_matrix=1)
    for m in (a, b):
        m.pool_sizes, m.num_pool_matrix, m.num_pool_final_matrix = [3, 2], 2, 1
    assert ET.tripletnet(a, args).cache is ET.tripletnet(a, args).cache and ET.tripletnet(a, args).cache is RS.resident_cache(a)
    assert ET.tripletnet(b, args).cache is RS.resident_cache(b) and ET.tripletnet(b, args).cache is not ET.tripletnet(a, args).cache
