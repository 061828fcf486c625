"""Stage two of the two-stage scheme: embed every graph of the train and validation sets and classify by k-nearest-neighbour on the
embeddings — the reference's ``evaluate()`` (Code/sage+gat+diffpool/train_triplet.py:36-101, Code/sag/train_triplet.py:34-73), which
runs one B = 1 forward per graph, copies every embedding to the host and fits sklearn's ``KNeighborsClassifier`` there.

Here the graphs go through the encoder in block-diagonal chunks (``embed_dataset``: the resident per-graph device pieces of
``triplet.py`` / ``sag_triplet.py``, per-graph statistics, so row i is the eval-mode B = 1 forward of graph i), the classifier is one
HIP launch per prediction (csrc/knn.hip: distances, selection, vote and confusion matrix) and ``evaluate`` copies two small confusion
matrices to the host, once.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from . import _native as nat
from . import message_passing as mp


# ----------------------------------------------------------------------------- containers
def _flatten(graphs):
    """the reference's two call shapes -> a list: ``{class: [graphs]}`` dictionaries in iteration order (train_triplet.py:49-50) or any
    sequence / iterable of graphs (Code/sag: a loader of single graphs)"""
    if isinstance(graphs, dict):
        return [g for c in graphs.keys() for g in graphs[c]]
    return list(graphs)


def _is_dense(g):
    return isinstance(getattr(g, "graph", None), dict)


def _labels(graphs):
    """host labels of the graphs: ``graph.graph['label']`` or ``data.y`` (labels that live on the device come back in ONE copy)"""
    if not graphs:
        return np.zeros(0, dtype=np.int64)
    if _is_dense(graphs[0]):
        return np.asarray([np.asarray(g.graph["label"]).reshape(-1)[0] for g in graphs])
    ys = [g.y for g in graphs]
    if any(isinstance(y, torch.Tensor) and y.is_cuda for y in ys):
        return torch.cat([torch.as_tensor(y).reshape(-1)[:1].to(ys[0].device) for y in ys]).cpu().numpy()
    return np.asarray([(y.detach().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)).reshape(-1)[0] for y in ys])


# ----------------------------------------------------------------------------- embed_dataset
_NET_CHUNK = 512            # sag_layers.Net: the fused per-graph kernels take any number of graphs; this bounds a chunk's rows in memory
_DENSE_CHUNK = 128          # dense family, when the fused slot kernels take none of its widths (the composed path has no limit)


@contextlib.contextmanager
def _eval_mode(model):
    """eval mode (dropout off), per-graph batch-norm statistics (trap T2: the slot batch-norm uses fresh statistics in eval mode too,
    so a chunk must give every graph the statistics it has alone), no autograd; everything restored on exit, also on an exception"""
    training = model.training
    has_pg = hasattr(model, "per_graph_bn")
    per_graph = getattr(model, "per_graph_bn", None)
    try:
        model.eval()
        if has_pg:
            model.per_graph_bn = True
        with torch.no_grad():
            yield
    finally:
        model.train(training)
        if has_pg:
            model.per_graph_bn = per_graph


def _device_of(model):
    p = next(iter(model.parameters()), None) if hasattr(model, "parameters") else None
    return p.device if p is not None else torch.device("cpu")


def dense_chunk_limit(model):
    """the largest number of graphs the fused per-graph launches of a GraphSage / DiffPool encoder take in one batch, asked of the
    library (``tsgnn_slot_fused_supported`` for the widths of the conv stack)"""
    lib = nat.lib()
    widths = (int(model.conv_first.output_dim), int(model.conv_last.output_dim))

    def ok(b):
        return all(lib.tsgnn_slot_fused_supported(int(b), w) for w in widths)
    if not ok(1):
        return _DENSE_CHUNK
    lo, hi = 1, 2
    while hi <= (1 << 16) and ok(hi):
        lo, hi = hi, hi * 2
    while hi - lo > 1:                      # ok(lo) and not ok(hi)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def _embed_dense_chunk(model, graphs, dev, cache):
    from . import triplet as T
    g, x, xa, sizes = T._assemble([T._resident(o, dev, cache) for o in graphs], dev, cache)
    _, feat = model(x, g, sizes, assign_x=x if xa is None else xa)
    return feat


def _embed_net_chunk(tnet, graphs):
    """sag_layers.Net on a chunk: per-graph pooling and read-outs (Net has no batch-norm: this IS one forward per graph), the head on
    all rows of the chunk at once"""
    from . import pyg
    m = tnet.model
    r = tnet._readout(tnet.batch_of(graphs))
    if mp.mlp3_ok(r, m.lin1, m.lin2, m.lin3):
        return mp.mlp3_log_softmax(r, m.lin1, m.lin2, m.lin3, m.dropout_ratio, False)
    h = pyg.relu(mp.linear_oi(r, m.lin1.weight, m.lin1.bias))
    h = pyg.relu(mp.linear_oi(h, m.lin2.weight, m.lin2.bias))
    return F.log_softmax(mp.linear_oi(h, m.lin3.weight, m.lin3.bias), dim=-1)


def _embed_one(model, g, dev):
    """the reference's own call for one graph (train_triplet.py:52-59; Code/sag/train_triplet.py:45-47)"""
    if _is_dense(g):
        d = g.graph
        adj = torch.as_tensor(np.asarray(d["adj"], dtype=np.float32)[None], device=dev)
        h0 = torch.as_tensor(np.asarray(d["feats"], dtype=np.float32)[None], device=dev)
        fa = np.asarray(d["assign_feats"], dtype=np.float32)
        same = fa.shape == tuple(h0.shape[1:]) and np.array_equal(fa, np.asarray(d["feats"], dtype=np.float32))
        assign = h0 if same else torch.as_tensor(fa[None], device=dev)
        _, feat = model(h0, adj, np.array([int(d["num_nodes"])]), assign_x=assign)
        return feat[0]
    return model(g)[0]


def embed_dataset(model, graphs, chunk=None):
    """-> [len(graphs), E] float32 on the model's device, no grad: row i is the eval-mode B = 1 forward of graph i alone, as the
    reference's ``evaluate()`` stores it (``feat[0]`` of ``out, feat = model(...)`` for the dense encoders, ``model(data)[0]`` for the
    SAGPool network).

    ``graphs``: a sequence (or a ``{class: [graphs]}`` dictionary) of objects with ``.graph = {'adj', 'feats', 'num_nodes',
    'assign_feats', ...}`` (dense family) or of ``Data``-like objects with ``.x`` / ``.edge_index`` on the GPU (SAGPool family).

    ``dense_encoders.GcnEncoderGraph`` / ``SoftPoolingGcnEncoder`` and ``sag_layers.Net`` run in block-diagonal chunks of ``chunk``
    graphs (default: the most the fused per-graph launches take) on the graphs' resident device pieces — the caches of
    ``triplet.tripletnet`` / ``sag_triplet.tripletnet`` around the same model, so a graph a training step has used is not uploaded
    again, and the reverse.  ANY OTHER model (the GAT encoder, EigenGCN, a module of your own) gets a plain loop of B = 1 forwards
    with the rows kept on the device: correct, and not fast.  ``model`` may also be a ``tripletnet`` (its ``.model`` is used)."""
    from . import dense_encoders as E, sag_layers as S, sag_triplet as ST, triplet as T
    if isinstance(model, (T.tripletnet, ST.tripletnet)):
        model = model.model
    graphs = _flatten(graphs)
    dev = _device_of(model)
    if chunk is not None and int(chunk) < 1:
        raise ValueError("chunk must be at least 1")
    rows = []
    with _eval_mode(model):
        if not graphs:
            return torch.zeros(0, 0, dtype=torch.float32, device=dev)
        if isinstance(model, E.GcnEncoderGraph) and dev.type == "cuda" and T.RESIDENT and _is_dense(graphs[0]):
            step = int(chunk) if chunk is not None else dense_chunk_limit(model)
            cache = T.resident_cache(model)
            for i in range(0, len(graphs), step):
                rows.append(_embed_dense_chunk(model, graphs[i:i + step], dev, cache))
        elif isinstance(model, S.Net) and dev.type == "cuda" and not _is_dense(graphs[0]):
            step = int(chunk) if chunk is not None else _NET_CHUNK
            tnet = ST.tripletnet(model)
            for i in range(0, len(graphs), step):
                rows.append(_embed_net_chunk(tnet, graphs[i:i + step]))
        else:
            rows = [_embed_one(model, g, dev).reshape(1, -1) for g in graphs]
        out = torch.cat(rows) if len(rows) > 1 else rows[0]
        out = out.float() if out.dtype != torch.float32 else out
    return _rows16(out)                                        # 16-byte rows: what the kNN kernel reads


# ----------------------------------------------------------------------------- k-nearest-neighbour classifier
def _rows16(t):
    """float32 rows the kernel takes as they are (unit column stride, row stride a multiple of 4 floats >= dim rounded up, 16-byte
    aligned), else a zero-padded copy"""
    n, d = t.shape
    pad = (d + 3) // 4 * 4
    if t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= pad and t.data_ptr() % 16 == 0:
        return t
    out = torch.zeros(n, pad, dtype=torch.float32, device=t.device)
    out[:, :d] = t
    return out[:, :d]


def _as_matrix(a, dev=None):
    """float32 rows [n, d]; a tensor stays where it is, host data goes to ``dev`` (default: the current GPU when there is one)"""
    if isinstance(a, torch.Tensor):
        t = a.detach()
    else:
        if isinstance(a, (list, tuple)) and len(a) and isinstance(a[0], torch.Tensor):
            t = torch.stack([r.detach().reshape(-1) for r in a])
        else:
            t = torch.as_tensor(np.asarray(a, dtype=np.float32))
        if dev is None and not t.is_cuda and torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
    if t.dim() != 2:
        raise ValueError("expected a 2-D array of rows")
    if dev is not None:
        t = t.to(dev)
    return t.float() if t.dtype != torch.float32 else t


def _upload(arr, dev):
    """a small host array -> device without a host synchronisation (pinned staging; the caching host allocator keeps the buffer
    until the copy has run)"""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t


def knn_torch(X, cls, Q, k, n_classes, block=1024):
    """the kernel's semantics as a torch composition (shapes ``tsgnn_knn_supported`` does not take, and tensors on the CPU): exact
    difference-form distances (cdist's default switches to the cancelling product form above 25 rows) and a STABLE sort, so equal
    distances keep the lower training index (topk's order among equals is undefined).  -> (pred int32 [nq], idx int32 [nq, k],
    dist [nq, k])"""
    preds, idxs, dists = [], [], []
    rank = torch.arange(n_classes - 1, -1, -1, device=X.device)
    for i in range(0, Q.size(0), block):
        d = torch.cdist(Q[i:i + block].contiguous(), X.contiguous(), compute_mode="donot_use_mm_for_euclid_dist")
        dv, di = torch.sort(d, dim=1, stable=True)
        dv, di = dv[:, :k], di[:, :k]
        votes = F.one_hot(cls.long()[di], n_classes).sum(1)
        preds.append(torch.argmax(votes * n_classes + rank, dim=1).int())     # (rank: a tied vote goes to the smallest class)
        idxs.append(di.int())
        dists.append(dv)
    return torch.cat(preds), torch.cat(idxs), torch.cat(dists)


class KNeighborsClassifier:
    """``sklearn.neighbors.KNeighborsClassifier(n_neighbors=k)`` (uniform weights, Euclidean, brute force) as every ``evaluate()`` of
    the reference constructs it.  Neighbours ascend by distance, equal distances go to the lower training index (sklearn leaves that
    order open); a query that is a training row finds itself at distance 0; a tied vote goes to the smallest class of ``classes_``.

    ``X`` / ``Q``: device tensors (``embed_dataset``'s output) or anything ``torch.as_tensor`` takes (computed on the GPU when there
    is one).  ``fit`` keeps the tensors: there is no tree."""

    def __init__(self, n_neighbors=3):
        if int(n_neighbors) < 1:
            raise ValueError("n_neighbors must be at least 1")
        self.n_neighbors = int(n_neighbors)

    def fit(self, X, y, classes=None):
        """``y``: labels on the host (a list, an array, a CPU tensor; a device tensor is copied back).  ``classes`` (optional): the
        sorted label table to count votes over when it is wider than the labels of ``y`` (``evaluate``: the union with the validation
        labels, so both confusion matrices share their axes); default: the sorted unique labels, sklearn's ``classes_``"""
        yh = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        yh = yh.reshape(-1)
        self._X = _rows16(_as_matrix(X))
        if self._X.size(0) != yh.size:
            raise ValueError("X has %d rows, y has %d labels" % (self._X.size(0), yh.size))
        if self.n_neighbors > self._X.size(0):
            raise ValueError("n_neighbors = %d > %d training rows" % (self.n_neighbors, self._X.size(0)))
        self.classes_ = np.unique(yh) if classes is None else np.asarray(classes)
        self._y_tensor = isinstance(y, torch.Tensor)
        self._cls = self.class_index(yh)
        return self

    def class_index(self, labels):
        """host labels -> int32 device tensor of their positions in ``classes_``"""
        labels = np.asarray(labels).reshape(-1)
        pos = np.searchsorted(self.classes_, labels)
        if labels.size and ((pos >= self.classes_.size).any() or (self.classes_[np.minimum(pos, self.classes_.size - 1)] != labels).any()):
            raise ValueError("a label is not in classes_")
        return _upload(pos.astype(np.int32), self._X.device)

    def kernel_ok(self, dim=None):
        d = int(self._X.size(1)) if dim is None else int(dim)
        return bool(self._X.is_cuda and nat.lib().tsgnn_knn_supported(d, self.n_neighbors, int(self.classes_.size)))

    def classify(self, Q, query_class=None, confusion=None, neighbours=False):
        """-> (pred int32 [nq] as positions in ``classes_``, idx int32 [nq, k] or None, dist [nq, k] or None); with ``query_class``
        (int32 positions) and ``confusion`` (int32 [C, C] on the device): ``confusion[t, p] += 1`` per query.  ONE launch, nothing
        copied to the host"""
        X, k, C = self._X, self.n_neighbors, int(self.classes_.size)
        Q = _as_matrix(Q, X.device)
        if Q.size(1) != X.size(1):
            raise ValueError("query rows have %d columns, training rows %d" % (Q.size(1), X.size(1)))
        nq = int(Q.size(0))
        if nq == 0:
            z = torch.zeros(0, k, device=X.device)
            return torch.zeros(0, dtype=torch.int32, device=X.device), z.int(), z
        if self.kernel_ok():
            Q = _rows16(Q)
            pred = torch.empty(nq, dtype=torch.int32, device=X.device)
            idx = torch.empty(nq, k, dtype=torch.int32, device=X.device) if neighbours else None
            dist = torch.empty(nq, k, dtype=torch.float32, device=X.device) if neighbours else None
            nat.call("knn_classify_f32", X, X.stride(0), self._cls, int(X.size(0)), Q, Q.stride(0), nq, int(X.size(1)), k, C,
                     query_class if confusion is not None else None, confusion, pred, idx, dist)
            return pred, idx, dist
        pred, idx, dist = knn_torch(X, self._cls, Q, k, C)
        if confusion is not None and query_class is not None:
            confusion.view(-1).index_add_(0, query_class.long() * C + pred.long(), torch.ones(nq, dtype=confusion.dtype, device=X.device))
        return pred, idx, dist

    def _classes_on(self, dev):
        return _upload(self.classes_, dev)

    def predict(self, Q):
        """labels of the rows of ``Q`` with the dtype of ``y``: a tensor on Q's device for a tensor, else a numpy array"""
        pred = self.classify(Q)[0]
        if isinstance(Q, torch.Tensor):
            return self._classes_on(pred.device)[pred.long()].to(Q.device)
        return self.classes_[pred.cpu().numpy()]

    def kneighbors(self, Q):
        """-> (dist [nq, k], idx [nq, k] int64), neighbours ascending by distance"""
        _, idx, dist = self.classify(Q, neighbours=True)
        if isinstance(Q, torch.Tensor):
            return dist.to(Q.device), idx.long().to(Q.device)
        return dist.cpu().numpy(), idx.long().cpu().numpy()


# ----------------------------------------------------------------------------- metrics (numpy, sklearn's rules)
def confusion_matrix(y_true, y_pred, labels):
    """int64 [C, C] over the sorted label table ``labels``: rows true, columns predicted"""
    labels = np.asarray(labels)
    t, p = np.searchsorted(labels, np.asarray(y_true).reshape(-1)), np.searchsorted(labels, np.asarray(y_pred).reshape(-1))
    cm = np.zeros((labels.size, labels.size), dtype=np.int64)
    np.add.at(cm, (t, p), 1)
    return cm


def metrics_from_confusion(cm):
    """{'prec', 'recall', 'acc', 'F1'} of a confusion matrix as ``sklearn.metrics`` computes them from the label vectors
    (train_triplet.py:90-93): macro precision and recall over the labels that occur as true OR predicted (a class nobody predicted has
    precision 0, a class that is never true has recall 0, the plain mean over that set), accuracy, micro F1 (for single-label data:
    the accuracy)"""
    cm = np.asarray(cm, dtype=np.int64)
    tp, true_n, pred_n = np.diag(cm), cm.sum(1), cm.sum(0)
    present = (true_n + pred_n) > 0
    tp, true_n, pred_n = tp[present], true_n[present], pred_n[present]
    prec = np.divide(tp, pred_n, out=np.zeros(tp.size, dtype=np.float64), where=pred_n > 0)
    rec = np.divide(tp, true_n, out=np.zeros(tp.size, dtype=np.float64), where=true_n > 0)
    total, hit = int(cm.sum()), int(tp.sum())
    fp_fn = 2 * (total - hit)
    return {"prec": float(prec.mean()) if tp.size else 0.0, "recall": float(rec.mean()) if tp.size else 0.0,
            "acc": hit / total if total else 0.0, "F1": 2 * hit / (2 * hit + fp_fn) if total else 0.0}


def knn_confusions_device(X_train, y_train, X_val, y_val, n_neighbors=3):
    """fit on the training rows, predict the validation rows and the training rows themselves -> (int32 [2, C, C] ON THE DEVICE: the
    validation and the train-on-train confusion matrices over ``labels``, labels).  Two launches, no host synchronisation"""
    y_train, y_val = np.asarray(y_train).reshape(-1), np.asarray(y_val).reshape(-1)
    labels = np.unique(np.concatenate([y_train, y_val]))
    knn = KNeighborsClassifier(n_neighbors).fit(X_train, y_train, classes=labels)
    C = int(labels.size)
    conf = torch.zeros(2, C, C, dtype=torch.int32, device=knn._X.device)
    if y_val.size:
        knn.classify(X_val, knn.class_index(y_val), conf[0])
    knn.classify(knn._X, knn._cls, conf[1])
    return conf, labels


def knn_confusions(X_train, y_train, X_val, y_val, n_neighbors=3):
    """``knn_confusions_device`` and its ONE device-to-host copy -> (int64 [2, C, C] numpy, labels)"""
    conf, labels = knn_confusions_device(X_train, y_train, X_val, y_val, n_neighbors)
    return conf.cpu().numpy().astype(np.int64), labels


def evaluate(train_graphs, val_graphs, model, n_neighbors=3, chunk=None):
    """The reference's ``evaluate()``: embed both sets, fit the k-NN classifier on the training embeddings, predict both sets -> the
    same dictionary (train_triplet.py:90-94): 'prec' (macro precision), 'recall' (macro recall), 'acc', 'F1' (micro) of the validation
    set and 'train acc'.  Both sets are ``{class: [graphs]}`` dictionaries (iteration order kept) or plain sequences; labels come from
    ``graph.graph['label']`` or ``data.y``.  After the embeddings exist nothing returns to the host but the two confusion matrices,
    in one copy; the metrics are numpy on those."""
    train, val = _flatten(train_graphs), _flatten(val_graphs)
    y_train, y_val = _labels(train), _labels(val)
    emb = embed_dataset(model, train + val, chunk)
    conf, _ = knn_confusions(emb[:len(train)], y_train, emb[len(train):], y_val, n_neighbors)
    result = metrics_from_confusion(conf[0])
    total = int(conf[1].sum())
    result["train acc"] = int(np.trace(conf[1])) / total if total else 0.0
    return result
