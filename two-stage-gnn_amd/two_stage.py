"""Stage two of the two-stage scheme: embed every graph of the train and validation sets and classify by k-nearest-neighbour on the
embeddings — the reference's ``evaluate()`` (Code/sage+gat+diffpool/train_triplet.py:36-101, Code/sag/train_triplet.py:34-73), which
runs one B = 1 forward per graph, copies every embedding to the host and fits sklearn's ``KNeighborsClassifier`` there.

Here the graphs go through the encoder in block-diagonal chunks (``embed_dataset``: the resident per-graph device pieces of
``resident.py``, per-graph statistics, so row i is the eval-mode B = 1 forward of graph i), the classifier is one
HIP launch per prediction (csrc/knn.hip: distances, selection, vote and confusion matrix) and ``evaluate`` copies two small confusion
matrices to the host, once.

The reference's other probe, ``evaluate_mlp()`` (train_triplet.py:105-183: a fresh three-layer MLP trained with one Adam step per
training embedding, then one forward per validation graph), is ``MLPProbe`` / ``evaluate_mlp`` at the end of this module: the whole
training loop is ONE launch of one workgroup (csrc/mlp_probe.hip), the predictions and their correct count a second one.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from . import _native as nat
from . import message_passing as mp
from . import resident as R


# ----------------------------------------------------------------------------- containers
def _flatten(graphs):
    """the reference's two call shapes -> a list: ``{class: [graphs]}`` dictionaries in iteration order (train_triplet.py:49-50) or any
    sequence / iterable of graphs (Code/sag: a loader of single graphs)"""
    if isinstance(graphs, dict):
        return [g for c in graphs.keys() for g in graphs[c]]
    return list(graphs)


def _is_dense(g):
    return isinstance(getattr(g, "graph", None), dict)


def _is_eigen_dict(g):
    """a bare ``.graph`` dict (what ``GraphSampler.__getitem__`` returns): only the EigenGCN route takes these"""
    return isinstance(g, dict) and "adj" in g


def _labels(graphs):
    """host labels of the graphs: ``graph.graph['label']`` or ``data.y`` (labels that live on the device come back in ONE copy)"""
    if not graphs:
        return np.zeros(0, dtype=np.int64)
    if _is_dense(graphs[0]) or _is_eigen_dict(graphs[0]):
        return np.asarray([np.asarray((g if isinstance(g, dict) else g.graph)["label"]).reshape(-1)[0] for g in graphs])
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
    try:
        model.eval()
        with R.per_graph_statistics(model), torch.no_grad():
            yield
    finally:
        model.train(training)


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
    g, x, xa, sizes = T.assemble([T.resident_graph(o, dev, cache) for o in graphs], dev)
    _, feat = model(x, g, sizes, assign_x=x if xa is None else xa)
    return feat


def _embed_net_chunk(tnet, graphs):
    """sag_layers.Net on a chunk: per-graph pooling and read-outs (Net has no batch-norm: this IS one forward per graph), the head on
    all rows of the chunk at once"""
    from . import pyg
    m = tnet.model
    r = tnet.readout(tnet.batch_of(graphs))
    if mp.mlp3_ok(r, m.lin1, m.lin2, m.lin3):
        return mp.mlp3_log_softmax(r, m.lin1, m.lin2, m.lin3, m.dropout_ratio, False)
    h = pyg.relu(mp.linear_oi(r, m.lin1.weight, m.lin1.bias))
    h = pyg.relu(mp.linear_oi(h, m.lin2.weight, m.lin2.bias))
    return F.log_softmax(mp.linear_oi(h, m.lin3.weight, m.lin3.bias), dim=-1)


def _embed_one(model, g, dev):
    """the reference's own call for one graph (train_triplet.py:52-59; Code/sag/train_triplet.py:45-47; an EigenGCN encoder:
    ``eigen_triplet.embed_one``, Code/eigengcn/train_triplet.py:42-78)"""
    from . import eigen_encoders as EE, eigen_triplet as ET
    if isinstance(model, EE.WavePoolingGcnEncoder):
        return ET.embed_one(model, g, dev)[0]
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
    again, and the reverse.  A ``gat_triplet.tripletnet`` (or a bare ``gat_encoders.DGATEncoderGraph`` when ``chunk`` is given) runs its
    GAT encoder on packed chunks with one ghost representative per graph, assembled from the same cache (default
    ``gat_triplet.DEFAULT_CHUNK`` graphs, at most the 1024 rows the encoder's fused head takes).

    An ``eigen_triplet.tripletnet`` or a bare ``eigen_encoders.WavePoolingGcnEncoder`` (its ``pool_sizes``, ``num_pool_matrix`` and
    ``num_pool_final_matrix`` say what the dicts must hold) runs in chunks of ``eigen_triplet.DEFAULT_CHUNK`` graphs: the chunk's
    ``EigenBatch`` is written from the graphs' resident pieces by one launch per 32 graphs (``eigen_triplet.assemble``, csrc/eigen_assemble.hip), the
    model runs once on it, row i is ``feat[0]`` of Code/eigengcn/train_triplet.py:77-78 for graph i.  Pass the LIST of graph objects
    (``.graph`` = {'adj', 'feats', 'num_nodes', 'adj_pool_i', 'num_nodes_i', 'pool_adj_i_j', 'label'}, what ``GraphSampler`` fills and
    ``TripletSampler`` hands out), not the reference's shuffled batch-1 ``DataLoader``: rows come back in the list's order, and the
    objects key the cache shared with the triplet step.  Bare ``.graph`` dicts are taken too and packed at every call (the sampler
    makes a new dict per access).  ValueError for mixed Nmax, mixed feature widths, a dict prepared for other L / J / Jf than the
    model's.  With ``TSGNN_TRIPLET_CACHE=0``, or more pooling levels than the assembler takes, every graph gets a call of its own
    on a one-graph ``EigenBatch`` (``eigen_triplet.embed_one``).

    ANY OTHER model (a bare GAT encoder without ``chunk``, a module of your own) gets a plain loop of B = 1 forwards with the rows
    kept on the device: correct, and not fast.  ``model`` may also be a ``tripletnet`` (its ``.model`` is used)."""
    from . import dense_encoders as E, gat_encoders as GE, gat_triplet as GT, sag_layers as S, sag_triplet as ST, triplet as T
    from . import eigen_encoders as EE, eigen_triplet as ET
    gat_chunks = isinstance(model, GT.tripletnet)             # (a bare GAT encoder takes the chunked path only when chunk= is given)
    if isinstance(model, (T.tripletnet, ST.tripletnet, GT.tripletnet, ET.tripletnet)):
        model = model.model
    graphs = _flatten(graphs)
    dev = _device_of(model)
    if chunk is not None and int(chunk) < 1:
        raise ValueError("chunk must be at least 1")
    rows = []
    with _eval_mode(model):
        if not graphs:
            return torch.zeros(0, 0, dtype=torch.float32, device=dev)
        if isinstance(model, EE.WavePoolingGcnEncoder):       # (a GcnEncoderGraph by inheritance: asked first)
            if dev.type == "cuda" and R.RESIDENT and len(model.pool_sizes) <= ET.max_levels():
                step = int(chunk) if chunk is not None else ET.DEFAULT_CHUNK
                cache = R.resident_cache(model)
                for i in range(0, len(graphs), step):
                    rows.append(ET.embed_chunk(model, graphs[i:i + step], dev, cache))
            else:
                rows = [_embed_one(model, g, dev).reshape(1, -1) for g in graphs]
        elif isinstance(model, E.GcnEncoderGraph) and dev.type == "cuda" and R.RESIDENT and _is_dense(graphs[0]):
            step = int(chunk) if chunk is not None else dense_chunk_limit(model)
            cache = R.resident_cache(model)
            for i in range(0, len(graphs), step):
                rows.append(_embed_dense_chunk(model, graphs[i:i + step], dev, cache))
        elif isinstance(model, GE.DGATEncoderGraph) and (gat_chunks or chunk is not None) and dev.type == "cuda" and R.RESIDENT \
                and _is_dense(graphs[0]):
            step = min(int(chunk) if chunk is not None else GT.DEFAULT_CHUNK, GT.HEAD_ROWS_MAX)
            cache = R.resident_cache(model)
            for i in range(0, len(graphs), step):
                rows.append(GT.embed_chunk(model, graphs[i:i + step], dev, cache))
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


def predict_dataset(graphs, model, chunk=None):
    """class index per graph, int32 on the model's device: the argmax (a tie to the lowest class) of ``model.map2_model`` on the
    graph's ``embed_dataset`` row.  For a final_dim "pretrain" encoder that row is ``out`` and the result the argmax of the reference's
    ``pred`` (train_triplet_pre_train.py:59-63).  A head of the MLP probe's shape (``post_train.make_head``) is ONE launch of
    ``tsgnn_mlp_probe_predict_f32``; any other ``map2_model`` is applied as torch modules"""
    from . import post_train as PT
    net = model.model if (hasattr(model, "model") and not hasattr(model, "map2_model")) else model
    emb = embed_dataset(model, graphs, chunk)
    n = int(emb.size(0))
    if n == 0:
        return torch.zeros(0, dtype=torch.int32, device=emb.device)
    layers = PT.head_layers(net)
    if layers is not None and emb.is_cuda:
        _, l1, l2, l3, slope = layers
        E, h1, h2, C = int(l1.in_features), int(l1.out_features), int(l2.out_features), int(l3.out_features)
        ps = [t.detach() for m in (l1, l2, l3) for t in (m.weight, m.bias)]
        if (E == emb.size(1) and nat.lib().tsgnn_mlp_probe_supported(E, h1, h2, C)
                and all(t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda for t in ps)):
            pred = torch.empty(n, dtype=torch.int32, device=emb.device)
            nat.call("mlp_probe_predict_f32", emb, emb.stride(0), n, E, h1, h2, C, *ps, slope, None, pred, None, None)
            return pred
    with _eval_mode(net):
        z = net.map2_model(emb)
    return (z == z.max(dim=1, keepdim=True).values).int().argmax(dim=1).int()      # (the first maximum: the lowest class)


def evaluate_pred(graphs, model, chunk=None):
    """The ``evaluate()`` of the 2stg+ post-training phase (train_triplet_pre_train.py:36-72): the argmax of ``pred`` per graph against
    ``graph.graph['label']`` -> {'prec' (macro), 'recall' (macro), 'acc', 'F1' (micro)}.  ``graphs``: a ``{class: [graphs]}`` dictionary
    (iteration order kept) or a sequence.  After the embeddings exist: one predict launch and ONE copy of the predictions to the
    host; the metrics are numpy on the confusion matrix."""
    graphs = _flatten(graphs)
    y = _labels(graphs).reshape(-1)
    pred = predict_dataset(graphs, model, chunk).cpu().numpy().astype(np.int64)
    labels = np.unique(np.concatenate([y.astype(np.int64), pred]))
    return metrics_from_confusion(confusion_matrix(y, pred, labels))


# ----------------------------------------------------------------------------- the MLP probe
def _probe_sizes(E, h1, h2, C):
    """element counts of W1, b1, W2, b2, W3, b3: the order of the flat parameter and moment buffers (and of the C ABI)"""
    return [h1 * E, h1, h2 * h1, h2, C * h2, C]


def _probe_views(flat, E, h1, h2, C):
    shapes = [(h1, E), (h1,), (h2, h1), (h2,), (C, h2), (C,)]
    out, o = [], 0
    for n, shp in zip(_probe_sizes(E, h1, h2, C), shapes):
        out.append(flat[o:o + n].view(shp))
        o += n
    return out


def mlp_probe_torch(X, cls, params, exp_avg, exp_avg_sq, step0, lr, betas, eps, negative_slope):
    """the fit kernel's semantics as a torch composition (tensors on the CPU, sizes ``tsgnn_mlp_probe_supported`` does not take): the
    reference's loop itself, one ``torch.optim.Adam`` step per row on that row's cross-entropy.  ``params`` (six tensors) and the
    moments (six views each, same order) are updated in place, ``step0`` steps lie behind them.  -> per-step losses [n]"""
    ps = [torch.nn.Parameter(t) for t in params]                       # (a Parameter shares its tensor's storage)
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps)
    for p, m, v in zip(ps, exp_avg, exp_avg_sq):
        opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m, "exp_avg_sq": v}
    losses = []
    target = cls.long()
    for i in range(X.size(0)):
        h = F.leaky_relu(F.linear(X[i], ps[0], ps[1]), negative_slope)
        h = F.leaky_relu(F.linear(h, ps[2], ps[3]), negative_slope)
        loss = F.cross_entropy(F.linear(h, ps[4], ps[5]).unsqueeze(0), target[i:i + 1])
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.detach())
    return torch.stack(losses) if losses else torch.zeros(0, device=X.device)


class MLPProbe:
    """The classifier of the reference's ``evaluate_mlp()``: ``Linear(E, h1) - LeakyReLU - Linear(h1, h2) - LeakyReLU - Linear(h2, C)``
    trained by ONE pass over the training rows, in row order, one ``torch.optim.Adam`` step per row on that row's cross-entropy.  On
    device tensors the pass is one launch of one workgroup (csrc/mlp_probe.hip) and ``fit`` never waits for the device; CPU tensors
    and sizes outside ``tsgnn_mlp_probe_supported`` take ``mlp_probe_torch``, the same loop written with torch.

    ``C = max(2, len(classes_))`` unless ``n_classes`` asks for more (the reference's last layer has two rows whatever the labels).
    ``X`` / ``Q``: what ``KNeighborsClassifier`` takes."""

    def __init__(self, hidden=(64, 32), n_classes=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, negative_slope=0.01):
        if len(hidden) != 2 or min(int(h) for h in hidden) < 1:
            raise ValueError("hidden must be two positive widths")
        if n_classes is not None and int(n_classes) < 2:
            raise ValueError("n_classes must be at least 2")
        self.hidden = (int(hidden[0]), int(hidden[1]))
        self.n_classes = None if n_classes is None else int(n_classes)
        self.lr, self.betas, self.eps, self.negative_slope = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(negative_slope)

    # ---- parameters
    def _initial(self, init, E, C):
        """six host tensors [out, in]: copies of ``init`` (an ``nn.Sequential`` of the reference's shape or its six tensors), or what the
        reference's ``nn.Linear(E, h1)``, ``nn.Linear(h1, h2)``, ``nn.Linear(h2, C)`` hold when constructed now, in that order, on the
        host (train_triplet.py:151-155 builds them there before ``.cuda()``: the same draws from torch's global generator)"""
        h1, h2 = self.hidden
        if init is None:
            lins = [torch.nn.Linear(E, h1), torch.nn.Linear(h1, h2), torch.nn.Linear(h2, C)]
            ts = [t for m in lins for t in (m.weight, m.bias)]
        elif isinstance(init, torch.nn.Module):
            lins = [m for m in init.modules() if isinstance(m, torch.nn.Linear)]
            if len(lins) != 3:
                raise ValueError("init must hold three Linear layers")
            ts = [t for m in lins for t in (m.weight, m.bias)]
        else:
            ts = list(init)
            if len(ts) != 6:
                raise ValueError("init must be six tensors: W1, b1, W2, b2, W3, b3")
        ts = [torch.as_tensor(t).detach().to("cpu", torch.float32) for t in ts]
        want = [(h1, E), (h1,), (h2, h1), (h2,), (C, h2), (C,)]
        if [tuple(t.shape) for t in ts] != want:
            raise ValueError("initial parameters have shapes %s, expected %s" % ([tuple(t.shape) for t in ts], want))
        return ts

    def _dims(self):
        return (self._E,) + self.hidden + (self._C,)

    def kernel_ok(self):
        return bool(self._flat.is_cuda and nat.lib().tsgnn_mlp_probe_supported(*self._dims()))

    # ---- training
    def fit(self, X, y, classes=None, init=None):
        """one pass over the rows of ``X`` from fresh parameters (``init``, never written; default: the reference's own construction
        under torch's global generator) and zero moments.  ``y`` / ``classes``: as ``KNeighborsClassifier.fit``"""
        yh = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        yh = yh.reshape(-1)
        X = _rows16(_as_matrix(X))
        if X.size(0) != yh.size:
            raise ValueError("X has %d rows, y has %d labels" % (X.size(0), yh.size))
        if X.size(0) < 1 or X.size(1) < 1:
            raise ValueError("fit needs at least one row and one column")
        self.classes_ = np.unique(yh) if classes is None else np.asarray(classes)
        self._y_tensor = isinstance(y, torch.Tensor)
        self._E = int(X.size(1))
        self._C = max(2, int(self.classes_.size), self.n_classes or 0)
        host = torch.cat([t.reshape(-1) for t in self._initial(init, self._E, self._C)])
        self._flat = _upload(host.numpy(), X.device) if X.is_cuda else host.clone()
        self._params = _probe_views(self._flat, *self._dims())
        self._exp_avg, self._exp_avg_sq = torch.zeros_like(self._flat), torch.zeros_like(self._flat)
        self._step = 0
        return self._steps(X, yh)

    def partial_fit(self, X, y):
        """continue with the rows of ``X`` from the kept parameters, moments and step count: ``fit(X[:h])`` then ``partial_fit(X[h:])``
        is ``fit(X)``, bit for bit.  Labels must be in ``classes_``"""
        if not hasattr(self, "_flat"):
            raise RuntimeError("partial_fit continues a fit: call fit first")
        yh = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        X = _rows16(_as_matrix(X, self._flat.device))
        if X.size(1) != self._E or X.size(0) != yh.size:
            raise ValueError("rows of %d columns with %d labels; fitted on %d columns" % (X.size(1), yh.size, self._E))
        return self._steps(X, yh.reshape(-1))

    def _steps(self, X, yh):
        n = int(X.size(0))
        if n == 0:
            self.losses_ = torch.zeros(0, device=X.device)
            return self
        cls = self.class_index(yh)
        if self.kernel_ok():
            self.losses_ = torch.empty(n, dtype=torch.float32, device=X.device)
            E, h1, h2, C = self._dims()
            nat.call("mlp_probe_fit_f32", X, X.stride(0), cls, n, E, h1, h2, C, *self._params, self._exp_avg, self._exp_avg_sq,
                     self._step, self.lr, self.betas[0], self.betas[1], self.eps, self.negative_slope, self.losses_)
        else:
            dims = self._dims()
            self.losses_ = mlp_probe_torch(X, cls, self._params, _probe_views(self._exp_avg, *dims), _probe_views(self._exp_avg_sq, *dims),
                                           self._step, self.lr, self.betas, self.eps, self.negative_slope)
        self._step += n
        return self

    def class_index(self, labels, strict=True):
        """host labels -> int32 tensor (on the parameters' device) of their positions in ``classes_``; a label that is not in
        ``classes_`` raises, or with ``strict=False`` becomes -1 (a class no prediction equals)"""
        labels = np.asarray(labels).reshape(-1)
        pos = np.searchsorted(self.classes_, labels)
        bad = (pos >= self.classes_.size) | (self.classes_[np.minimum(pos, self.classes_.size - 1)] != labels) if labels.size else np.zeros(0, bool)
        if strict and bad.any():
            raise ValueError("a label is not in classes_")
        return _upload(np.where(bad, -1, pos).astype(np.int32), self._flat.device)

    # ---- prediction
    def forward(self, Q, query_class=None, correct=None, logits=False):
        """-> (pred int32 [nq]: positions in ``classes_`` (the argmax of the logits, a tie to the lowest class), logits [nq, C] or None);
        with ``query_class`` (int32 positions) and ``correct`` (int32 [1] on the device): ``correct[0] += 1`` per row predicted right.
        ONE launch, nothing copied to the host"""
        dev = self._flat.device
        Q = _as_matrix(Q, dev)
        if Q.size(1) != self._E:
            raise ValueError("query rows have %d columns, training rows %d" % (Q.size(1), self._E))
        nq, C = int(Q.size(0)), self._C
        if nq == 0:
            return torch.zeros(0, dtype=torch.int32, device=dev), (torch.zeros(0, C, device=dev) if logits else None)
        if self.kernel_ok():
            Q = _rows16(Q)
            pred = torch.empty(nq, dtype=torch.int32, device=dev)
            out = torch.empty(nq, C, dtype=torch.float32, device=dev) if logits else None
            count = correct is not None and query_class is not None
            E, h1, h2, _ = self._dims()
            nat.call("mlp_probe_predict_f32", Q, Q.stride(0), nq, E, h1, h2, C, *self._params, self.negative_slope, out, pred,
                     query_class if count else None, correct if count else None)
            return pred, out
        p = self._params
        h = F.leaky_relu(F.linear(Q, p[0], p[1]), self.negative_slope)
        h = F.leaky_relu(F.linear(h, p[2], p[3]), self.negative_slope)
        out = F.linear(h, p[4], p[5])
        pred = (out == out.max(dim=1, keepdim=True).values).int().argmax(dim=1).int()      # (the first maximum: the lowest class)
        if correct is not None and query_class is not None:
            correct += (pred == query_class.to(dev)).sum().to(correct.dtype)
        return pred, (out if logits else None)

    def decision_function(self, Q):
        """logits [nq, C]: a tensor on Q's device for a tensor, else a numpy array"""
        out = self.forward(Q, logits=True)[1]
        return out.to(Q.device) if isinstance(Q, torch.Tensor) else out.cpu().numpy()

    def _label_table(self):
        """classes_, continued past its end when the last layer has more rows than there are labels (a row nobody was trained
        towards can still win): those read as max(classes_) + 1, + 2, ..."""
        extra = self._C - int(self.classes_.size)
        if extra <= 0:
            return self.classes_
        return np.concatenate([self.classes_, (self.classes_.max() + 1 + np.arange(extra)).astype(self.classes_.dtype)])

    def predict(self, Q):
        """labels of the rows of ``Q`` with the dtype of ``y``: a tensor on Q's device for a tensor, else a numpy array"""
        pred = self.forward(Q)[0]
        if isinstance(Q, torch.Tensor):
            return _upload(self._label_table(), pred.device)[pred.long()].to(Q.device)
        return self._label_table()[pred.cpu().numpy()]

    def correct_count(self, Q, y, correct=None):
        """-> int32 [1] on the device: rows of ``Q`` whose prediction is their label in ``y`` (a label outside ``classes_`` counts as
        wrong), added to ``correct`` when given.  One launch, no copy to the host"""
        yh = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        if correct is None:
            correct = torch.zeros(1, dtype=torch.int32, device=self._flat.device)
        self.forward(Q, self.class_index(yh, strict=False), correct)
        return correct

    def score(self, Q, y):
        """accuracy on (Q, y): one launch and ONE copy to the host"""
        n = len(Q)
        return int(self.correct_count(Q, y).cpu()) / n if n else 0.0

    def module(self):
        """an ``nn.Sequential`` of the reference's shape holding (copies of) the trained parameters, on their device"""
        E, h1, h2, C = self._dims()
        seq = torch.nn.Sequential(torch.nn.Linear(E, h1), torch.nn.LeakyReLU(self.negative_slope), torch.nn.Linear(h1, h2),
                                  torch.nn.LeakyReLU(self.negative_slope), torch.nn.Linear(h2, C)).to(self._flat.device)
        with torch.no_grad():
            for lin, (w, b) in zip((seq[0], seq[2], seq[4]), zip(self._params[0::2], self._params[1::2])):
                lin.weight.copy_(w)
                lin.bias.copy_(b)
        return seq


def evaluate_mlp(train_graphs, val_graphs, model, hidden=(64, 32), n_classes=None, init=None, chunk=None, probe=None):
    """The reference's ``evaluate_mlp()`` (train_triplet.py:105-183): embed both sets, train the probe on the training embeddings in
    dataset order (one Adam step per graph), predict the validation set -> ``{'acc': ...}``.  Containers and labels as ``evaluate``.
    After the embeddings exist: one fit launch, one predict launch, ONE copy to the host (the correct count).

    accuracy count: intent, not the reference's arithmetic.  The reference adds ``pred.eq(torch.Tensor(val_labels[i]))``, and
    ``torch.Tensor(int)`` is an UNINITIALISED tensor of that length (empty for label 0), so its printed accuracy is not a function of
    its predictions.  Here a graph counts when its prediction equals its label; a validation label the training set does not have
    counts as wrong.  Everything up to the predictions is the reference's."""
    train, val = _flatten(train_graphs), _flatten(val_graphs)
    y_train, y_val = _labels(train), _labels(val)
    emb = embed_dataset(model, train + val, chunk)
    probe = MLPProbe(hidden, n_classes) if probe is None else probe
    probe.fit(emb[:len(train)], y_train, init=init)
    return {"acc": probe.score(emb[len(train):], y_val)}
