"""EigenPooling (Code/eigengcn): host coarsening, the device-side batch of a mini-batch, and the pooling operator X' = P^T Z.

The reference (coarsen_pooling_with_last_eigen_padding.py, graph_sampler.py) stores every pooling matrix as a dense padded
``[B, Nmax, Nmax]`` tensor per eigenvector index and multiplies with ``torch.matmul``.  P is block-sparse: every node lies in
exactly one cluster, so P^T Z is a segmented weighted row sum.  Here a level is held compactly:

* ``cluster_of[row]`` (int32, -1 for a row that adds nothing) and ``coef[row, J]`` (the row's entries u_j(v) of the J matrices),
* the rows grouped into buckets, ``bptr`` / ``members``: bucket gp1[b] + b = graph b's unassigned rows, bucket c + b + 1 = the
  members of cluster c of graph b (rows ascending inside a bucket),
* the pooled graph as a weighted ``GraphBatch`` in the packed layout with the usual Nmax ghost-slot rows.

The pooling and the max readout of the rows it reads are one launch forward and one backward (csrc/eigen_pool.hip).
"""
import weakref

import numpy as np
import torch

from . import _native as nat
from . import message_passing as mp
from .graph import GraphBatch, exclusive_scan
from .resident import concat_csr

N_POOL = 5          # pooling matrices per level (the reference hard-codes num_nodes_in_largest_clusters = 5)
N_FINAL = 4         # final matrices (num_nodes_before_final = 4)


# ----------------------------------------------------------------------------- host coarsening
def laplacian(W, normalize=False):
    """graph.py:117-135 on a dense float64 [.., n, n] stack: D - W, or I - D^-1/2 W D^-1/2 (d += spacing(0))."""
    d = W.sum(axis=-2)
    if not normalize:
        return d[..., :, None] * np.eye(W.shape[-1]) - W
    d = 1.0 / np.sqrt(d + np.spacing(np.array(0, W.dtype)))
    return np.eye(W.shape[-1]) - d[..., :, None] * W * d[..., None, :]


def _signed_padded(U, count):
    """first `count` eigenvectors (columns) with the reference's sign rule (negate when the entry at the first node is negative) and
    padding rule (indices >= n repeat column n - 1).  U: [.., n, n] -> [.., n, count]"""
    n = U.shape[-1]
    idx = np.minimum(np.arange(count), n - 1)
    V = U[..., :, idx]
    sign = np.where(V[..., :1, :] < 0, -1.0, 1.0)
    return V * sign


def _spectral_labels(A, k, random_state):
    try:
        from sklearn.cluster import SpectralClustering
    except ImportError as e:           # pragma: no cover - depends on the environment
        raise ImportError("coarsen(labels=None) clusters with sklearn.cluster.SpectralClustering, which is not importable; "
                          "pass the cluster labels instead") from e
    sc = SpectralClustering(n_clusters=k, affinity="precomputed", n_init=10, random_state=random_state)
    return np.asarray(sc.fit(np.asarray(A)).labels_, dtype=np.int64)


def coarsen(adj, pool_sizes, normalize=False, labels=None, random_state=None):
    """Graphs(adj, pool_sizes).coarsening_pooling(normalize) of the reference, vectorised.

    adj: dense or scipy [n, n] adjacency.  labels: None (SpectralClustering, as the reference), a list with one label array per
    level, or a callable ``labels(A_level, n_clusters, level) -> int[n_level]``.
    Returns None for a graph the reference rejects (a singleton cluster, or a one-node last coarsened graph), else a dict:
    ``graphs`` [A_0 .. A_L] (float64 dense), ``labels`` [L] int64, ``coef`` [L] float64 [n_i, 5] (row v: the entries of the 5
    pooling matrices in its cluster's column), ``final`` float64 [n_L, 4]."""
    A = np.asarray(adj.todense() if hasattr(adj, "todense") else adj, dtype=np.float64)
    graphs, labs, coefs = [A], [], []
    for level, ps in enumerate(pool_sizes):
        n = A.shape[0]
        k = max(1, int(n / ps))
        if labels is None:
            lab = _spectral_labels(A, k, random_state)
        elif callable(labels):
            lab = np.asarray(labels(A, k, level), dtype=np.int64)
        else:
            lab = np.asarray(labels[level], dtype=np.int64)
        if lab.shape != (n,) or lab.min() < 0:
            raise ValueError("level %d: labels must be %d non-negative cluster ids" % (level, n))
        K = int(lab.max()) + 1
        cnt = np.bincount(lab, minlength=K)
        if (cnt == 0).any():
            raise ValueError("level %d: cluster ids must be 0..K-1 without gaps" % level)
        if (cnt == 1).any():
            return None                                    # a singleton cluster: the reference returns -1
        coef = np.zeros((n, N_POOL))
        for s in np.unique(cnt):                           # one batched eigh per cluster size
            cl = np.nonzero(cnt == s)[0]
            mem = np.stack([np.nonzero(lab == c)[0] for c in cl])          # [k, s] members in node order
            W = A[mem[:, :, None], mem[:, None, :]]
            _, U = np.linalg.eigh(laplacian(W, normalize))
            coef[mem.reshape(-1)] = _signed_padded(U, N_POOL).reshape(-1, N_POOL)
        Om = np.zeros((n, K))
        Om[np.arange(n), lab] = 1.0
        A = Om.T @ A @ Om
        np.fill_diagonal(A, 0.0)                           # Omega^T A_ext Omega: intra-cluster edges removed
        graphs.append(A)
        labs.append(lab)
        coefs.append(coef)
    if A.shape[0] <= 1:
        return None
    _, U = np.linalg.eigh(laplacian(A, normalize))
    return {"graphs": graphs, "labels": labs, "coef": coefs, "final": _signed_padded(U, N_FINAL)}


def l1_normalize(coef, labels=None):
    """graph_sampler.py:150-175 (--norm l1): every pooling column divided by its L1 norm (a column = a cluster; the final matrices: the
    whole graph).  coef [n, J]; labels None = one column."""
    coef = np.asarray(coef, dtype=np.float64)
    lab = np.zeros(coef.shape[0], dtype=np.int64) if labels is None else np.asarray(labels)
    norm = np.zeros((int(lab.max()) + 1, coef.shape[1]))
    np.add.at(norm, lab, np.abs(coef))
    d = norm[lab]
    return np.where(d > 0, coef / np.where(d > 0, d, 1.0), 0.0)


# ----------------------------------------------------------------------------- device-side batch
class EigenLevel:
    """one pooling level on the device: rows of the level it pools -> rows of ``g`` (the pooled graph)."""
    __slots__ = ("g", "cluster_of", "coef", "bptr", "members", "J")


class EigenBatch:
    """a mini-batch for WavePoolingGcnEncoder: ``g0`` (level 0), ``levels`` (EigenLevel per pooling), ``final_coef``
    [rows of the last level, Jf] (or None), ``nmax``."""

    def __init__(self, g0, levels, final_coef, nmax):
        self.g0, self.levels, self.final_coef, self.nmax = g0, levels, final_coef, int(nmax)

    @property
    def B(self):
        return self.g0.B


def _csr_batch(mats, nmax, device):
    """packed-layout weighted GraphBatch of dense [n_b, n_b] host matrices: columns ascending, val = the weights, as
    GraphBatch.from_dense lays out the same padded tensor"""
    sizes = np.asarray([m.shape[0] for m in mats], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    rows, cols, vals = [], [], []
    for b, m in enumerate(mats):
        r, c = np.nonzero(m)
        rows.append(r + offs[b])
        cols.append(c + offs[b])
        vals.append(m[r, c])
    r = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    c = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    v = np.concatenate(vals) if vals else np.zeros(0)
    n_rows = int(offs[-1])
    rowptr = np.zeros(n_rows + nmax + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=n_rows), out=rowptr[1:n_rows + 1])
    rowptr[n_rows + 1:] = rowptr[n_rows]
    col = torch.from_numpy(np.ascontiguousarray(c.astype(np.int32) if c.size else np.zeros(1, np.int32))).to(device)
    val = torch.from_numpy(np.ascontiguousarray(v.astype(np.float32) if v.size else np.zeros(1, np.float32))).to(device)
    g = GraphBatch.from_csr(torch.from_numpy(rowptr).to(device), col, val, sizes, nmax, assume_symmetric=False)
    g.nnz = int(c.size)                     # (an edgeless batch keeps a one-entry buffer, as GraphBatch.from_dense does)
    return g


def _bucket_key(cluster_of, gp0, gp1):
    """tsgnn_eigen_pool_from_dense_f32's bucket of every row (host side): gp1[b] + b if unassigned, cluster_of + b + 1 otherwise"""
    graph = np.repeat(np.arange(gp0.size - 1), np.diff(gp0))
    return np.where(cluster_of >= 0, cluster_of + graph + 1, gp1[graph] + graph).astype(np.int64)


def collate(results, nmax, num_pool_matrix, num_pool_final_matrix=0, norm=None, device=None):
    """EigenBatch of a mini-batch of coarsen() results (none of them None).  norm='l1': graph_sampler.py's --norm l1."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    J, Jf = int(num_pool_matrix), int(num_pool_final_matrix)
    if not 1 <= J <= N_POOL or not 0 <= Jf <= N_FINAL:
        raise ValueError("num_pool_matrix must lie in [1, 5] and num_pool_final_matrix in [0, 4]")
    L = len(results[0]["labels"])
    g0 = _csr_batch([r["graphs"][0] for r in results], nmax, device)
    levels = []
    for i in range(L):
        sizes0 = np.asarray([r["graphs"][i].shape[0] for r in results], dtype=np.int64)
        sizes1 = np.asarray([r["graphs"][i + 1].shape[0] for r in results], dtype=np.int64)
        gp0 = np.concatenate([[0], np.cumsum(sizes0)])
        gp1 = np.concatenate([[0], np.cumsum(sizes1)])
        coef = []
        for r in results:
            c = r["coef"][i][:, :J]
            coef.append(l1_normalize(c, r["labels"][i]) if norm == "l1" else c)
        coef = np.concatenate(coef).astype(np.float32)
        clus = np.concatenate([r["labels"][i] + gp1[b] for b, r in enumerate(results)]).astype(np.int64)
        clus[(coef == 0).all(axis=1)] = -1                 # adds nothing (what the dense conversion decides too)
        key = _bucket_key(clus, gp0, gp1)
        members = np.argsort(key, kind="stable").astype(np.int32)          # rows ascending inside a bucket
        bptr = np.zeros(int(gp1[-1]) + len(results) + 1, dtype=np.int64)
        np.cumsum(np.bincount(key, minlength=bptr.size - 1), out=bptr[1:])
        lv = EigenLevel()
        lv.g = _csr_batch([r["graphs"][i + 1] for r in results], nmax, device)
        lv.cluster_of = torch.from_numpy(clus.astype(np.int32)).to(device)
        lv.coef = torch.from_numpy(np.ascontiguousarray(coef)).to(device)
        lv.bptr = torch.from_numpy(bptr.astype(np.int32)).to(device)
        lv.members = torch.from_numpy(members).to(device)
        lv.J = J
        levels.append(lv)
    fc = None
    if Jf:
        f = [l1_normalize(r["final"][:, :Jf]) if norm == "l1" else r["final"][:, :Jf] for r in results]
        fc = torch.from_numpy(np.ascontiguousarray(np.concatenate(f).astype(np.float32))).to(device)
    return EigenBatch(g0, levels, fc, nmax)


def dense_inputs(results, nmax, num_pool_matrix, num_pool_final_matrix=0, norm=None):
    """the reference's padded inputs of the same mini-batch (graph_sampler.py:102-175): (adj [B,N,N], adj_pooled_list,
    batch_num_nodes, batch_num_nodes_list, pool_matrices_dic), float64 CPU tensors"""
    B, L = len(results), len(results[0]["labels"])
    adj = np.zeros((B, nmax, nmax))
    pooled = [np.zeros((B, nmax, nmax)) for _ in range(L)]
    pm = {i: [np.zeros((B, nmax, nmax)) for _ in range(num_pool_matrix)] for i in range(L)}
    if num_pool_final_matrix:
        pm[L] = [np.zeros((B, nmax, nmax)) for _ in range(num_pool_final_matrix)]
    for b, r in enumerate(results):
        n0 = r["graphs"][0].shape[0]
        adj[b, :n0, :n0] = r["graphs"][0]
        for i in range(L):
            n, k = r["graphs"][i].shape[0], r["graphs"][i + 1].shape[0]
            pooled[i][b, :k, :k] = r["graphs"][i + 1]
            for j in range(num_pool_matrix):
                col = r["coef"][i][:, j]
                P = np.zeros((n, k))
                P[np.arange(n), r["labels"][i]] = col
                if norm == "l1":
                    s = np.abs(P).sum(axis=0)
                    P = np.where(s > 0, P / np.where(s > 0, s, 1.0), 0.0)
                pm[i][j][b, :n, :k] = P
        for j in range(num_pool_final_matrix):
            col = r["final"][:, j:j + 1]
            pm[L][j][b, :col.shape[0], :1] = l1_normalize(col) if norm == "l1" else col
    t = torch.from_numpy
    return (t(adj), [t(p) for p in pooled], [r["graphs"][0].shape[0] for r in results],
            [[r["graphs"][i + 1].shape[0] for r in results] for i in range(L)], {i: [t(p) for p in v] for i, v in pm.items()})


# ----------------------------------------------------------------------------- dense reference inputs -> EigenBatch (cached)
_dense_cache = {}


def _key_of(t):
    return (t.data_ptr(), tuple(t.shape), t._version, str(t.device))


def _pool_operand(mats, count, B, nmax, device, what):
    """[count, B, nmax, nmax] float32 stack of the first ``count`` padded pooling matrices; every shape is checked, since the
    conversion launch indexes the stack with these sizes"""
    mats = list(mats)
    if len(mats) < count:
        raise ValueError("%s: %d pooling matrices given, %d needed" % (what, len(mats), count))
    for m in mats[:count]:
        if tuple(m.shape) != (B, nmax, nmax):
            raise ValueError("%s: a pooling matrix of shape %s, expected %s" % (what, tuple(m.shape), (B, nmax, nmax)))
    return torch.stack([m.to(device, torch.float32) for m in mats[:count]]).contiguous()


def level_from_dense(P, g, g1, bad):
    """EigenLevel pooling the rows of ``g`` into the rows of ``g1`` from P [J, B, nmax, nmax] (_pool_operand): the rows' clusters,
    coefficients and bucket keys (tsgnn_eigen_pool_from_dense_f32), the bucket CSR by tsgnn_coo_count / tsgnn_coo_fill.
    ``bad`` (int32 [1], device) is set when an entry lies beyond its graph's pooled node count."""
    dev, J, R = P.device, P.size(0), g.n_rows
    lv = EigenLevel()
    lv.g, lv.J = g1, J
    lv.cluster_of = torch.empty(max(R, 1), dtype=torch.int32, device=dev)
    lv.coef = torch.empty(max(R, 1), J, dtype=torch.float32, device=dev)
    key = torch.empty(max(R, 1), dtype=torch.int64, device=dev)
    nat.call("eigen_pool_from_dense_f32", P, J, g.B, g.nmax, g.row_graph, g.row_slot, g1.graph_ptr, R, 0, lv.cluster_of, lv.coef,
             key, bad)
    nb = g1.n_rows + g.B                       # buckets: per graph its unassigned rows, then its clusters
    cnt = torch.zeros(nb, dtype=torch.int32, device=dev)
    nat.call("coo_count", key, R, nb, cnt, bad)
    lv.bptr = exclusive_scan(cnt)
    lv.members = torch.empty(max(R, 1), dtype=torch.int32, device=dev)
    nat.call("coo_fill", key, torch.arange(max(R, 1), dtype=torch.int64, device=dev), R, nb, max(R, 1), lv.bptr,
             torch.empty(nb, dtype=torch.int32, device=dev), lv.members, torch.empty(max(R, 1), dtype=torch.int32, device=dev), None)
    return lv


def batch_from_dense(adj, batch_num_nodes, adj_pooled_list, batch_num_nodes_list, pool_matrices_dic, J, Jf, L):
    """the reference's padded tensors -> EigenBatch on the GPU.  Cached on the identity and version of every input tensor."""
    from .dense_encoders import _batch_from_dense
    if batch_num_nodes is None:
        raise ValueError("WavePoolingGcnEncoder needs batch_num_nodes (the reference masks level 0 with it)")
    if adj.dim() != 3 or adj.size(1) != adj.size(2):
        raise ValueError("adj must be [B, Nmax, Nmax]")
    B, nmax = adj.size(0), adj.size(1)
    if len(adj_pooled_list) < L or len(batch_num_nodes_list) < L or any(i not in pool_matrices_dic for i in range(L + (1 if Jf else 0))):
        raise ValueError("the pooled inputs cover fewer levels than the model's %d (+ the final matrices)" % L)
    for i in range(L):
        if tuple(adj_pooled_list[i].shape) != (B, nmax, nmax):
            raise ValueError("adj_pooled_list[%d] has shape %s, expected %s" % (i, tuple(adj_pooled_list[i].shape), (B, nmax, nmax)))
    dev = torch.device("cuda", torch.cuda.current_device())
    ts = [adj] + [adj_pooled_list[i] for i in range(L)] + [p for i in range(L) for p in list(pool_matrices_dic[i])[:J]]
    if Jf:
        ts += list(pool_matrices_dic[L])[:Jf]
    sizes_all = (tuple(int(s) for s in np.asarray(batch_num_nodes).reshape(-1)),
                 tuple(tuple(int(s) for s in np.asarray(batch_num_nodes_list[i]).reshape(-1)) for i in range(L)))
    key = (tuple(_key_of(t) for t in ts), sizes_all, J, Jf, L)
    hit = _dense_cache.get(key)
    if hit is not None and hit[0]() is adj:
        return hit[1]
    adj_d = adj.to(dev, torch.float32)
    g = _batch_from_dense(adj_d, np.asarray(sizes_all[0]), "packed") if adj_d is adj else \
        GraphBatch.from_dense(adj_d, sizes=np.asarray(sizes_all[0]), layout="packed")
    g0 = g
    levels = []
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(L):
        g1 = GraphBatch.from_dense(adj_pooled_list[i].to(dev, torch.float32), sizes=np.asarray(sizes_all[1][i]), layout="packed")
        P = _pool_operand(pool_matrices_dic[i], J, B, nmax, dev, "pool_matrices_dic[%d]" % i)
        levels.append(level_from_dense(P, g, g1, bad))
        g = g1
    fc = None
    if Jf:
        P = _pool_operand(pool_matrices_dic[L], Jf, B, nmax, dev, "pool_matrices_dic[%d] (final)" % L)
        fc = torch.empty(max(g.n_rows, 1), Jf, dtype=torch.float32, device=dev)
        nat.call("eigen_pool_from_dense_f32", P, Jf, g.B, nmax, g.row_graph, g.row_slot, None, g.n_rows, 1,
                 torch.empty(max(g.n_rows, 1), dtype=torch.int32, device=dev), fc, None, bad)
    if int(bad.item()):
        raise ValueError("a pooling matrix has an entry in a column beyond its graph's pooled node count")
    eb = EigenBatch(g0, levels, fc, nmax)
    if len(_dense_cache) > 4:
        _dense_cache.clear()
    _dense_cache[key] = (weakref.ref(adj), eb)
    return eb


# ----------------------------------------------------------------------------- EigenBatches -> one EigenBatch, on the device
def _concat(gs, nmax):
    """block-diagonal packed GraphBatch of the graphs of several packed GraphBatches (``resident.concat_csr``: device-side
    concatenations, no host synchronisation)"""
    rowptr, col, val, nnz, sym = concat_csr([(q.rowptr, q.col, q.val, q.n_rows, q.nnz, q.symmetric) for q in gs], nmax + 1)
    g = GraphBatch.from_csr(rowptr, col, val, np.concatenate([np.asarray(q.sizes, dtype=np.int64) for q in gs]), nmax, assume_symmetric=sym)
    g.nnz = nnz
    return g


def concat_batches(batches):
    """One EigenBatch holding the graphs of several (e.g. cached one-graph batches -> a mini-batch), in order.  Everything is
    concatenated on the device: rows and clusters of a later batch are offset by the rows before them, and since the bucket order is
    per graph [unassigned rows, clusters ...] the bucket lists concatenate with a running offset.  The result equals ``collate`` /
    ``batch_from_dense`` of all the graphs at once.  The batches must share nmax, the number of levels and of pooling matrices."""
    batches = list(batches)
    first = batches[0]
    nmax, L = first.nmax, len(first.levels)
    for eb in batches:
        if eb.nmax != nmax or len(eb.levels) != L or (eb.final_coef is None) != (first.final_coef is None) or \
                any(a.J != b.J for a, b in zip(eb.levels, first.levels)) or \
                (eb.final_coef is not None and eb.final_coef.size(1) != first.final_coef.size(1)):
            raise ValueError("concat_batches: the batches must share Nmax, the number of levels and of pooling matrices")
    prev = [eb.g0 for eb in batches]
    g0 = _concat(prev, nmax)
    dev = g0.device
    levels = []
    for i in range(L):
        lvs = [eb.levels[i] for eb in batches]
        clus, coef, mem, bp, r0, c0 = [], [], [], [], 0, 0
        for q, lv in zip(prev, lvs):
            R, K = q.n_rows, lv.g.n_rows
            c = lv.cluster_of[:R]
            clus.append(torch.where(c >= 0, c + c0, c) if c0 else c)
            coef.append(lv.coef[:R])
            m = lv.members[:R]
            mem.append(m + r0 if r0 else m)
            b = lv.bptr[:K + q.B]                      # (K + B buckets: the closing entry is the next batch's first)
            bp.append(b + r0 if r0 else b)
            r0 += R
            c0 += K
        bp.append(torch.full((1,), r0, dtype=torch.int32, device=dev))
        out = EigenLevel()
        out.g, out.J = _concat([lv.g for lv in lvs], nmax), lvs[0].J
        out.cluster_of, out.coef, out.members, out.bptr = torch.cat(clus), torch.cat(coef), torch.cat(mem), torch.cat(bp)
        levels.append(out)
        prev = [lv.g for lv in lvs]
    fc = torch.cat([eb.final_coef[:q.n_rows] for eb, q in zip(batches, prev)]) if first.final_coef is not None else None
    return EigenBatch(g0, levels, fc, nmax)


# ----------------------------------------------------------------------------- the operator
class _EigenPool(torch.autograd.Function):
    """(pooled rows, [readout of z]) or, final: (max(P^T z, 0) [B, J*C], [readout of z]); see tsgnn_eigen_pool_fwd_f32"""

    @staticmethod
    def forward(ctx, z, g, lvl, coef, final, ghost_mode, want_ro, into, into_final):
        if z.stride(1) != 1:
            z = z.contiguous()
        C = z.size(1)
        J = coef.size(1)
        dev = z.device
        ro = arg = None
        if want_ro:
            ro = into.t if into is not None else torch.empty(g.B, C, dtype=torch.float32, device=dev)
            arg = torch.empty(g.B, C, dtype=torch.int32, device=dev)
        if final:
            out = into_final.t if into_final is not None else torch.empty(g.B, J * C, dtype=torch.float32, device=dev)
            fsum = torch.empty(g.B, J * C, dtype=torch.float32, device=dev)
            nat.call("eigen_pool_fwd_f32", z, z.stride(0), C, g.graph_ptr, g.B, g.nmax, g.n_rows, ghost_mode, None, None, None, coef, J,
                     1, out, out.stride(0), 0, 0, fsum, ro, ro.stride(0) if ro is not None else 0, arg)
            ctx.save_for_backward(coef, fsum, arg)
        else:
            g1 = lvl.g
            out = torch.empty(g1.total_rows, J * C, dtype=torch.float32, device=dev)
            # a capacity batch (eigen_stream.py): g1.n_rows is a capacity, and the launch also zeroes the padding rows behind the
            # batch's own clusters — the pooled level's stack forms X^T dY over every row of `out`
            nat.call("eigen_pool_fwd_cap_f32" if getattr(g1, "capacity", False) else "eigen_pool_fwd_f32", z, z.stride(0), C, g.graph_ptr, g.B, g.nmax, g.n_rows, ghost_mode, g1.graph_ptr, lvl.bptr,
                     lvl.members, coef, J, 0, out, out.stride(0), g1.n_rows, g1.n_ghost, None, ro, ro.stride(0) if ro is not None else 0, arg)
            ctx.save_for_backward(coef, lvl.cluster_of, arg)
        ctx.g, ctx.final, ctx.ghost_mode, ctx.C, ctx.J, ctx.rows = g, final, ghost_mode, C, J, z.size(0)
        ctx.out_shape = tuple(out.shape)
        ctx.set_materialize_grads(False)
        return (out, ro) if want_ro else out

    @staticmethod
    def backward(ctx, dout, dro=None):
        g, C, J = ctx.g, ctx.C, ctx.J
        coef, aux, arg = ctx.saved_tensors
        dev = coef.device
        if dout is None:
            dout = torch.zeros(ctx.out_shape, dtype=torch.float32, device=dev)
        if dout.stride(1) != 1:
            dout = dout.contiguous()
        if dro is not None:
            dro = mp.readout_dout_in_place(dro)
        dz = torch.empty(ctx.rows, C, dtype=torch.float32, device=dev)
        if ctx.final:
            nat.call("eigen_pool_bwd_f32", dout, dout.stride(0), aux, None, g.row_graph, coef, J, C, dro,
                     dro.stride(0) if dro is not None else 0, arg if dro is not None else None, g.B, g.nmax, g.n_rows,
                     ctx.ghost_mode, 1, dz, dz.stride(0), ctx.rows)
        else:
            nat.call("eigen_pool_bwd_f32", dout, dout.stride(0), None, aux, g.row_graph, coef, J, C, dro,
                     dro.stride(0) if dro is not None else 0, arg if dro is not None else None, g.B, g.nmax, g.n_rows,
                     ctx.ghost_mode, 0, dz, dz.stride(0), ctx.rows)
        return dz, None, None, None, None, None, None, None, None


def eigen_pool(z, g, lvl, ghost_mode, want_readout=False, into=None):
    """X' = P^T z in the rows of ``lvl.g`` (+ the max readout of z, written into ``into`` when given)"""
    return _EigenPool.apply(z, g, lvl, lvl.coef, False, int(ghost_mode), bool(want_readout), into, None)


def eigen_pool_final(z, g, coef, ghost_mode, want_readout=False, into=None, into_final=None):
    """max(P_j^T z, 0) of the single-column final matrices, [B, J*C] (+ the max readout of z)"""
    return _EigenPool.apply(z, g, None, coef, True, int(ghost_mode), bool(want_readout), into, into_final)
