"""Drop-in for Code/eigengcn/tripletnet.py:11-155 — the triplet pre-training step of the EigenGCN family (train_triplet.py:289-317).

The reference calls ``WavePoolingGcnEncoder`` three times at B = 1 (anchor, positive, negative), each time from 1 + L + L J + Jf dense
``[1, Nmax, Nmax]`` tensors built from the graph object's ``.graph`` dict.  Here

* a graph object's dict is packed ONCE on the host (``pack_host``: CSR of the adjacency and of every pooled adjacency, the rows'
  clusters / coefficients / bucket lists, the final coefficients — the compact pieces ``eigen_pool.collate`` builds) and goes to the
  device at the object's first use, together with its feature rows (16-byte row stride).  No ``[Nmax, Nmax]`` array is uploaded.
  ``feats`` are host numpy arrays that cross_val.py builds once and the reference never writes, so they are cached with the structure
  (as ``triplet.resident_graph`` caches them; ``Code/sag`` keeps device tensors instead, which ``sag_triplet`` reads in place).  The
  cache is the model's ``resident.ResidentCache``, keyed by the object's identity; ``TSGNN_TRIPLET_CACHE=0`` rebuilds every step;
* a step concatenates three cached graphs into one three-graph ``EigenBatch`` on the device (``eigen_pool.concat_batches``) and runs the
  model ONCE with per-graph statistics (``per_graph_bn``: the fresh ``BatchNorm1d(Nmax)`` at B = 1 is a per-row layer norm) — level 0
  as the fused stack node, pooled levels layer by layer;
* ``pred_model`` on the three readout rows and both ``F.pairwise_distance`` are one launch each way (csrc/mlp2_triplet.hip for
  Linear-ReLU-Linear, csrc/triplet.hip for a single Linear); any other head runs through torch.

``batch(a, p, n)`` / ``embed(batch)`` split the call for a step replayed from a hipGraph on a resident triplet (refill ``batch.x`` in place).

Stage two (``two_stage.embed_dataset``: the reference's ``evaluate()`` / ``evaluate_mlp()``, train_triplet.py:30-268) embeds hundreds of
graphs per call.  What is resident per graph object is therefore ONE int32 device buffer, the piece (``piece_buffer``: every level's
CSR, every pooling level's clusters / coefficients / bucket lists, the final coefficients and the feature rows, piece-local indices,
sections on 16 bytes at ``tsgnn_eigen_assemble_layout``'s offsets), uploaded in one copy.  The triplet step's one-graph ``EigenBatch``
is made of views of that buffer at its first use; ``assemble`` writes the complete ``EigenBatch`` of a chunk from the pieces
(csrc/eigen_assemble.hip), and ``embed_chunk`` runs the model once on it.  Either side finds the other's entries in the model's
``resident.ResidentCache``, so a graph is uploaded once whoever sees it first.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import eigen_pool as ep
from . import message_passing as mp
from . import resident as R
from . import triplet as _t
from .graph import GraphBatch

MarginRankingLoss = _t.MarginRankingLoss        # the documented replacement for the loop's `criterion` (train_triplet.py:292)
DEFAULT_CHUNK = 256                             # graphs per chunk of stage two: the fastest of 32 / 64 / 128 / 256 (profiles/r10/eigen_two_stage.txt)
GUARD = 0x5A5A5A5A                              # assemble(guard=...): the word tests look for behind the arrays


# ----------------------------------------------------------------------------- host half: a .graph dict -> compact pieces (pure numpy)
def _square(d, key, nmax):
    if key not in d:
        raise ValueError("the graph dict has no '%s'" % key)
    a = np.asarray(d[key])
    if a.ndim != 2 or a.shape[0] != a.shape[1] or (nmax is not None and a.shape[0] != nmax):
        raise ValueError("%s has shape %s, expected [Nmax, Nmax]%s" % (key, a.shape, "" if nmax is None else " with Nmax = %d" % nmax))
    return a


def pack_host(graph, L, J, Jf):
    """One ``.graph`` dict (cross_val.py: 'adj', 'feats', 'num_nodes', 'adj_pool_{i+1}', 'num_nodes_{i+1}', 'pool_adj_{i}_{j}') -> the
    compact form of its L pooling levels, J matrices per level and Jf final matrices:

    ``n`` [L + 1] node counts, ``nmax``, ``graphs`` [L + 1] (rowptr int32[n_i + 1], col int32, val float32, symmetric) of
    ``adj[:n, :n]`` and ``adj_pool_{i+1}[:k, :k]``, ``levels`` [L] dicts with ``cluster_of`` int32[n_i] (the first column with a
    non-zero entry in any of the J matrices — the rule of tsgnn_eigen_pool_from_dense_f32 —, -1 for a row whose J entries are all
    zero), ``coef`` float32[n_i, J], and the local bucket list ``bptr`` int32[k + 2] / ``members`` int32[n_i] (bucket 0 = the
    unassigned rows, bucket c + 1 = cluster c; rows ascending inside a bucket), ``final`` float32[n_L, Jf] (column 0 of
    ``pool_adj_{L}_{j}``) or None.

    ValueError for: a matrix that is not [Nmax, Nmax]; an entry in a column >= the pooled node count; a row with entries in two
    different columns; a non-zero in a row >= n_i."""
    nmax = _square(graph, "adj", None).shape[0]
    n0 = int(graph["num_nodes"])
    if not 1 <= n0 <= nmax:
        raise ValueError("num_nodes must lie in [1, Nmax]")
    sizes, graphs, levels = [n0], [R.dense_csr_host(_square(graph, "adj", nmax), n0)], []
    for i in range(L):
        n = sizes[-1]
        k = int(graph["num_nodes_%d" % (i + 1)])
        if not 1 <= k <= nmax:
            raise ValueError("num_nodes_%d must lie in [1, Nmax]" % (i + 1))
        P = np.stack([np.asarray(_square(graph, "pool_adj_%d_%d" % (i, j), nmax), dtype=np.float32) for j in range(J)])    # [J, N, N]
        nz = (P != 0).any(axis=0)
        if nz[n:].any():
            raise ValueError("pool_adj_%d_*: a non-zero entry in a row >= the level's node count %d" % (i, n))
        if nz[:, k:].any():
            raise ValueError("pool_adj_%d_*: an entry in a column >= the pooled node count %d" % (i, k))
        cnt = nz[:n].sum(axis=1)
        if (cnt > 1).any():
            raise ValueError("pool_adj_%d_*: row %d has entries in two different columns" % (i, int(np.nonzero(cnt > 1)[0][0])))
        clus = np.where(cnt > 0, nz[:n].argmax(axis=1), -1).astype(np.int32)
        coef = np.where(clus[None, :] >= 0, P[:, np.arange(n), np.maximum(clus, 0)], 0.0).T.astype(np.float32)
        key = clus.astype(np.int64) + 1
        members = np.argsort(key, kind="stable").astype(np.int32)
        bptr = np.zeros(k + 2, dtype=np.int32)
        np.cumsum(np.bincount(key, minlength=k + 1), out=bptr[1:])
        levels.append({"cluster_of": clus, "coef": np.ascontiguousarray(coef), "bptr": bptr, "members": members})
        graphs.append(R.dense_csr_host(_square(graph, "adj_pool_%d" % (i + 1), nmax), k))
        sizes.append(k)
    final = None
    if Jf:
        nL = sizes[-1]
        P = np.stack([np.asarray(_square(graph, "pool_adj_%d_%d" % (L, j), nmax), dtype=np.float32) for j in range(Jf)])
        nz = (P != 0).any(axis=0)
        if nz[nL:].any():
            raise ValueError("pool_adj_%d_*: a non-zero entry in a row >= the level's node count %d" % (L, nL))
        if nz[:, 1:].any():
            raise ValueError("pool_adj_%d_*: an entry in a column >= the pooled node count 1" % L)
        final = np.ascontiguousarray(P[:, :nL, 0].T)
    return {"n": sizes, "nmax": nmax, "graphs": graphs, "levels": levels, "final": final}


# ----------------------------------------------------------------------------- the graphs of the dataset, resident
def graph_dict(obj):
    """the ``.graph`` dict of a graph object, or the dict itself (``GraphSampler.__getitem__`` hands out bare dicts)"""
    return obj if isinstance(obj, dict) else obj.graph


def check_dict(d, L, J, Jf):
    """ValueError for a dict that was prepared for another number of levels or pooling matrices than the model's (the sampler writes
    exactly ``num_pool_matrix`` matrices per level and ``num_pool_final_matrix`` final ones): a key the model needs is missing, or a
    level / matrix beyond the model's is present"""
    need = ["adj", "feats", "num_nodes"] + [k % (i + 1) for i in range(L) for k in ("adj_pool_%d", "num_nodes_%d")] + \
        ["pool_adj_%d_%d" % (i, j) for i in range(L) for j in range(J)] + ["pool_adj_%d_%d" % (L, j) for j in range(Jf)]
    over = ["adj_pool_%d" % (L + 1), "num_nodes_%d" % (L + 1), "pool_adj_%d_%d" % (L, Jf)] + ["pool_adj_%d_%d" % (i, J) for i in range(L)]
    for k in need:
        if k not in d:
            raise ValueError("the graph dict has no '%s': the model has %d pooling levels, %d pooling and %d final matrices" % (k, L, J, Jf))
    for k in over:
        if k in d:
            raise ValueError("the graph dict has '%s': the model has %d pooling levels, %d pooling and %d final matrices" % (k, L, J, Jf))


def padded_rows_host(f, n):
    """``resident.padded_rows`` on the host: the first n rows, zero-padded to a row stride that is a multiple of 4 floats"""
    f = np.asarray(f, dtype=np.float32)
    if f.ndim != 2 or f.shape[0] < n:
        raise ValueError("feats must be [Nmax, F]")
    out = np.zeros((n, max(4, (f.shape[1] + 3) // 4 * 4)), dtype=np.float32)
    out[:, :f.shape[1]] = f[:n]
    return out


def piece_layout(n, nnz, J, Jf, ldf):
    """word offsets of a piece buffer's sections (``tsgnn_eigen_assemble_layout``; the last entry is the buffer's length): per level
    graph rowptr | col | val, per pooling level cluster_of | coef | bptr | members, then final | feature rows"""
    nlev = len(n)
    off = np.zeros(7 * nlev - 1, dtype=np.int64)
    nn, zz = np.asarray(n, dtype=np.int64), np.asarray(nnz, dtype=np.int64)
    nat.call_nostream("eigen_assemble_layout", nlev, max(int(J), 1), int(Jf), int(ldf), nn.ctypes.data, zz.ctypes.data, off.ctypes.data)
    return off


def piece_buffer(packed, feats, J):
    """pack_host's result + the feature rows (``padded_rows_host``) as the ONE int32 buffer the assembler reads -> (buffer, offsets)"""
    n, L = packed["n"], len(packed["levels"])
    nnz = [int(c[1].size) for c in packed["graphs"]]
    Jf = 0 if packed["final"] is None else int(packed["final"].shape[1])
    off = piece_layout(n, nnz, J, Jf, feats.shape[1])
    buf = np.zeros(int(off[-1]), dtype=np.int32)
    parts = []
    for rp, col, val, _ in packed["graphs"]:
        parts += [rp, col, val.view(np.int32)]
    for lv in packed["levels"]:
        parts += [lv["cluster_of"], lv["coef"].reshape(-1).view(np.int32), lv["bptr"], lv["members"]]
    parts += [(packed["final"].reshape(-1).view(np.int32) if Jf else np.zeros(0, np.int32)), feats.reshape(-1).view(np.int32)]
    for o, part in zip(off[:-1], parts):
        buf[int(o):int(o) + part.size] = part
    return buf, off


def unpack_piece(buf, n, nnz, J, Jf, ldf):
    """the sections of a piece buffer back as arrays (host or device, views): ``graphs`` [(rowptr, col, val)], ``levels`` [dicts as
    pack_host's], ``final`` [n_L, Jf] or None, ``feats`` [n_0, ldf]"""
    off = piece_layout(n, nnz, J, Jf, ldf)
    f32 = (lambda a: a.view(np.float32)) if isinstance(buf, np.ndarray) else (lambda a: a.view(torch.float32))
    sec = lambda s, count: buf[int(off[s]):int(off[s]) + int(count)]
    nlev, L = len(n), len(n) - 1
    graphs = [(sec(3 * i, n[i] + 1), sec(3 * i + 1, nnz[i]), f32(sec(3 * i + 2, nnz[i]))) for i in range(nlev)]
    levels = []
    for i in range(L):
        s = 3 * nlev + 4 * i
        levels.append({"cluster_of": sec(s, n[i]), "coef": f32(sec(s + 1, n[i] * J)).reshape(n[i], J), "bptr": sec(s + 2, n[i + 1] + 2),
                       "members": sec(s + 3, n[i])})
    s = 3 * nlev + 4 * L
    final = f32(sec(s, n[L] * Jf)).reshape(n[L], Jf) if Jf else None
    return {"graphs": graphs, "levels": levels, "final": final, "feats": f32(sec(s + 1, n[0] * ldf)).reshape(n[0], ldf)}


class _Graph:
    """device side of one graph object: the piece buffer ``buf``, the host numbers the assembler's description needs, and — built from
    views of the buffer when the triplet step first asks — the one-graph EigenBatch ``eb`` and the feature rows ``feats`` [n, ld]"""
    __slots__ = ("ref", "buf", "ptr", "sizes", "nnz", "sym", "n", "nmax", "ldf", "fin", "L", "J", "Jf", "_eb", "_feats")

    @property
    def eb(self):
        if self._eb is None:
            self._eb, self._feats = _views(self)
        return self._eb

    @property
    def feats(self):
        if self._feats is None:
            self._eb, self._feats = _views(self)
        return self._feats


def _views(e):
    """the one-graph EigenBatch and feature rows of a resident piece, on the device: views of its buffer (only ``rowptr`` is a new
    tensor: the piece's n + 1 entries and the Nmax closing entries of the empty ghost-slot rows).  No graph data is uploaded, which
    is what ``cache.h2d`` counts; like ``tripletnet.batch``, every ``GraphBatch.from_csr`` here still uploads its ``graph_ptr`` and
    ``slot_count`` (a few dozen bytes from host-known sizes) and launches ``row_maps``, once per object"""
    dev, nmax = e.buf.device, e.nmax
    u = unpack_piece(e.buf, e.sizes, e.nnz, e.J, e.Jf, e.ldf)
    gs = []
    for (rp, col, val), n, z, sym in zip(u["graphs"], e.sizes, e.nnz, e.sym):
        rowptr = torch.cat([rp, rp[n:n + 1].expand(nmax)])
        if not z:
            col, val = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
        g = GraphBatch.from_csr(rowptr, col, val, np.array([n], dtype=np.int64), nmax, assume_symmetric=sym)
        g.nnz = int(z)
        gs.append(g)
    levels = []
    for i, h in enumerate(u["levels"]):
        lv = ep.EigenLevel()
        lv.g, lv.J = gs[i + 1], e.J
        lv.cluster_of, lv.coef, lv.bptr, lv.members = h["cluster_of"], h["coef"], h["bptr"], h["members"]
        levels.append(lv)
    return ep.EigenBatch(gs[0], levels, u["final"], nmax), u["feats"]


def device_piece(packed, feats, J, dev):
    """pack_host's result + the graph's ``feats`` -> the resident entry: ONE host-to-device copy"""
    rows = padded_rows_host(feats, packed["n"][0])
    buf, _ = piece_buffer(packed, rows, J)
    e = _Graph()
    e.buf = torch.from_numpy(buf).to(dev)
    e.ptr = int(e.buf.data_ptr())
    e.sizes, e.nnz = [int(v) for v in packed["n"]], [int(c[1].size) for c in packed["graphs"]]
    e.sym = [bool(c[3]) for c in packed["graphs"]]
    e.n, e.nmax, e.ldf, e.fin = e.sizes[0], int(packed["nmax"]), int(rows.shape[1]), int(np.asarray(feats).shape[1])
    e.L, e.J, e.Jf = len(packed["levels"]), int(J), 0 if packed["final"] is None else int(packed["final"].shape[1])
    e._eb = e._feats = None
    return e


def resident_graph(obj, dev, cache, L, J, Jf, check=False):
    """the resident piece of one graph object (packed and uploaded — one copy — at its first use), keyed by the object; a bare dict is
    packed at every call (the sampler makes a new one per access: there is nothing to key on).  ``check``: ``check_dict`` before
    packing"""
    keyed = R.RESIDENT and not isinstance(obj, dict)
    e = cache.lookup(obj, dev.index) if keyed else None
    if e is not None:
        return e
    d = graph_dict(obj)
    if check:
        check_dict(d, L, J, Jf)
    e = device_piece(pack_host(d, L, J, Jf), d["feats"], J, dev)
    cache.h2d += 1
    return cache.store(obj, e, dev.index) if keyed else e


class _Triplet:
    """three graphs as one batch on the device: the ``EigenBatch`` ``eb`` and the feature rows ``x`` [rows + Nmax, ld] (refill it in
    place between hipGraph replays; the Nmax ghost-slot rows stay zero)"""
    __slots__ = ("eb", "x", "sizes")


def to_device(packed, feats, dev):
    """pack_host's result + the feature rows -> (one-graph EigenBatch, feats [n, ld] with a 16-byte row stride, host-to-device copies):
    the piece buffer in ONE copy, both results views of it"""
    J = int(packed["levels"][0]["coef"].shape[1]) if packed["levels"] else 1
    e = device_piece(packed, feats, J, dev)
    return e.eb, e.feats, 1


# ----------------------------------------------------------------------------- resident pieces -> the EigenBatch of a chunk
def _a4(v):
    return (int(v) + 3) // 4 * 4


def chunk_shape(parts):
    """(Nmax, ldf, L, J, Jf) shared by the pieces of a chunk; ValueError when they differ"""
    f = parts[0]
    if any(p.nmax != f.nmax for p in parts):
        raise ValueError("the graphs of a chunk must be padded to the same Nmax")
    if any(p.ldf != f.ldf or p.fin != f.fin for p in parts):
        raise ValueError("the graphs of a chunk must have the same number of features")
    if any((p.L, p.J, p.Jf) != (f.L, f.J, f.Jf) for p in parts):
        raise ValueError("the graphs of a chunk must share the number of levels and of pooling matrices")
    return f.nmax, f.ldf, f.L, f.J, f.Jf


def max_levels():
    """pooling levels the assembler takes (``tsgnn_eigen_assemble_max_levels``)"""
    return int(nat.lib().tsgnn_eigen_assemble_max_levels())


def assemble(parts, dev, guard=0):
    """resident pieces (a chunk of a dataset) -> (feature rows [R_0 + Nmax, ldf] with the ghost rows zero, EigenBatch): every array of
    ``eigen_pool.concat_batches`` of the same one-graph batches, word for word, with the row bookkeeping ``GraphBatch.from_csr`` would
    launch and upload (``graph_ptr``, ``row_graph``, ``row_slot``, ``slot_count``) written by the same kernel.  Two allocations (the
    integer and the float arrays, every array on 16 bytes), all sizes host numbers: ceil(len(parts) / 32) launches with the pieces'
    records in the kernel arguments, no upload, no host synchronisation.  ``guard`` (tests): that many words of ``GUARD`` behind every array; ``eb._raw`` = (both buffers, the arrays' offsets and
    lengths in them)."""
    lib = nat.lib()
    kmax, hw, pw = (int(f()) for f in (lib.tsgnn_eigen_assemble_max_pieces, lib.tsgnn_eigen_assemble_header_words,
                                       lib.tsgnn_eigen_assemble_piece_words))
    nmax, ldf, L, J, Jf = chunk_shape(parts)
    if L > max_levels():
        raise ValueError("the assembler takes up to %d pooling levels" % max_levels())
    B, nlev = len(parts), L + 1
    n = np.array([p.sizes for p in parts], dtype=np.int64).reshape(B, nlev)
    z = np.array([p.nnz for p in parts], dtype=np.int64).reshape(B, nlev)
    row0, e0 = np.zeros((B + 1, nlev), dtype=np.int64), np.zeros((B + 1, nlev), dtype=np.int64)
    np.cumsum(n, axis=0, out=row0[1:])
    np.cumsum(z, axis=0, out=e0[1:])
    Rr, E = [int(v) for v in row0[-1]], [int(v) for v in e0[-1]]
    isz, fsz = [], []
    for i in range(nlev):                                    # rowptr, col, graph_ptr, row_graph, row_slot, slot_count | val
        isz += [Rr[i] + nmax + 1, max(E[i], 1), B + 1, Rr[i], Rr[i], nmax]
        fsz.append(max(E[i], 1))
    for i in range(L):                                       # cluster_of, bptr, members | coef
        isz += [Rr[i], Rr[i + 1] + B + 1, Rr[i]]
        fsz.append(Rr[i] * J)
    fsz += [Rr[L] * Jf, (Rr[0] + nmax) * ldf]
    ioff = np.concatenate([[0], np.cumsum([_a4(s + guard) for s in isz])])
    foff = np.concatenate([[0], np.cumsum([_a4(s + guard) for s in fsz])])
    ibuf = torch.empty(int(ioff[-1]), dtype=torch.int32, device=dev)
    fbuf = torch.empty(int(foff[-1]), dtype=torch.float32, device=dev)
    if guard:
        ibuf.fill_(GUARD)
        fbuf.view(torch.int32).fill_(GUARD)
    iv = [ibuf[int(o):int(o) + s] for o, s in zip(ioff, isz)]
    fv = [fbuf[int(o):int(o) + s] for o, s in zip(foff, fsz)]
    head = np.zeros(hw, dtype=np.int64)
    head[1:8] = (B, nlev, J, Jf, ldf, nmax, 1)
    head[9], head[10] = fv[-1].data_ptr(), fv[-2].data_ptr() if Jf else 0
    for i in range(nlev):
        head[12 + 2 * i], head[13 + 2 * i] = Rr[i], E[i]
        g = iv[6 * i:6 * i + 6]
        head[20 + 7 * i:27 + 7 * i] = [g[0].data_ptr(), g[1].data_ptr(), fv[i].data_ptr()] + [t.data_ptr() for t in g[2:]]
        if E[i] == 0:                                        # (one unread word each; kept defined, as concat_csr's zeros(1))
            g[1].zero_()
            fv[i].zero_()
    for i in range(L):
        lv = iv[6 * nlev + 3 * i:6 * nlev + 3 * i + 3]
        head[48 + 4 * i:52 + 4 * i] = (lv[0].data_ptr(), fv[nlev + i].data_ptr(), lv[1].data_ptr(), lv[2].data_ptr())
    rec = np.zeros((B, pw), dtype=np.int64)
    rec[:, 0] = [p.ptr for p in parts]
    rec[:, 1] = np.arange(B)
    rec[B - 1, 2] = 1
    for i in range(nlev):
        rec[:, 3 + 4 * i], rec[:, 4 + 4 * i], rec[:, 5 + 4 * i], rec[:, 6 + 4 * i] = n[:, i], z[:, i], row0[:B, i], e0[:B, i]
    for s in range(0, B, kmax):
        d = np.concatenate([head, rec[s:s + kmax].reshape(-1)])
        d[0], d[7] = min(kmax, B - s), int(s == 0)             # (the first launch starts the slot counts, the others continue them)
        nat.call("eigen_assemble_f32", d.ctypes.data)
    gs = []
    for i in range(nlev):
        g = GraphBatch()
        g.layout, g.B, g.nmax, g.device = "packed", B, nmax, dev
        g.sizes, g.n_rows, g.n_ghost = n[:, i].copy(), Rr[i], nmax
        g.rowptr, g.col, g.graph_ptr, g.row_graph, g.row_slot, g.slot_count = iv[6 * i:6 * i + 6]
        g.val, g.nnz, g.symmetric = fv[i], E[i], all(p.sym[i] for p in parts)
        gs.append(g)
    levels = []
    for i in range(L):
        lv = ep.EigenLevel()
        lv.g, lv.J = gs[i + 1], J
        lv.cluster_of, lv.bptr, lv.members = iv[6 * nlev + 3 * i:6 * nlev + 3 * i + 3]
        lv.coef = fv[nlev + i].view(Rr[i], J)
        levels.append(lv)
    eb = ep.EigenBatch(gs[0], levels, fv[-2].view(Rr[L], Jf) if Jf else None, nmax)
    eb._raw = (ibuf, fbuf, ioff, isz, foff, fsz)
    eb._pieces = parts                                     # (a recorded launch replays by address: the buffers outlive the batch's use)
    return fv[-1].view(Rr[0] + nmax, ldf), eb


# ----------------------------------------------------------------------------- stage two: the embeddings of a chunk of graphs
def model_shape(model):
    """(L, J, Jf) of a ``WavePoolingGcnEncoder``"""
    return len(model.pool_sizes), int(model.num_pool_matrix), int(model.num_pool_final_matrix)


def embed_one(model, obj, dev):
    """the embedding [1, E] of one graph object or bare ``.graph`` dict by a call of its own: a one-graph ``EigenBatch`` from
    ``pack_host`` / ``to_device`` through the model call of ``embed_chunk`` (``TSGNN_TRIPLET_CACHE=0``, a chunk the assembler does not
    take).  Nothing is cached.  The caller holds eval mode / no_grad."""
    if dev.type != "cuda":
        raise RuntimeError(R.GPU_ONLY)
    L, J, Jf = model_shape(model)
    d = graph_dict(obj)
    check_dict(d, L, J, Jf)
    eb, feats, _ = to_device(pack_host(d, L, J, Jf), d["feats"], dev)
    x = torch.cat([feats, R.ghost_zeros(eb.nmax, feats.size(1), dev)])
    with R.per_graph_statistics(model):
        return model.pred_model(model(x, eb, readout_only=True))


def embed_chunk(model, graphs, dev, cache):
    """embeddings [len(graphs), E] of a chunk of graph objects (or bare ``.graph`` dicts): the chunk's ``EigenBatch`` assembled from
    the resident pieces, the model ONCE under per-graph statistics, ``pred_model`` on all rows — row i is ``feat[0]`` of the
    reference's eval-mode B = 1 call for graph i (train_triplet.py:77-78).  The caller holds eval mode / no_grad
    (``two_stage.embed_dataset``).  ValueError for mixed Nmax, mixed feature widths, a dict prepared for another L / J / Jf than the
    model's."""
    L, J, Jf = model_shape(model)
    if L > max_levels():
        return torch.cat([embed_one(model, o, dev) for o in graphs])
    parts = [resident_graph(o, dev, cache, L, J, Jf, check=True) for o in graphs]
    x, eb = assemble(parts, dev)
    with R.per_graph_statistics(model):
        return model.pred_model(model(x, eb, readout_only=True))


# ----------------------------------------------------------------------------- pred_model + both distances: one launch each way
class _Mlp2TripletTail(torch.autograd.Function):
    """(readouts r[3, D], Linear-ReLU-Linear weights and biases) -> (dist_p[1], dist_n[1], embed_a[1, E], embed_p, embed_n).  The five
    outputs are separate tensors, so no slice (and no zero-filled slice gradient) is launched around them."""

    @staticmethod
    def forward(ctx, r, w1, b1, w2, b2):
        params = (w1, b1, w2, b2)                         # (the Parameter objects: their slices of a trainer's flat gradient bucket)
        r, w1, w2 = r.contiguous(), w1.contiguous(), w2.contiguous()
        D, H, E = int(w1.size(1)), int(w1.size(0)), int(w2.size(0))
        dev = r.device
        h, embed, dist = mp._f32(3, H, device=dev), mp._f32(3, E, device=dev), mp._f32(2, device=dev)
        nat.call("mlp2_triplet_fwd_f32", r, r.stride(0), w1, b1, w2, b2, D, H, E, R.EPS, h, embed, dist)
        ctx.save_for_backward(r, w1, w2, h, embed, dist)
        ctx.params = params
        ctx.set_materialize_grads(False)                  # an unused output's gradient arrives as None, not as a zero-filled tensor
        return dist[0:1], dist[1:2], embed[0:1], embed[1:2], embed[2:3]

    @staticmethod
    def backward(ctx, g_dp, g_dn, g_a, g_p, g_n):
        r, w1, w2, h, embed, dist = ctx.saved_tensors
        D, H, E = int(w1.size(1)), int(w1.size(0)), int(w2.size(0))
        dev = r.device
        c = lambda t: t.contiguous() if t is not None else None
        # straight into the trainer's flat gradient bucket when one is installed (FlatTrainer): no AccumulateGrad copy, no zeroing
        (dw1, db1, dw2, db2), grads = mp._sinks_or_new(ctx.params, ((H, D), (H,), (E, H), (E,)), dev)
        dr = mp._f32(3, D, device=dev) if ctx.needs_input_grad[0] else None
        nat.call("mlp2_triplet_bwd_f32", r, r.stride(0), w1, w2, h, embed, dist, R.EPS, c(g_dp), c(g_dn), c(g_a), c(g_p), c(g_n), D, H, E,
                 dr, D, dw1, db1, dw2, db2)
        return (dr,) + grads


def _linears(pred):
    """the nn.Linear layers of a pred_model built by build_pred_layers (Linear, or Linear (ReLU Linear)*), or None"""
    if isinstance(pred, nn.Linear):
        return [pred]
    if isinstance(pred, nn.Sequential) and len(pred) % 2 == 1 and all(
            isinstance(m, nn.Linear if i % 2 == 0 else nn.ReLU) for i, m in enumerate(pred)):
        return [m for m in pred if isinstance(m, nn.Linear)]
    return None


def _lin_ok(lin):
    w = lin.weight
    return w.dtype == torch.float32 and w.is_cuda and w.is_contiguous() and w.data_ptr() % 16 == 0 and \
        (lin.bias is None or lin.bias.dtype == torch.float32)


def tail_kind(model, r):
    """'mlp2' (csrc/mlp2_triplet.hip), 'linear' (csrc/triplet.hip) or None (torch) for this pred_model on these readout rows
    (``TSGNN_TRIPLET_TAIL=0``: never a fused tail)"""
    lins = _linears(getattr(model, "pred_model", None))
    if not (_t.FUSED_TAIL and lins and r is not None and r.is_cuda and r.dim() == 2 and r.size(0) == 3 and r.dtype == torch.float32
            and r.size(1) == lins[0].in_features and r.is_contiguous() and r.data_ptr() % 16 == 0 and all(_lin_ok(l) for l in lins)):
        return None
    if len(lins) == 2 and nat.lib().tsgnn_mlp2_triplet_supported(int(lins[0].in_features), int(lins[0].out_features),
                                                                  int(lins[1].out_features)):
        return "mlp2"
    if len(lins) == 1 and lins[0].in_features % 4 == 0 and lins[0].out_features <= 512:      # (triplet.tail_ok's limits)
        return "linear"
    return None


class tripletnet(nn.Module):
    """``tripletnet(model, args).forward(a, p, n) -> (dist_p, dist_n, embed_a, embed_p, embed_n)`` for ``model`` =
    ``eigen_encoders.WavePoolingGcnEncoder``; ``args`` supplies ``pool_sizes`` ('10', '3_2'), ``num_pool_matrix`` and
    ``num_pool_final_matrix``, which must agree with the model's."""

    def __init__(self, model, args):
        super().__init__()
        self.model = model
        self.args = args
        pool_sizes = [int(i) for i in str(args.pool_sizes).split("_")]
        if pool_sizes != [int(s) for s in model.pool_sizes]:
            raise ValueError("args.pool_sizes = %r, the model was built with %r" % (args.pool_sizes, list(model.pool_sizes)))
        if int(args.num_pool_matrix) != int(model.num_pool_matrix):
            raise ValueError("args.num_pool_matrix = %d, the model's is %d" % (args.num_pool_matrix, model.num_pool_matrix))
        if int(args.num_pool_final_matrix) != int(model.num_pool_final_matrix):
            raise ValueError("args.num_pool_final_matrix = %d, the model's is %d"
                             % (args.num_pool_final_matrix, model.num_pool_final_matrix))
        self.L, self.J, self.Jf = len(pool_sizes), int(args.num_pool_matrix), int(args.num_pool_final_matrix)
        self.cache = R.cache_for(model)                      # (the entries depend on (L, J, Jf) only, which equal the model's)

    # ------------------------------------------------------------------ graphs
    def _graph(self, obj, dev):
        """the device side of one graph object (built at its first use)"""
        return resident_graph(obj, dev, self.cache, self.L, self.J, self.Jf)

    def batch(self, a, p, n):
        """the triplet as one three-graph batch on the device: the cached pieces concatenated there (no host synchronisation, no
        upload of the graphs' structure or features once the three objects have been seen).  What a step still sends is the row
        bookkeeping of the new batch: every one of its L + 1 ``GraphBatch``es uploads ``graph_ptr`` and ``slot_count`` (a few dozen
        bytes from host-known sizes, ``GraphBatch._set_sizes``) and launches ``row_maps``; ``cache.h2d`` does not count these, and they
        lie outside a step captured on ``embed(batch)``."""
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(R.GPU_ONLY)
        parts = [self._graph(o, dev) for o in (a, p, n)]
        if any(q.nmax != parts[0].nmax for q in parts):
            raise ValueError("the graphs of a triplet must be padded to the same Nmax")
        if any(q.feats.size(1) != parts[0].feats.size(1) for q in parts):
            raise ValueError("the graphs of a triplet must have the same number of features")
        b = _Triplet()
        b.eb = ep.concat_batches([q.eb for q in parts])
        b.x = torch.cat([q.feats for q in parts] + [R.ghost_zeros(parts[0].nmax, parts[0].feats.size(1), dev)])
        b.sizes = b.eb.g0.sizes
        return b

    # ------------------------------------------------------------------ forward
    def _tail(self, r):
        """readout rows [3, D] -> (dist_p, dist_n, embed_a, embed_p, embed_n): one launch, or the torch composition for a head the
        kernels do not take"""
        pm = self.model.pred_model
        kind = tail_kind(self.model, r)
        if kind == "mlp2":
            return _Mlp2TripletTail.apply(r, pm[0].weight, pm[0].bias, pm[2].weight, pm[2].bias)
        if kind == "linear":
            return _t._TripletTail.apply(r, pm.weight, pm.bias)
        return R.torch_distances(pm(r))

    def embed(self, b):
        """the step on a batch from ``batch()``: the model once with the per-graph statistics of a B = 1 call, then the tail"""
        with R.per_graph_statistics(self.model):
            r = self.model(b.x, b.eb, readout_only=True)
        return self._tail(r)

    def forward(self, a, p, n):
        """a, p, n: objects with ``.graph`` = {'adj', 'feats', 'num_nodes', 'adj_pool_i', 'num_nodes_i', 'pool_adj_i_j'} as
        cross_val.py prepares them ('assign_feats' is not needed: the reference reads it and never uses it)"""
        return self.embed(self.batch(a, p, n))
