"""Drop-in for Code/sage+gat+diffpool/tripletnet.py:11-45 around a ``gat_encoders.DGATEncoderGraph`` — the triplet pre-training step of
the GAT encoder (train_triplet.py --method=GAT), and the chunks of stage two (``two_stage.embed_dataset``).

The reference calls the encoder three times at B = 1 (anchor, positive, negative), each time from a dense ``[1, Nmax, Nmax]`` adjacency.
Here

* a graph object is packed ONCE on the host (``pack_host``: the one-graph piece of ``GraphBatch.from_dense_ghost1``'s layout — CSR of
  ``adj[:n, :n] > 0`` and its transpose with the entry maps, ONE representative of the Nmax - n padded rows, the edge-less columns, the
  feature rows) and goes to the device as one buffer at the object's first use, into the model's ``resident.ResidentCache``;
* a step concatenates cached pieces into the packed block-diagonal batch with ONE launch per 8 graphs (csrc/gat_assemble.hip): every
  array ``gat_fused`` / ``attention`` look for on a ``GraphBatch`` is written by it, all sizes are host numbers, so nothing is uploaded
  and nothing waits for the device;
* the encoder runs ONCE on the batch, every graph on its own rows (at B = 1 the reference's ``input[0]`` IS the graph's own rows, so
  the result is the three B = 1 forwards whatever ``per_graph_features`` says), and the Linear head with both ``F.pairwise_distance``
  is one launch each way (csrc/triplet.hip) when the head is a single ``nn.Linear``.

Fallback — three B = 1 calls of the module on dense tensors, the reference literally, correct and not fast: attention or input dropout
active in training mode (a representative is exact only while its copies stay identical), a graph whose padded feature rows differ or
whose ``adj`` has a positive entry outside ``[:n, :n]``, ``resident.RESIDENT`` off, a model on the CPU.
"""
import contextlib

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import message_passing as mp
from . import resident as R
from . import triplet as _t
from .gat_encoders import DGATEncoderGraph, DGATHead
from .graph import GraphBatch

MarginRankingLoss = _t.MarginRankingLoss        # the documented replacement for the loop's `criterion` (train_triplet.py:235)
DEFAULT_CHUNK = 256                             # graphs per chunk of stage two: the fastest of 32 / 64 / 128 / 256 (profiles/r09/gat_two_stage.txt)
GUARD = 0x5A5A5A5A                              # assemble(guard=...): the word tests look for behind the arrays
HEAD_ROWS_MAX = 1024                            # DGATEncoderGraph.forward's fused head: x.size(0) <= 1024


# ----------------------------------------------------------------------------- host half: a graph object -> its piece (pure numpy)
def representable(adj, feats, n):
    """one representative row can stand for the padded rows of this graph: the rows ``feats[n:]`` are all identical and ``adj`` has no
    positive entry outside ``[:n, :n]`` (an edge of a padded row; the dense B = 1 reference would use it)"""
    inside = int(np.count_nonzero(adj[:n, :n] > 0))
    return bool((n >= feats.shape[0] - 1 or (feats[n + 1:] == feats[n]).all()) and int(np.count_nonzero(adj > 0)) == inside)


def pack_host(obj):
    """One graph object (``.graph`` = {'adj', 'feats', 'num_nodes', ...}) -> the one-graph piece of the ghost-1 layout, a dict:

    ``n``, ``nmax``, ``nr`` = n + 1 when n < Nmax (the closing row is the representative of the Nmax - n padded rows, ``mult`` =
    Nmax - n on it) else n; ``rowptr`` int32[nr + 1] / ``col`` int32[nnz] of ``adj[:n, :n] > 0`` (a mask: no weights), columns ascending;
    ``rowptr_t`` / ``col_t`` of the transpose, entries of a transposed row ascending by source row, ``src_e_t[p]`` = the entry of A
    that transposed entry p is and ``inv_e_t`` its inverse; ``iso_rows`` int32[k] / ``iso_w`` float32[k]: the columns without an edge
    and what each stands for (1, or ``mult`` for the representative); ``feats`` float32[nr, ldf]: rows ``feats[:n]`` and row n,
    zero-padded to a 16-byte row stride, ``fin`` their width; ``exact``: ``representable`` — the rows ``feats[n:]`` are all identical and
    ``adj`` has no positive entry outside ``[:n, :n]`` (else one representative cannot stand for the padded rows: the fallback).

    ValueError for a non-square ``adj`` or ``num_nodes`` outside [0, Nmax]."""
    d = obj.graph
    a = np.asarray(d["adj"])
    n = int(d["num_nodes"])
    if a.ndim != 2 or a.shape[0] != a.shape[1] or not 0 <= n <= a.shape[0]:
        raise ValueError("adj must be [Nmax, Nmax] with num_nodes <= Nmax")
    nmax = int(a.shape[0])
    f = np.asarray(d["feats"], dtype=np.float32)
    if f.ndim != 2 or f.shape[0] != nmax:
        raise ValueError("feats must be [Nmax, F]")
    ghost = n < nmax
    nr = n + int(ghost)
    r, c = np.nonzero(a[:n, :n] > 0)                                # (row-major: columns ascend inside a row)
    nnz = int(r.size)
    rowptr = np.zeros(nr + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=nr), out=rowptr[1:])
    order = np.lexsort((r, c))                                      # by column, then by source row
    rowptr_t = np.zeros(nr + 1, dtype=np.int32)
    np.cumsum(np.bincount(c, minlength=nr), out=rowptr_t[1:])
    inv = np.empty(nnz, dtype=np.int32)
    inv[order] = np.arange(nnz, dtype=np.int32)
    mult = np.ones(nr, dtype=np.float32)
    if ghost:
        mult[n] = nmax - n
    iso_rows = np.nonzero(np.diff(rowptr_t) == 0)[0].astype(np.int32)
    fin = int(f.shape[1])
    feats = np.zeros((nr, max(4, (fin + 3) // 4 * 4)), dtype=np.float32)
    feats[:, :fin] = f[:nr]
    return {"n": n, "nmax": nmax, "nr": nr, "nnz": nnz, "mult": nmax - n, "rowptr": rowptr, "col": c.astype(np.int32),
            "rowptr_t": rowptr_t, "col_t": r[order].astype(np.int32), "src_e_t": order.astype(np.int32), "inv_e_t": inv,
            "iso_rows": iso_rows, "iso_w": mult[iso_rows], "k": int(iso_rows.size), "feats": feats, "fin": fin,
            "exact": representable(a, f, n)}


def piece_buffer(p):
    """pack_host's piece as the ONE int32 buffer the assembler reads (sections at tsgnn_gat_assemble_layout's offsets)"""
    off = np.zeros(10, dtype=np.int64)
    nat.call_nostream("gat_assemble_layout", p["nr"], p["nnz"], p["k"], p["feats"].shape[1], off.ctypes.data)
    buf = np.zeros(int(off[9]), dtype=np.int32)
    parts = (p["rowptr"], p["rowptr_t"], p["col"], p["col_t"], p["src_e_t"], p["inv_e_t"], p["iso_rows"], p["iso_w"].view(np.int32),
             p["feats"].reshape(-1).view(np.int32))
    for o, part in zip(off[:9], parts):
        buf[int(o):int(o) + part.size] = part
    return buf


# ----------------------------------------------------------------------------- the graphs of the dataset, resident
class _Piece:
    """device side of one graph object: the piece buffer and the host numbers the assembler's description needs"""
    __slots__ = ("ref", "buf", "n", "nr", "nnz", "k", "mult", "nmax", "ldf", "fin", "exact")


def resident_piece(obj, dev, cache):
    """the resident piece of one graph object (built and uploaded — one copy — at its first use), keyed by the object"""
    e = cache.lookup(obj, dev.index) if R.RESIDENT else None
    if e is not None:
        return e
    p = pack_host(obj)
    e = _Piece()
    e.n, e.nr, e.nnz, e.k, e.mult, e.nmax, e.fin, e.exact = p["n"], p["nr"], p["nnz"], p["k"], p["mult"], p["nmax"], p["fin"], p["exact"]
    e.ldf = int(p["feats"].shape[1])
    e.buf = None
    if e.exact:
        e.buf = torch.from_numpy(piece_buffer(p)).to(dev)
        cache.h2d += 1
    return cache.store(obj, e, dev.index) if R.RESIDENT else e


_slot_zeros = {}


def _no_slot_counts(nmax, dev):
    """``GraphBatch.slot_count`` of a batch without ghost-slot rows: never read (n_ghost = 0), one tensor per (Nmax, device)"""
    z = _slot_zeros.get((nmax, dev.index))
    if z is None:
        z = _slot_zeros[(nmax, dev.index)] = torch.zeros(max(nmax, 1), dtype=torch.int32, device=dev)
    return z


def _a4(v):
    return (int(v) + 3) // 4 * 4


def assemble(parts, dev, heads=(), guard=0):
    """resident pieces (the three of a triplet, or a chunk of a dataset) -> (feature rows [R, ldf], GraphBatch): the packed
    block-diagonal batch with one ghost representative per graph, with everything ``gat_fused`` / ``attention`` cache on a batch
    (the transpose and its entry maps, the edge-less columns as indicator [R, H] for up to four H of ``heads`` and as list) already on it.
    ceil(len(parts) / 8) launches, no upload, no host synchronisation.  ``guard`` (tests): that many words of ``GUARD`` behind every
    array; ``g._raw`` = (both buffers, the arrays' offsets and lengths in them)."""
    lib = nat.lib()
    kmax, hw, pw = int(lib.tsgnn_gat_assemble_max_pieces()), int(lib.tsgnn_gat_assemble_header_words()), int(lib.tsgnn_gat_assemble_piece_words())
    nmax, ldf, B = parts[0].nmax, parts[0].ldf, len(parts)
    if any(p.nmax != nmax for p in parts):
        raise ValueError("the graphs of a batch must be padded to the same Nmax")
    if any(p.ldf != ldf or p.fin != parts[0].fin for p in parts):
        raise ValueError("the graphs of a batch must have the same number of features")
    heads = sorted(set(int(h) for h in heads))[:4]          # (a fifth head count: ``attention._isolated_columns`` builds its indicator at first use)
    nr = np.array([p.nr for p in parts], dtype=np.int64)
    nnz = np.array([p.nnz for p in parts], dtype=np.int64)
    ks = np.array([p.k for p in parts], dtype=np.int64)
    row0, e0, i0 = (np.concatenate([[0], np.cumsum(v)]) for v in (nr, nnz, ks))
    Rr, E, I = int(row0[-1]), int(e0[-1]), int(i0[-1])
    # two allocations: the integer arrays and the float arrays, every array on 16 bytes
    isz = [Rr + 1, Rr + 1, max(E, 1), max(E, 1), max(E, 1), max(E, 1), B + 1, max(Rr, 1), max(Rr, 1), max(I, 1), B + 1]
    fsz = [max(Rr, 1), max(I, 1), max(Rr, 1) * ldf] + [max(Rr, 1) * h for h in heads]
    ioff = np.concatenate([[0], np.cumsum([_a4(s + guard) for s in isz])])
    foff = np.concatenate([[0], np.cumsum([_a4(s + guard) for s in fsz])])
    ibuf = torch.empty(int(ioff[-1]), dtype=torch.int32, device=dev)
    fbuf = torch.empty(int(foff[-1]), dtype=torch.float32, device=dev)
    if guard:
        ibuf.fill_(GUARD)
        fbuf.view(torch.int32).fill_(GUARD)
    iv = [ibuf[int(o):int(o) + s] for o, s in zip(ioff, isz)]
    fv = [fbuf[int(o):int(o) + s] for o, s in zip(foff, fsz)]
    rowptr, rowptr_t, col, col_t, src_e_t, inv, graph_ptr, row_graph, row_slot, iso_idx, iso_ptr = iv
    row_mult, iso_w, x = fv[0], fv[1], fv[2].view(max(Rr, 1), ldf)
    iso_cols = {h: fv[3 + j].view(max(Rr, 1), h) for j, h in enumerate(heads)}
    if E == 0:
        for t in (col, col_t, src_e_t, inv):                 # (one unread word each; kept defined)
            t.zero_()
    if I == 0:
        iso_idx.zero_()
        iso_w.zero_()
    head = np.zeros(hw, dtype=np.int64)
    head[1:7] = (Rr, E, I, B, ldf, len(heads))
    head[7:7 + len(heads)] = heads
    head[11:25] = [t.data_ptr() for t in (rowptr, col, rowptr_t, col_t, src_e_t, inv, row_mult, graph_ptr, row_graph, row_slot, iso_idx,
                                          iso_w, iso_ptr, x)]
    for j, h in enumerate(heads):
        head[25 + j] = iso_cols[h].data_ptr()
    for s in range(0, B, kmax):
        grp = parts[s:s + kmax]
        d = np.zeros(hw + pw * len(grp), dtype=np.int64)
        d[:hw] = head
        d[0] = len(grp)
        for j, p in enumerate(grp):
            b = s + j
            d[hw + pw * j:hw + pw * (j + 1)] = (p.buf.data_ptr(), p.n, p.nr, p.nnz, p.k, p.mult, row0[b], e0[b], i0[b], b, int(b == B - 1))
        nat.call("gat_assemble_f32", d.ctypes.data)
    g = GraphBatch()
    g.layout, g.B, g.nmax, g.device = "packed", B, nmax, dev
    g.sizes, g.real_sizes = nr, np.array([p.n for p in parts], dtype=np.int64)
    g.n_rows, g.n_ghost = Rr, 0
    g.graph_ptr, g.row_graph, g.row_slot, g.slot_count = graph_ptr, row_graph, row_slot, _no_slot_counts(nmax, dev)
    g.rowptr, g.col, g.val, g.nnz, g.symmetric = rowptr, col, None, E, False
    g.row_mult = row_mult
    g._t, g.src_e_t, g._inv_e_t = (rowptr_t, col_t, None), src_e_t, inv
    g._iso_cols = iso_cols
    g._iso_list = (iso_idx, iso_w, iso_ptr, I)
    g._raw = (ibuf, fbuf, ioff, isz, foff, fsz)
    g._pieces = parts                                      # (a recorded launch replays by address: the buffers outlive the batch's use)
    return x, g


# ----------------------------------------------------------------------------- the model on a packed batch
@contextlib.contextmanager
def own_rows(model):
    """every ``DGATHead`` of the model with ``per_graph_features = True`` inside the block (every graph of the packed batch reads its
    own rows, as in the reference's B = 1 calls), the previous values after it, also on an exception"""
    heads = [m for m in model.modules() if isinstance(m, DGATHead)]
    prev = [m.__dict__.get("per_graph_features", None) for m in heads]
    for m in heads:
        m.per_graph_features = True
    try:
        yield
    finally:
        for m, v in zip(heads, prev):
            if v is None:
                del m.per_graph_features                    # (the class default was in effect)
            else:
                m.per_graph_features = v


def head_counts(model):
    layers = [model.conv_first] + (list(model.conv_block) if model.conv_block is not None else []) + [model.conv_last]
    return [len(l.attentions) for l in layers]


def dropout_active(model):
    return model.training and any(hd.dropout > 0 for hd in model.modules() if isinstance(hd, DGATHead))


def head_linear(model):
    """the Linear between readout and embedding (encoders_GAT.py:191-198): ``map_model`` for final_dim 'output_dim', else ``pred_model``"""
    return model.map_model if model.final_dim == "output_dim" else model.pred_model


def readout_rows(model, x, g):
    """max readouts [B, E] of the encoder on the packed batch (x, g): ``gcn_forward`` + the readout (encoders_GAT.py:185-189)"""
    with own_rows(model):
        r, made = model.gcn_forward(x, g, model.conv_first, model.conv_block, model.conv_last, readout=True)
        if not made:
            r = mp.readout_max(r, g)
    return r


def tail_ok(lin, map2, r):
    return (_t.FUSED_TAIL and isinstance(lin, nn.Linear) and isinstance(map2, nn.Identity) and r.is_cuda and r.dim() == 2 and r.size(0) == 3
            and r.dtype == torch.float32 and lin.in_features == r.size(1) and lin.in_features % 4 == 0 and lin.out_features <= 512
            and lin.weight.dtype == torch.float32)


def packable(model, dev):
    return R.RESIDENT and dev.type == "cuda" and not dropout_active(model)


def dense_forward(model, obj, dev, exact=None):
    """the reference's own call for one graph object (tripletnet.py:18-38) -> the embedding [1, E].  ``num_nodes`` is handed over only
    when one representative can stand for the padded rows (the module packs a B = 1 batch with it); otherwise all Nmax rows are computed"""
    d = obj.graph
    feats = np.asarray(d["feats"], dtype=np.float32)
    n = int(d["num_nodes"])
    if exact is None:
        exact = representable(np.asarray(d["adj"]), feats, n)
    adj = torch.as_tensor(np.asarray(d["adj"], dtype=np.float32)[None], device=dev)
    h0 = torch.as_tensor(feats[None], device=dev)
    return model(h0, adj, np.array([n]) if exact else None)[1]


def embed_chunk(model, graphs, dev, cache):
    """embeddings [len(graphs), E] of a chunk of graph objects: one packed batch, or one dense B = 1 call per graph when a graph of
    the chunk cannot be packed (its padded feature rows differ).  The caller holds eval mode / no_grad (``two_stage.embed_dataset``)."""
    parts = [resident_piece(o, dev, cache) for o in graphs]
    if not all(p.exact for p in parts):
        return torch.cat([dense_forward(model, o, dev, p.exact) for o, p in zip(graphs, parts)])
    x, g = assemble(parts, dev, head_counts(model))
    return model.head(readout_rows(model, x, g))


class tripletnet(nn.Module):
    """``tripletnet(model).forward(a, p, n) -> (dist_p, dist_n, embed_a, embed_p, embed_n)`` for ``model`` = a
    ``gat_encoders.DGATEncoderGraph``: always the reference's three B = 1 forwards, whatever ``per_graph_features`` is on the model.
    ``batch(a, p, n)`` / ``embed(batch)`` split the call for a step replayed from a hipGraph on a resident triplet."""

    def __init__(self, model):
        super().__init__()
        if not isinstance(model, DGATEncoderGraph):
            raise TypeError("gat_triplet.tripletnet wraps a gat_encoders.DGATEncoderGraph")
        self.model = model
        self.cache = R.cache_for(model)

    # ------------------------------------------------------------------ graphs
    def batch(self, a, p, n):
        """(feature rows, GraphBatch) of the triplet as one packed batch, or None when it takes the fallback"""
        dev = next(self.model.parameters()).device
        if not packable(self.model, dev):
            return None
        parts = [resident_piece(o, dev, self.cache) for o in (a, p, n)]
        if not all(q.exact for q in parts):
            return None
        return assemble(parts, dev, head_counts(self.model))

    # ------------------------------------------------------------------ forward
    def embed(self, b):
        m = self.model
        r = readout_rows(m, *b)
        lin = head_linear(m)
        if tail_ok(lin, m.map2_model, r):
            return _t._TripletTail.apply(r, lin.weight, lin.bias)
        return R.torch_distances(m.head(r))

    def _reference(self, trip):
        """the reference, literally: three B = 1 calls of the module on dense tensors"""
        dev = next(self.model.parameters()).device
        return R.torch_distances(torch.cat([dense_forward(self.model, o, dev) for o in trip]))

    def forward(self, a, p, n):
        """a, p, n: objects with ``.graph`` = {'adj', 'feats', 'num_nodes', ...} as cross_val.split_train_val prepares them
        ('assign_feats' is read by the reference and never used by this encoder)"""
        b = self.batch(a, p, n)
        return self.embed(b) if b is not None else self._reference((a, p, n))
