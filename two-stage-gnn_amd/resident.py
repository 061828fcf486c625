"""What every "graph object -> device pieces -> block-diagonal batch" path shares: the cache of resident graphs, the concatenation of
CSR pieces, the host conversions, and the small helpers of the ``tripletnet`` drop-ins (``triplet`` / ``sag_triplet`` / ``eigen_triplet``)
and of stage two (``two_stage``).

The reference uploads the graphs of a triplet at every step although its sampler draws them from a fixed set of objects.  Here the
device pieces of a graph object (CSR rows and, for the families whose features are host arrays, the feature rows) are built at the
object's first use and stay on the device, in ONE ``ResidentCache`` per model (``resident_cache(model)``): every ``tripletnet`` around
a model and ``two_stage.embed_dataset`` see the same entries, so a graph is uploaded once.  An entry answers only for the object it
was built from and goes when that object dies.  A step concatenates cached pieces on the device (``concat_csr``): no PCIe traffic, no
host synchronisation.  The objects are taken to be immutable, as the reference treats them; ``TSGNN_TRIPLET_CACHE=0`` (``RESIDENT``,
read at every call, also assignable as ``triplet.RESIDENT``) rebuilds the pieces at every step.
"""
import contextlib
import os
import weakref

import numpy as np
import torch
import torch.nn.functional as F

RESIDENT = os.environ.get("TSGNN_TRIPLET_CACHE", "1") != "0"
EPS = 1e-6                      # F.pairwise_distance's default
GPU_ONLY = "two_stage_gnn_amd operators run on the GPU only (no CPU fallback)"
_MAX_RESIDENT = 1 << 17
_PER_PIECE_MAX = 8              # up to this many graphs (a triplet) every piece gets its own offset launch: nothing is uploaded


# ----------------------------------------------------------------------------- the graphs of the dataset, resident
class ResidentCache:
    """entries keyed by the identity of the object they were built from; an entry only answers for THAT object (a weak reference is
    compared on every look-up, so a recycled ``id()`` cannot hit a stale entry).  Objects that cannot be weakly referenced are kept
    alive by their entry instead.  Counters: ``hits`` / ``misses`` of look-ups, ``h2d`` = host-to-device copies of graph pieces."""

    def __init__(self):
        self._entries = {}
        self.hits = self.misses = self.h2d = 0

    def lookup(self, obj, dev_index=None):
        hit = self._entries.get((id(obj), dev_index))
        if hit is not None and hit.ref() is obj:
            self.hits += 1
            return hit
        self.misses += 1
        return None

    def store(self, obj, entry, dev_index=None):
        key = (id(obj), dev_index)
        try:
            entry.ref = weakref.ref(obj, lambda _r, k=key, e=entry: self._drop(k, e))
        except TypeError:
            entry.ref = lambda o=obj: o
        if len(self._entries) >= _MAX_RESIDENT:
            self._entries.clear()
        self._entries[key] = entry
        return entry

    def _drop(self, key, entry):
        if self._entries.get(key) is entry:
            del self._entries[key]

    def __len__(self):
        return len(self._entries)

    def items(self):
        """a snapshot of (key, entry)"""
        return list(self._entries.items())

    def __iter__(self):
        return iter(self.items())


_shared_resident = weakref.WeakKeyDictionary()


def resident_cache(model):
    """the ResidentCache of `model`: ONE per network, whatever its family, shared by every ``tripletnet`` around it and by
    ``two_stage.embed_dataset``, so a graph object uploaded by a training step is not uploaded again by an evaluation (and the reverse)"""
    c = _shared_resident.get(model)
    if c is None:
        c = _shared_resident[model] = ResidentCache()
    return c


def cache_for(model):
    """what a ``tripletnet`` keeps: the model's shared cache, or with ``RESIDENT`` off a cache of its own that only counts"""
    return resident_cache(model) if RESIDENT else ResidentCache()


_ghost = {}


def ghost_zeros(nmax, width, dev):
    """the Nmax zero feature rows of the ghost slots, one tensor per (Nmax, width, device): only ever read, by ``torch.cat``"""
    key = (nmax, width, dev.index)
    z = _ghost.get(key)
    if z is None:
        z = _ghost[key] = torch.zeros(nmax, width, dtype=torch.float32, device=dev)
    return z


# ----------------------------------------------------------------------------- CSR pieces -> one block-diagonal CSR, on the device
def offset_cat(pieces, counts, offsets, dev):
    """cat(pieces[i] + offsets[i]) with ONE add for all pieces (a chunk of a dataset has hundreds of them: two small uploads of
    host-known numbers instead of one launch per graph); counts[i] = len(pieces[i])"""
    off = torch.from_numpy(np.asarray(offsets, dtype=np.int32)).to(dev)
    cnt = torch.from_numpy(np.asarray(counts, dtype=np.int64)).to(dev)
    return torch.cat(pieces) + torch.repeat_interleave(off, cnt, output_size=int(np.sum(counts)))


def concat_csr(pieces, closing, per_piece=None):
    """pieces ``(rowptr, col, val or None, n, nnz, symmetric)`` -> ``(rowptr, col, val or None, nnz, symmetric)`` of their block-diagonal
    graph: the pieces' first n ``rowptr`` entries with a running entry offset, then ``closing`` entries equal to nnz (1, or Nmax + 1
    with empty ghost-slot rows behind the real ones); ``col[:nnz]`` with a running row offset.  No edges at all: ``col`` is
    ``zeros(1)``.  Weighted pieces beside unweighted ones: the latter count as ones.  Sizes are host-known numbers, so nothing
    synchronises.  ``per_piece``: one offset launch per piece (default up to ``_PER_PIECE_MAX`` pieces), else one ``offset_cat``."""
    pieces = list(pieces)
    dev = pieces[0][0].device
    last = len(pieces) - 1
    nnz = sum(p[4] for p in pieces)
    if per_piece is None:
        per_piece = len(pieces) <= _PER_PIECE_MAX
    own_close = per_piece and closing == 1      # (no ghost rows: the last piece's own closing entry serves, no fill launch)
    tail = [] if own_close else [torch.full((closing,), nnz, dtype=torch.int32, device=dev)]
    col = val = None
    if per_piece:
        rps, cols, e0, r0 = [], [], 0, 0
        for i, (rp, c, _, n, z, _) in enumerate(pieces):
            rp = rp[:n + 1] if own_close and i == last else rp[:n]
            rps.append(rp + e0 if e0 else rp)
            if z:
                cols.append(c[:z] + r0 if r0 else c[:z])
            e0 += z
            r0 += n
        if nnz:
            col = torch.cat(cols)
    else:
        ns, zs = [p[3] for p in pieces], [p[4] for p in pieces]
        rps = [offset_cat([p[0][:p[3]] for p in pieces], ns, np.concatenate([[0], np.cumsum(zs)[:-1]]), dev)]
        if nnz:
            col = offset_cat([p[1][:p[4]] for p in pieces], zs, np.concatenate([[0], np.cumsum(ns)[:-1]]), dev)
    weighted = any(p[2] is not None for p in pieces)
    if weighted and nnz:
        val = torch.cat([p[2][:p[4]] if p[2] is not None else torch.ones(p[4], dtype=torch.float32, device=dev) for p in pieces if p[4]])
    if not nnz:
        col = torch.zeros(1, dtype=torch.int32, device=dev)
        val = torch.zeros(1, dtype=torch.float32, device=dev) if weighted else None
    return torch.cat(rps + tail), col, val, nnz, all(p[5] for p in pieces)


# ----------------------------------------------------------------------------- host conversions (pure numpy)
def dense_csr_host(a, n):
    """weighted CSR of a[:n, :n] -> (rowptr int32[n + 1], col int32, val float32, symmetric): columns ascend inside a row (as
    GraphBatch.from_dense fills them); whatever lies outside [:n, :n] is padding"""
    sub = np.asarray(a, dtype=np.float32)[:n, :n]
    r, c = np.nonzero(sub)
    rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    return rp, c.astype(np.int32), np.ascontiguousarray(sub[r, c]), bool(np.array_equal(sub, sub.T))


def padded_rows(f, n, dev):
    """the first n rows of the host array f on `dev`, zero-padded to a row stride that is a multiple of 4 floats (16-byte rows for
    the float4 gather)"""
    f = np.asarray(f, dtype=np.float32)[:n]
    out = np.zeros((n, (f.shape[1] + 3) // 4 * 4), dtype=np.float32)
    out[:, :f.shape[1]] = f
    return torch.from_numpy(out).to(dev)


# ----------------------------------------------------------------------------- the small shared pieces of the drop-ins
@contextlib.contextmanager
def per_graph_statistics(model):
    """``model.per_graph_bn = True`` inside the block (every graph of a batch on the batch-norm statistics it has alone, as in the
    reference's B = 1 calls), the previous value after it, also on an exception; a model without the attribute is left alone"""
    if not hasattr(model, "per_graph_bn"):
        yield
        return
    prev = model.per_graph_bn
    model.per_graph_bn = True
    try:
        yield
    finally:
        model.per_graph_bn = prev


def torch_distances(embed):
    """embeddings [3, E] -> (dist_p, dist_n, embed_a, embed_p, embed_n) as the reference composes them: the answer for a head the
    fused tails do not take"""
    a, p, n = embed[0:1], embed[1:2], embed[2:3]
    return F.pairwise_distance(a, p, 2), F.pairwise_distance(a, n, 2), a, p, n
