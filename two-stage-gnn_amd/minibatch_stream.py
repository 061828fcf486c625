"""Mini-batch stream: a NEW mini-batch of B graphs at every replay of ONE hipGraph, gathered on the device — the reference's
"original" setting (train.py:104-131: ``DataLoader(shuffle=True)`` -> model -> cross-entropy -> clip -> Adam, once per step).

``ingest.IngestPipeline`` feeds that loop through native collate threads, pinned staging buffers and a pull over PCIe, three slots
with one hipGraph each.  Every TU dataset the reference trains on fits in device memory many times over, so here the dataset is packed
once into the arena of ``triplet_stream`` (``pack_arena_tu`` from a CSR-resident ``tu_data.TUDataset``, or ``pack_arena`` from graph
objects), an epoch's batches go up as one index array [T, B] (``MiniBatchStream.load``), and the step's first launch
(``tsgnn_batch_gather_f32``, csrc/batch_stream.hip) writes the capacity-padded batch (``ingest.CapacityBatch``) of "schedule entry
number ``cursor``", its int64 labels and — for the TU "node-label" features (train.py:227-231) — the one-hot rows themselves:

    st = MiniBatchStream(model, ds, 32, features="node-label", max_steps=len(ds) // 32)
    gs = GraphedStep(FlatTrainer(model, lr=1e-3, clip=2.0), st.loss())
    for epoch in ...:
        full, rest = epoch_schedule(len(ds), 32, rng)            # one permutation, cut into batches (no drop_last)
        st.load(full)
        for _ in range(len(full)): gs.step()                     # no host work, no PCIe, no worker thread in the loop
        gs.synchronize()                                         # the replays run on the step's own stream: wait before eager work
        ... st.eager_loss(rest) ...                              # the epoch's remainder, an exact batch through the existing collate

For the ``GcnEncoderGraph`` family with concat and bn and a head (``final_dim`` other than 'output_dim') whose stack, readout tail and
head run as the fused node (``sage_stack.sage_stack_head``) on the capacity batch under BATCH statistics.

The slot's capacity is the sum of the ``batch`` largest graphs by default (any entry of distinct graphs fits), not ``batch`` times the
largest; ``load`` checks every entry's row and tail sums on the host, so the launch never sees one that does not fit.
"""
import numpy as np
import torch

from . import _native as nat
from .triplet_stream import HEAD, TICKET_WORDS, ArenaStream  # noqa: F401  (the stream's vocabulary)
from .triplet_stream import Arena, REC_WORDS, SageArenaStream, _align4, _graph_dict, check_schedule, pack_arena

MAX_BATCH = 128
EAGER = "; use the eager route, MiniBatchStream.eager_loss(ids) / tu_data.TUDataset.collate + model.loss(model(x, g)[1], y)"


# ----------------------------------------------------------------------------- the arena of a CSR-resident dataset
def pack_arena_tu(ds, nmax, ell_w=16, batch=3, features="table", table=None, limit=1 << 31):
    """``tu_data.TUDataset`` -> the ``Arena`` ``triplet_stream.pack_arena`` builds from the same graphs as objects, array for array,
    without a dense adjacency anywhere, plus ``labels`` (int32 [G], ``ds.graph_label``) and ``node_label`` (int32 per node, or None).
    ``features``: "table" — ``feats`` = ``table`` (float [nodes, fin]; default ``ds.features("node-feat")`` when the dataset has
    attributes, else its one-hot node labels); "node-label" — no table (``feats`` None): the gather launch writes the one-hot rows of
    ``ds.num_node_labels`` columns from ``node_label``.  ValueError, naming the graph, for a size outside 1..nmax, a column outside
    its graph, an adjacency that is not symmetric, a node label outside [0, num_node_labels); and for offsets that reach ``limit``."""
    if ell_w not in (4, 8, 16):
        raise ValueError("ell_w must be 4, 8 or 16")
    if features not in ("table", "node-label"):
        raise ValueError("features must be 'table' or 'node-label'")
    gp = np.asarray(ds.graph_ptr, dtype=np.int64)
    G, nmax = len(gp) - 1, int(nmax)
    if G < 1:
        raise ValueError("pack_arena_tu: no graphs")
    sizes = np.diff(gp)
    bad = np.flatnonzero((sizes < 1) | (sizes > nmax))
    if bad.size:
        raise ValueError("graph %d: num_nodes = %d lies outside 1..%d" % (bad[0], sizes[bad[0]], nmax))
    N = int(gp[-1])
    rowptr = np.asarray(ds.rowptr, dtype=np.int64)[:N + 1]
    nnz = int(rowptr[N])
    col = np.asarray(ds.col, dtype=np.int64)[:nnz]
    deg = np.diff(rowptr)
    ids = np.arange(G, dtype=np.int64)
    node_graph = np.repeat(ids, sizes)
    ent_graph = np.repeat(node_graph, deg)
    row0, ent0 = gp[:-1], rowptr[gp[:-1]]
    lcol = col - row0[ent_graph]
    out = np.flatnonzero((lcol < 0) | (lcol >= sizes[ent_graph]))
    if out.size:
        raise ValueError("graph %d: a column lies outside the graph" % ent_graph[out[0]])
    rows = np.repeat(np.arange(N, dtype=np.int64), deg)
    fwd, bwd = np.sort(rows * N + col), np.sort(col * N + rows)
    if not np.array_equal(fwd, bwd):
        miss = np.setdiff1d(fwd, bwd)
        raise ValueError("graph %d: the adjacency is not symmetric" % node_graph[(miss[0] if miss.size else np.setdiff1d(bwd, fwd)[0]) // N])
    over = np.maximum(deg - ell_w, 0)
    tcum = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(over, out=tcum[1:])
    tail0 = tcum[gp[:-1]]
    ntail, nnz_g = tcum[gp[1:]] - tail0, rowptr[gp[1:]] - ent0
    # the entries beyond the first ell_w of each row, row after row (what tsgnn_host_collate_compact computes per batch)
    k = np.arange(nnz, dtype=np.int64) - np.repeat(rowptr[:-1], deg)
    tc = lcol[k >= ell_w]
    rec = np.stack([sizes, nnz_g, ntail, row0, ent0, tail0, ids, np.zeros(G, dtype=np.int64)], axis=1)
    assert rec.shape[1] == REC_WORDS
    # graph g's n + 1 graph-local pointers start at first row + g
    pos, end = np.arange(N, dtype=np.int64) + node_graph, gp[1:] + ids
    rp_sec, tp_sec = np.zeros(N + G, dtype=np.int64), np.zeros(N + G, dtype=np.int64)
    rp_sec[pos], rp_sec[end] = rowptr[:N] - ent0[node_graph], nnz_g
    tp_sec[pos], tp_sec[end] = tcum[:N] - tail0[node_graph], ntail
    parts = {"rowptr": rp_sec, "col": lcol, "tail_ptr": tp_sec, "tail_col": tc}
    off, o = {}, 0
    for name in ("rowptr", "col", "tail_ptr", "tail_col"):
        off[name] = o
        o += _align4(max(parts[name].size, 1))
    node_label = None
    if ds.node_label is not None:
        nl = np.asarray(ds.node_label, dtype=np.int64)[:N]
        node_label = nl.astype(np.int32)
    if features == "node-label":
        if node_label is None:
            raise ValueError("pack_arena_tu: features='node-label' on a dataset without node labels")
        fin = int(ds.num_node_labels)
        badl = np.flatnonzero((nl < 0) | (nl >= fin))
        if badl.size:
            raise ValueError("graph %d: a node label lies outside [0, %d)" % (node_graph[badl[0]], fin))
        feats = None
    else:
        if table is None:
            table = ds.features("node-feat") if ds.node_attr is not None else ds.features("node-label")
        table = np.asarray(table, dtype=np.float32)
        if table.ndim != 2 or table.shape[0] < N:
            raise ValueError("pack_arena_tu: the feature table must be [>= %d nodes, fin]" % N)
        fin = int(table.shape[1])
    ld = (fin + 3) // 4 * 4
    if max(o, N + G, N * ld) >= int(limit):
        raise ValueError("pack_arena_tu: offsets reach %d (int32 records): %d buffer words, %d nodes" % (limit, o, N))
    buf = np.zeros(o, dtype=np.int32)
    for name, flat in parts.items():
        buf[off[name]:off[name] + flat.size] = flat
    if features == "table":
        feats = np.zeros((N, ld), dtype=np.float32)
        feats[:, :fin] = table[:N]
    top = lambda col_: int(batch) * int(rec[:, col_].max())
    return Arena(records=rec.astype(np.int32), buf=buf, off=off, words=o, feats=feats, fin=fin, ld=ld, nmax=nmax, ell_w=int(ell_w),
                 batch=int(batch), caps=(top(0), top(1), top(2)), largest=int(sizes.max()), n_graphs=G, total_nodes=N,
                 labels=np.asarray(ds.graph_label, dtype=np.int64)[:G].astype(np.int32), node_label=node_label)


def _pack_graph_objects(graphs, nmax, ell_w, batch, features, fin=None):
    """the graph-object route: ``pack_arena`` + ``labels`` (every ``graph['label']``) and ``node_label`` (``graph['node_label']``, where
    every graph carries one).  ``fin``: the width of the one-hot rows in the "node-label" mode (the dataset's number of node labels:
    a subset of a dataset need not hold the largest one); default, and whenever a label does not fit it, the largest label + 1"""
    from .post_train import _label_of
    ar = pack_arena(graphs, nmax, ell_w, batch=batch)
    ar.labels = np.asarray([_label_of(_graph_dict(o), "graph %d" % i) for i, o in enumerate(graphs)], dtype=np.int32)
    ar.node_label = None
    if all("node_label" in _graph_dict(o) for o in graphs):
        ar.node_label = np.concatenate([np.asarray(_graph_dict(o)["node_label"]).reshape(-1)[:int(_graph_dict(o)["num_nodes"])]
                                        for o in graphs]).astype(np.int32)
    if features == "node-label":
        if ar.node_label is None:
            raise ValueError("features='node-label' on a dataset without node labels")
        if int(ar.node_label.min()) < 0:
            raise ValueError("a node label is negative")
        ar.fin = max(int(ar.node_label.max()) + 1, int(fin) if fin is not None else 0)
        ar.ld = (ar.fin + 3) // 4 * 4
        ar.feats = None
    return ar


def arena_dataset(ar):
    """the arena's graphs back as a ``tu_data.TUDataset`` (one CSR over all nodes): what the existing collate reads"""
    from .tu_data import TUDataset
    rec = ar.records.astype(np.int64)
    G, n = rec.shape[0], rec[:, 0]
    gp = np.zeros(G + 1, dtype=np.int64)
    np.cumsum(n, out=gp[1:])
    N = int(gp[-1])
    ids = np.arange(G, dtype=np.int64)
    node_graph = np.repeat(ids, n)
    rp = ar.buf[ar.off["rowptr"]:].astype(np.int64)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[:N] = rp[np.arange(N, dtype=np.int64) + node_graph] + rec[node_graph, 4]
    rowptr[N] = int(rec[:, 1].sum())
    col = ar.buf[ar.off["col"]:ar.off["col"] + int(rowptr[N])].astype(np.int64) + np.repeat(rec[:, 3], rec[:, 1])
    nl = ar.node_label.astype(np.int64) if ar.node_label is not None else None
    return TUDataset(gp, rowptr, col, ar.labels.astype(np.int64), nl, None, ar.fin if ar.feats is None else 0)


# ----------------------------------------------------------------------------- schedules and capacities (host, no GPU)
def epoch_schedule(n_graphs, batch, rng):
    """one epoch of the reference's ``DataLoader(shuffle=True)`` without ``drop_last``: ONE permutation of the dataset cut into batches
    -> (full int64 [T, batch], rest int64 [n_graphs mod batch]).  ``rng``: a ``numpy.random.Generator``"""
    n_graphs, batch = int(n_graphs), int(batch)
    if n_graphs < 1 or batch < 1:
        raise ValueError("epoch_schedule: n_graphs and batch must be at least 1")
    perm = np.asarray(rng.permutation(n_graphs), dtype=np.int64)
    T = n_graphs // batch
    return perm[:T * batch].reshape(T, batch), perm[T * batch:]


def top_sum(v, batch):
    """the sum of the ``batch`` largest values of ``v`` (fewer values than ``batch``: the largest stands in for the missing ones): what
    no entry of ``batch`` DISTINCT graphs exceeds"""
    s = np.sort(np.asarray(v, dtype=np.int64))[::-1][:int(batch)]
    return int(s.sum() + (int(batch) - s.size) * s[0])


def compare(schedule, n_graphs, batch, need_of, caps):
    """the one need-versus-capacity comparison behind every family's ``fits_mask`` / ``check_fit``: ``check_schedule``'s ValueError
    for a wrong shape, a wrong dtype or an index out of range, then ``need_of(checked schedule)`` (int64 [T, C]: what every entry
    needs, duplicates inside an entry counted as often as they appear) against ``caps`` [C] -> (the checked int32 schedule, need,
    bool [T]: the entry exceeds a capacity)"""
    s = check_schedule(schedule, n_graphs, int(batch))
    need = np.asarray(need_of(s), dtype=np.int64)
    return s, need, (need > np.asarray([int(c) for c in caps], dtype=np.int64)).any(axis=1)


def default_capacity(records, batch):
    """(rows, tail entries) no entry of ``batch`` DISTINCT graphs exceeds: the sums of the ``batch`` largest n and ntail of the dataset
    (a dataset of fewer graphs: the largest stands in for the missing ones)"""
    return top_sum(records[:, 0], batch), top_sum(records[:, 2], batch)


def entry_sums(records, schedule):
    """(rows, tail entries) of every schedule entry: int64 [T] each"""
    rec = np.asarray(records, dtype=np.int64)
    return rec[schedule, 0].sum(axis=1), rec[schedule, 2].sum(axis=1)


def _compare(schedule, records, batch, row_cap, tail_cap):
    return compare(schedule, len(records), batch, lambda s: np.stack(entry_sums(records, s), axis=1), (row_cap, tail_cap))


def fits_mask(schedule, records, batch, row_cap, tail_cap):
    """bool [T]: the entry's row and tail sums lie within the capacities (duplicates inside an entry count as often as they appear).
    ``check_schedule``'s ValueError for a wrong shape, a wrong dtype or an index out of range"""
    return ~_compare(schedule, records, batch, row_cap, tail_cap)[2]


def check_fit(schedule, records, batch, row_cap, tail_cap):
    """-> the checked int32 schedule; ValueError naming the first entry that exceeds a capacity"""
    s, need, over = _compare(schedule, records, batch, row_cap, tail_cap)
    if over.any():
        k = int(np.argmax(over))
        raise ValueError("schedule entry %d has %d rows and %d tail entries: more than this stream's capacity (row_cap %d, tail_cap %d)%s"
                         % (k, need[k, 0], need[k, 1], int(row_cap), int(tail_cap), EAGER))
    return s


# ----------------------------------------------------------------------------- what the families' mini-batch streams share
class MiniBatchSteps:
    """The mini-batch layer over an ``ArenaStream``, whatever the family: the batch range, the label buffers, the ``mine()`` refusal,
    the warm-up entry, the ``ids`` of the eager route, ``step``, ``loss()`` and ``eager_loss()``.  A family supplies ``SORT_COLUMN`` (the
    record column the warm-up candidates are sorted by), ``_capacity_words()`` (how the warm-up ValueError names its capacities),
    ``fits`` / ``_checked`` over its own capacities, ``_gathered()`` (what ``_head`` takes of the gathered batch), ``_head(..., label)
    -> (loss, predictions)`` and ``eager_step(ids)``."""

    SORT_COLUMN = 0

    def _batch_in_range(self, batch):
        B = int(batch)
        if not 1 <= B <= MAX_BATCH:
            raise ValueError("%s: batch = %d lies outside 1..%d%s" % (self.NAME, B, MAX_BATCH, self.EAGER))
        return B

    def _init_labels(self, table, label=None):
        """the device label table and ``label``, the int64 [B] the gather launch writes and the loss takes (one that exists already,
        or a new one)"""
        self.labels = torch.from_numpy(table).to(self.device)
        self.label = label if label is not None else torch.zeros(self.B, dtype=torch.int64, device=self.device)

    def mine(self, *args, **kwargs):
        raise RuntimeError("%s: a schedule entry names a mini-batch, not a triplet: there is no negative to mine" % self.NAME)

    def _warm_up_schedule(self):
        """with ``max_steps``: a one-entry schedule for the ``GraphedStep``'s warm-up steps — ``batch`` copies of ONE graph, the
        smallest (by ``SORT_COLUMN``) whose copies fit every capacity.  ValueError, naming ``max_steps``, when no graph's copies fit:
        the caller then builds the step after the first ``load``"""
        if self.max_steps is not None:
            if self.max_steps < 1:
                raise ValueError("max_steps must be at least 1")
            rec = self.arena.records.astype(np.int64)
            one = np.arange(len(rec), dtype=np.int64).reshape(-1, 1).repeat(self.B, axis=1)
            ok = np.flatnonzero(self.fits(one))
            if not ok.size:
                raise ValueError("%s: max_steps asks for a warm-up entry, and %d copies of no graph fit %s; leave max_steps out and "
                                 "build the step after the first load(schedule)" % (self.NAME, self.B, self._capacity_words()))
            g = int(ok[np.argmin(rec[ok, self.SORT_COLUMN])])
            self.load(np.full((1, self.B), g, dtype=np.int64))

    def _checked_ids(self, ids):
        """the ``ids`` of ``eager_step``: 1 to ``batch`` integer indices into the dataset -> the array; ValueError otherwise"""
        ids = np.asarray(ids)
        if ids.ndim != 1 or not 1 <= ids.size <= self.B or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("eager_loss takes 1 to %d integer indices; got shape %s of %s" % (self.B, ids.shape, ids.dtype))
        if int(ids.min()) < 0 or int(ids.max()) >= self.arena.n_graphs:
            raise ValueError("indices must lie in [0, %d)" % self.arena.n_graphs)
        return ids

    def step(self):
        """gather launch + the family's forward, head and loss on the gathered batch -> (loss, predictions [batch, classes]) of the
        cursor's entry"""
        self.gather()
        return self._head(*self._gathered(), self.label)

    def loss(self):
        """-> callable for ``GraphedStep``: every call (every replay) consumes the next entry and returns its loss"""
        def step():
            return self.step()[0]
        return step

    def eager_loss(self, ids):
        return self.eager_step(ids)[0]


# ----------------------------------------------------------------------------- the stream
class MiniBatchStream(MiniBatchSteps, SageArenaStream):
    """``model``: a plain ``GcnEncoderGraph`` with concat, bn and a head (``final_dim`` other than 'output_dim') on the GPU; ``dataset``:
    a ``tu_data.TUDataset`` or a list of graph objects (``.graph`` = {'adj', 'feats', 'num_nodes', 'label'[, 'node_label']}).
    ``features``: "table" (a device feature table) or "node-label" (the launch writes the one-hot rows).  ``row_cap`` / ``tail_cap``:
    the slot's capacity (``row_cap`` rounded up to 32); default ``default_capacity``.  Anything the fused node does not take is a
    TypeError / ValueError whose message names the eager route.

    ``load(schedule)``: [T, batch] indices, every entry checked against the capacities on the host; ``fits(schedule)``: the mask.
    ``loss()``: the callable for ``GraphedStep`` — every call (every replay) consumes the next entry.  ``eager_loss(ids)``: the same
    step on the exact, unpadded batch of ``ids`` (any size up to ``batch``) built by ``TUDataset.collate``: for entries that do not
    fit and the epoch's remainder.  ``max_steps`` as ``TripletStream`` (the warm-up entry: ``batch`` copies of the smallest graph)."""

    NAME = "MiniBatchStream"
    TAKES = "takes a GcnEncoderGraph with concat, bn and a head (final_dim other than 'output_dim') under batch statistics"
    EAGER = EAGER

    def __init__(self, model, dataset, batch, nmax=None, row_cap=None, tail_cap=None, features="table", max_steps=None):
        B = self._batch_in_range(batch)
        if features not in ("table", "node-label"):
            raise ValueError("%s: features must be 'table' or 'node-label'%s" % (self.NAME, EAGER))
        self.features = features
        super().__init__(model, None, B, nmax, max_steps, pack=lambda: self._pack(model, dataset, B, nmax, row_cap, tail_cap), tickets=True)
        self._init_labels(self.arena.labels, self.batch.label)      # (label: what model.loss takes)
        self.node_label = torch.from_numpy(self.arena.node_label).to(self.device) if features == "node-label" else None
        self._table = None
        self._warm_up_schedule()

    def _pack(self, model, dataset, B, nmax, row_cap, tail_cap):
        """once the model and its device have passed: the arena of ``dataset`` and the capacities -> (arena, row_cap, tail_cap)"""
        from .ingest import ELL_W
        from .tu_data import TUDataset
        name, features = self.NAME, self.features
        try:
            if isinstance(dataset, TUDataset):
                self.dataset = dataset
                nmax = dataset.max_num_nodes() if nmax is None else nmax
                table = None
                if features == "table" and dataset.node_attr is None and dataset.node_label is None:
                    table = dataset.features("const", int(model.conv_stack()[0].input_dim))       # (train.py:233-236)
                arena = pack_arena_tu(dataset, nmax, ELL_W, batch=B, features=features, table=table)
            else:
                dataset = list(dataset)
                if nmax is None:
                    nmax = int(np.asarray(_graph_dict(dataset[0])["adj"]).shape[0])
                arena = _pack_graph_objects(dataset, nmax, ELL_W, B, features, fin=int(model.conv_stack()[0].input_dim))
                self.dataset = arena_dataset(arena)
        except ValueError as e:
            raise ValueError("%s: %s%s" % (name, e, EAGER)) from None
        fin_model = int(model.conv_stack()[0].input_dim)
        if arena.fin != fin_model:
            raise TypeError("%s: the dataset's feature width %d is not the model's %d%s" % (name, arena.fin, fin_model, EAGER))
        self.max_n, self.max_tail = int(arena.records[:, 0].max()), int(arena.records[:, 2].max())
        rows, tail = default_capacity(arena.records, B)
        row_cap = rows if row_cap is None else int(row_cap)
        tail_cap = tail if tail_cap is None else int(tail_cap)
        if row_cap < self.max_n or tail_cap < self.max_tail:
            raise ValueError("%s: row_cap %d / tail_cap %d lie below the dataset's largest graph (%d rows, %d tail entries)%s"
                             % (name, row_cap, tail_cap, self.max_n, self.max_tail, EAGER))
        return arena, row_cap, tail_cap

    def _model_ok(self, model):
        from .dense_encoders import GcnEncoderGraph
        return (type(model) is GcnEncoderGraph and bool(model.concat) and bool(model.bn) and not model.per_graph_bn
                and model._head() is not None)

    def _stacks_ok(self, model):
        """on the capacity batch under BATCH statistics: the fused stack + readout tail + head node (``GcnEncoderGraph.forward``)"""
        from . import dense_encoders as E, sage_stack
        convs, (lin1, lin2, _) = model.conv_stack(), model._head()
        if not (E.FUSED_HEAD and E.FUSED_STACK and sage_stack.eligible(self.g, convs, model.bn, self.x)
                and sage_stack.head_ok(self.g, convs, lin1, lin2)):
            raise TypeError("MiniBatchStream: the model's conv stack, readout and head do not run as the fused node "
                            "(sage_stack.eligible / head_ok) on this dataset%s" % EAGER)
        return True

    def _capacity_words(self):
        return "row_cap %d / tail_cap %d" % (self.row_cap, self.tail_cap)

    def _checked(self, schedule):
        return check_fit(schedule, self.arena.records, self.B, self.row_cap, self.tail_cap)

    def fits(self, schedule):
        return fits_mask(schedule, self.arena.records, self.B, self.row_cap, self.tail_cap)

    def gather(self):
        """enqueue (current stream; capturable) the launch that writes the batch and the labels of the cursor's entry and advances
        the cursor"""
        entries, _ = self._loaded()
        ar, g, b = self.arena, self.g, self.batch
        ell, ell_w, (tail_ptr, tail_col) = g._ell
        nat.call("batch_gather_f32", self.records, ar.n_graphs, self.buf, ar.off["rowptr"], ar.off["col"], ar.off["tail_ptr"],
                 ar.off["tail_col"], ar.words, self.feats, ar.ld, self.node_label, ar.fin, self.labels, self.max_n, self.max_tail,
                 entries, self.max_steps, self._sched, self._tickets, self.B, ar.nmax, self.row_cap, self.tail_cap, ell_w,
                 g.graph_ptr, g.slot_count, g.row_graph, g.row_slot, ell, tail_ptr, tail_col, b.ell_slots, b.tail_slots, self.x,
                 self.x.stride(0), self.ids_out, self.label)

    def _gathered(self):
        return self.x, self.g

    def _head(self, x, g, label):
        """the model on a batch -> (loss, ypred [batch, classes])"""
        ypred = self.model(x, g)[1]
        return self.model.loss(ypred, label), ypred

    # ------------------------------------------------------------------ the eager route
    def _host_table(self):
        if self._table is None:
            ar = self.arena
            if ar.feats is not None:
                self._table = ar.feats[:, :ar.fin]
            else:
                t = np.zeros((ar.total_nodes, ar.fin), dtype=np.float32)
                t[np.arange(ar.total_nodes), ar.node_label] = 1.0
                self._table = t
        return self._table

    def eager_step(self, ids):
        """the same step on the exact, unpadded batch of ``ids`` (1 to ``batch`` graphs) built by ``TUDataset.collate`` ->
        (loss, ypred)"""
        ids = self._checked_ids(ids)
        g, x, y = self.dataset.collate(ids.astype(np.int64), self.arena.nmax, self._host_table(), self.device)
        return self._head(x, g, y)
