"""GAT triplet stream: a NEW triplet at every replay of ONE hipGraph for ``gat_triplet.tripletnet`` over a
``gat_encoders.DGATEncoderGraph`` (Code/sage+gat+diffpool/train_triplet.py:247-287 with --method=GAT: ``tripletsampler_tr.sampler()``
-> ``TNet(a, p, n)`` -> margin loss -> clip -> Adam, thousands of times per epoch).

``triplet_stream.TripletStream`` does this for the GraphSage family, ``diffpool_stream.TripletStream`` for DiffPool and
``sag_stream.TripletStream`` for SAGPool.  ``gat_triplet.assemble`` writes arrays whose shapes (R rows, E entries, I listed edge-less
columns) are host numbers that change with the triplet, so no captured step can hold its batch.  Here the dataset's graph objects are
packed once into a device-resident arena of the pieces the assembler already reads (``pack_arena``), an epoch's triplets go up as
one index array (``load``), and the step's first launch (``tsgnn_gat_triplet_gather_f32``, csrc/gat_stream.hip) picks the three
pieces of "schedule entry number ``cursor``" on the device, writes the batch at capacities of three times the largest piece —
everything behind the triplet's own R / E / I is inert padding — and advances the cursor.  The fused GAT layers, the readout and the
triplet tail run unchanged on that batch: its host-side sizes are the capacities, the triplet's own sizes live in the row pointers,
``graph_ptr`` and ``iso_ptr`` on the device.

``PostTrainStream`` is the same machinery at ONE piece per schedule entry (``tsgnn_gat_anchor_gather_f32``): the anchor steps of the
2stg+ post-training phase (train_triplet_pre_train.py:233-262), with the loss on the readout row.  ``MiniBatchStream`` is the
classification loop of train.py --method=GAT (train.py:104-131): a NEW batch of 1..128 graphs per replay
(``tsgnn_gat_batch_gather_f32``, csrc/gat_batch_stream.hip), at capacities that default to the sums of the ``batch`` largest pieces and
are checked per entry at ``load`` (``default_caps``, ``schedule_capacity``, ``check_fit``).  ``GatArenaStream`` holds what the three
share.

No dropout (a ghost representative is exact only while its copies stay identical); anything the stream does not take is a TypeError
that names the eager drop-in."""
import numpy as np
import torch

from . import _native as nat
from . import gat_triplet as gt
from . import resident as R
from .graph import GraphBatch
from .minibatch_stream import MAX_BATCH, MiniBatchSteps, compare, top_sum
from .post_train import AnchorSteps
from .triplet_stream import HEAD, TICKET_WORDS, Arena, ArenaStream, TripletSteps, check_schedule, schedule_of  # noqa: F401  (the stream's vocabulary)

REC_WORDS = 8          # int32 words of a graph's record: piece offset (words), n, nr, nnz, k, Nmax - n, index, 0
EAGER = "; use the eager drop-in, tripletnet.forward(a, p, n)"


def pack_arena(graphs, limit=1 << 31, batch=3):
    """graph objects (``.graph`` = {'adj', 'feats', 'num_nodes', ...} as cross_val.split_train_val prepares them) -> ``Arena``.
    ValueError, naming the graph's index, for what one ghost representative cannot stand for (``pack_host``'s ``exact`` is False: the
    padded feature rows differ, or ``adj`` is positive outside ``[:n, :n]``), for an Nmax or a feature width that differs from the
    other graphs', and for offsets that reach ``limit`` (the records are int32).  ``batch``: the pieces a schedule entry names (3: a
    triplet; 1: the anchor of a post-training step); ``caps = batch * top``.  Host work only: no GPU is touched.
    The arena's fields:
      records  int32 [G, 8]    the piece's word offset in ``buf``, n, nr, nnz, k, mult = Nmax - n, the graph's index, 0
      buf      int32 [words]   every graph's ``gat_triplet.piece_buffer`` (sections at ``tsgnn_gat_assemble_layout``'s offsets, piece-local
                               indices), one behind the other, each piece on 16 bytes
      top      (nr, nnz, k)    the largest of each over the dataset
      caps     (rows, nnz, k)  ``batch`` (3) times ``top``: no triplet needs more, also when one object fills all three places (a sampler may
                               draw an anchor as its own negative's positive; the three largest DISTINCT graphs would not cover that)
      nmax, fin, ldf           what every graph shares: the padded size, the feature width, the 16-byte row stride of the feature rows"""
    graphs = list(graphs)
    if not graphs:
        raise ValueError("pack_arena: no graphs")
    G = len(graphs)
    rec = np.zeros((G, REC_WORDS), dtype=np.int64)
    bufs = []
    nmax = fin = ldf = None
    words = 0
    for i, obj in enumerate(graphs):
        try:
            p = gt.pack_host(obj)
        except ValueError as e:
            raise ValueError("graph %d: %s" % (i, e)) from None
        if not p["exact"]:
            raise ValueError("graph %d: one representative cannot stand for its padded rows (the rows feats[n:] differ, or adj has a "
                             "positive entry outside [:n, :n])" % i)
        if nmax is None:
            nmax, fin, ldf = p["nmax"], p["fin"], int(p["feats"].shape[1])
        if p["nmax"] != nmax:
            raise ValueError("graph %d: Nmax = %d differs from the other graphs' %d" % (i, p["nmax"], nmax))
        if p["fin"] != fin:
            raise ValueError("graph %d: feature width %d differs from the other graphs' %d" % (i, p["fin"], fin))
        b = gt.piece_buffer(p)
        rec[i] = (words, p["n"], p["nr"], p["nnz"], p["k"], p["mult"], i, 0)
        bufs.append(b)
        words += int(b.size)                                                # (a piece's length is a multiple of 4 words)
        if words >= int(limit):
            raise ValueError("graph %d: pack_arena: offsets reach %d (int32 records): %d buffer words" % (i, limit, words))
    top = tuple(int(rec[:, c].max()) for c in (2, 3, 4))
    caps = tuple(int(batch) * t for t in top)
    if max(caps[0] * ldf, caps[1]) >= int(limit):
        raise ValueError("pack_arena: offsets reach %d (int32 records): a batch of %d rows x %d, %d entries" % (limit, caps[0], ldf, caps[1]))
    return Arena(records=rec.astype(np.int32), buf=np.concatenate(bufs), words=words, top=top, caps=caps, nmax=nmax, fin=fin, ldf=ldf,
                 n_graphs=G, batch=int(batch))


def _layers(model):
    return [model.conv_first] + (list(model.conv_block) if model.conv_block is not None else []) + [model.conv_last]


class GatArenaStream(ArenaStream):
    """What the GAT streams share, whatever the number ``batch`` of pieces a schedule entry names (3: ``TripletStream``; 1: the anchor
    of the 2stg+ post-training step, ``PostTrainStream``): the refusals, the arena at ``batch`` times the largest piece, the persistent
    capacity batch and the gather launch (``tsgnn_gat_triplet_gather_f32`` / ``tsgnn_gat_anchor_gather_f32``).  ``NAME`` and ``EAGER``
    (where the caller's eager drop-in is) end every TypeError."""

    NAME = "gat_stream.GatArenaStream"
    EAGER = EAGER
    ENTRY = {3: "gat_triplet_gather_f32", 1: "gat_anchor_gather_f32"}

    def _refuse_device(self, model):
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            self._refuse("runs on the GPU only")
        if not R.RESIDENT:
            self._refuse("needs the resident pieces (resident.RESIDENT is off)")
        return dev

    def _refuse_layers(self, model):
        from . import gat_fused as gf
        from .gat_encoders import DGATLayer
        layers = _layers(model)
        heads = sorted(set(gt.head_counts(model)))
        if len(heads) > 4:
            self._refuse("writes the edge-less indicator for at most four distinct head counts (%d)" % len(heads))
        if len(layers) > gf._LMAX or not all(isinstance(l, DGATLayer) and gf.heads_ok(l.attentions) for l in layers):
            self._refuse("needs layers the fused GAT kernels take (gat_fused.heads_ok, at most %d layers)" % gf._LMAX)
        return heads

    def _refuse_dropout(self, model):
        from .gat_encoders import DGATHead
        if any(hd.dropout > 0 for hd in model.modules() if isinstance(hd, DGATHead)) or any(l.dropout > 0 for l in _layers(model)):
            self._refuse("takes no attention or input dropout (a ghost representative is exact only while its copies stay identical)")

    def _build(self, model, dev, heads, graphs, batch, max_steps, caps=None, arena=None, tickets=False):
        """the arena, the capacity batch and the uploads, once the model passed the refusals.  ``caps``: (rows, entries, listed
        columns) in place of ``batch`` times the largest piece, ``arena``: ``pack_arena(graphs, batch=batch)`` where the caller has
        packed already (``MiniBatchStream``, which reads its capacities off the records and whose ``load`` checks every entry
        against them)"""
        ar = pack_arena(graphs, batch=batch) if arena is None else arena
        if ar.fin != int(model.conv_first.attentions[0].input_dim):
            raise ValueError("%s: the dataset has %d features per node, the model takes %d"
                             % (self.NAME, ar.fin, model.conv_first.attentions[0].input_dim))
        self.heads = heads
        self.row_cap, self.nnz_cap, self.iso_cap = ar.caps if caps is None else caps
        self._init_protocol(model, dev, batch, ar, max_steps, self._allocate_checked, tickets)

    def _allocate_checked(self):
        """the capacity batch, and the fused node's check on it"""
        from . import gat_fused as gf
        from .gat_encoders import _fused_layer_ok
        model = self.model
        self._allocate()
        if not all(_fused_layer_ok(l.attentions, self.g, self.row_cap) for l in _layers(model)) or not gf.readout_ok(self.g, self.row_cap):
            self._refuse("needs the fused GAT node on the gathered batch (the dataset's graphs list up to %d edge-less columns per %s)"
                         % (self.iso_cap, "triplet" if self.B == 3 else "entry"))

    def _allocate(self):
        """the persistent batch: every array ``gat_fused`` / ``attention`` look up on a ``GraphBatch``, once, at capacity (two
        allocations, every array on 16 bytes: ``gat_triplet.assemble``'s layout with R, E, I = the capacities)"""
        ar, dev, B = self.arena, self.device, self.B
        Rc, E, I = self.row_cap, max(self.nnz_cap, 1), max(self.iso_cap, 1)
        isz = [Rc + 1, Rc + 1, E, E, E, E, B + 1, Rc, Rc, I, B + 1]
        fsz = [Rc, I, Rc * ar.ldf] + [Rc * h for h in self.heads]
        ioff = np.concatenate([[0], np.cumsum([gt._a4(s) for s in isz])])
        foff = np.concatenate([[0], np.cumsum([gt._a4(s) for s in fsz])])
        self._ibuf = torch.zeros(int(ioff[-1]), dtype=torch.int32, device=dev)
        self._fbuf = torch.zeros(int(foff[-1]), dtype=torch.float32, device=dev)
        self._views(self._ibuf, self._fbuf, ioff, isz, foff, fsz)

    def _views(self, ibuf, fbuf, ioff, isz, foff, fsz):
        """the arrays as views of the two buffers, the launch's description and the ``GraphBatch`` over them (tests hand in guarded
        buffers of their own)"""
        ar, dev, B, Rc = self.arena, self.device, self.B, self.row_cap
        iv = [ibuf[int(o):int(o) + s] for o, s in zip(ioff, isz)]
        fv = [fbuf[int(o):int(o) + s] for o, s in zip(foff, fsz)]
        rowptr, rowptr_t, col, col_t, src_e_t, inv, graph_ptr, row_graph, row_slot, iso_idx, iso_ptr = iv
        row_mult, iso_w, x = fv[0], fv[1], fv[2].view(Rc, ar.ldf)
        iso_cols = {h: fv[3 + j].view(Rc, h) for j, h in enumerate(self.heads)}
        d = np.zeros(int(nat.lib().tsgnn_gat_assemble_header_words()), dtype=np.int64)
        d[1:7] = (Rc, self.nnz_cap, self.iso_cap, B, ar.ldf, len(self.heads))
        d[7:7 + len(self.heads)] = self.heads
        d[11:25] = [t.data_ptr() for t in (rowptr, col, rowptr_t, col_t, src_e_t, inv, row_mult, graph_ptr, row_graph, row_slot, iso_idx,
                                           iso_w, iso_ptr, x)]
        for j, h in enumerate(self.heads):
            d[25 + j] = iso_cols[h].data_ptr()
        g = GraphBatch()
        g.layout, g.B, g.nmax, g.device = "packed", B, ar.nmax, dev
        g.sizes = np.full(B, ar.top[0], dtype=np.int64)         # (host-side sizes are capacities; the triplet's own live on the device)
        g.real_sizes = g.sizes
        g.n_rows, g.n_ghost = Rc, 0
        g.graph_ptr, g.row_graph, g.row_slot, g.slot_count = graph_ptr, row_graph, row_slot, gt._no_slot_counts(ar.nmax, dev)
        g.rowptr, g.col, g.val, g.nnz, g.symmetric = rowptr, col, None, self.nnz_cap, False
        g.row_mult = row_mult
        g._t, g.src_e_t, g._inv_e_t = (rowptr_t, col_t, None), src_e_t, inv
        g._iso_cols = iso_cols
        g._iso_list = (iso_idx, iso_w, iso_ptr, self.iso_cap)
        g._raw = (ibuf, fbuf, ioff, isz, foff, fsz)
        self._desc, self.g, self.x = d, g, x

    def gather(self):
        """enqueue (current stream; capturable) the launch that writes the batch of the cursor's entry and advances the cursor"""
        entries, ticket = self._loaded(self.NAME)
        ar = self.arena
        nat.call(self.ENTRY[self.B], self.records, ar.n_graphs, self.buf, ar.words, ar.top[0], ar.top[1], ar.top[2],
                 entries, self.max_steps, self._sched, ticket, self._desc.ctypes.data, self.ids_out)


class TripletStream(TripletSteps, GatArenaStream):
    """``net``: a ``gat_triplet.tripletnet``; ``graphs``: the dataset's graph objects (they are packed once).  The interface of
    ``triplet_stream.TripletStream``: ``load(schedule)`` (``[T, 3]`` indices into ``graphs``), ``gather``, ``embed``,
    ``loss(criterion, target)`` (the step for ``GraphedStep``: every call, every replay, consumes the next entry), ``position``,
    ``ids_out``, ``len``; with ``max_steps`` the stream starts on the one-entry schedule [0, 0, 0].  TypeError (ending in the eager
    drop-in) for anything that is not a ``gat_triplet.tripletnet``, a model on the CPU, ``resident.RESIDENT`` off, a layer the fused
    GAT kernels do not take, more than four distinct head counts, attention or input dropout > 0 on any head (whatever the mode)."""

    NAME = "gat_stream.TripletStream"

    def __init__(self, net, graphs, max_steps=None):
        if not isinstance(net, gt.tripletnet):
            self._refuse("takes a gat_triplet.tripletnet")
        model = net.model
        dev = self._refuse_device(model)
        heads = self._refuse_layers(model)
        self._refuse_dropout(model)
        self.net = net
        self._build(model, dev, heads, graphs, 3, max_steps)
        self._warm_up_schedule()

    def embed(self):
        """gather + the encoder on the gathered batch + the triplet tail -> (dist_p, dist_n, embed_a, embed_p, embed_n), as
        ``tripletnet.forward`` returns"""
        if gt.dropout_active(self.model):
            raise RuntimeError("%s: dropout became active on the model after the stream was built%s" % (self.NAME, EAGER))
        self.gather()
        return self.net.embed((self.x, self.g))


class PostTrainStream(AnchorSteps, GatArenaStream):
    """An epoch of the 2stg+ post-training steps with --method=GAT (train_triplet_pre_train.py:233-262) from ONE hipGraph: per replay
    the one-piece gather launch (the anchor of "schedule entry number cursor"), the fused GAT layers and the readout over ONE graph's
    capacity, and the loss on the readout row.

    ``DGATEncoderGraph(final_dim='output_dim')`` returns ``(x, map2_model(map_model(x)))`` with ``x`` the max-readout row
    (encoders_GAT.py:189-198), so the driver's ``pred`` IS the readout row [1, embedding_dim]: the loss is the reference's doubled
    soft-max cross-entropy over ``embedding_dim`` columns, ``map_model`` and ``map2_model`` receive no gradient (under
    ``FlatTrainer(clip=0)`` they do not move: zero moments, which equals Adam skipping them), and a label >= ``embedding_dim`` is an
    error.  That order is a quirk of the reference, kept literally like the doubled soft-max.

    ``model``: a ``gat_encoders.DGATEncoderGraph`` with ``final_dim == 'output_dim'`` (not a tripletnet); the layer and dropout refusals
    of ``TripletStream``; TypeErrors end in ``post_train.post_train_step``.  ``load(anchors)``: [T] or [T, 1] indices into ``graphs``
    (``post_train.check_anchors``).  ``step()`` -> ``(loss, pred, out)``; the label is ``labels[ids_out[0]]``, read on the device.
    ``out = map2_model(map_model(pred))`` is what the reference's loop binds and never uses: it is computed outside the autograd graph
    (on ``pred.detach()`` under ``no_grad``), and NOT AT ALL by ``step_loss()``, the callable for ``GraphedStep`` (``step(with_out=False)``
    returns None in its place).  ``mine()`` refuses: an entry names one graph, there is no negative to mine."""

    NAME = "gat_stream.PostTrainStream"
    EAGER = "; use the eager drop-in, post_train.post_train_step(model, graph)"
    STEP_ARGS = {"with_out": False}

    def __init__(self, model, graphs, max_steps=None):
        from . import post_train as PT
        from .gat_encoders import DGATEncoderGraph
        if not isinstance(model, DGATEncoderGraph):
            self._refuse("takes a gat_encoders.DGATEncoderGraph")
        if model.final_dim != "output_dim":
            self._refuse("takes a model with final_dim = 'output_dim' (the reference's --method=GAT constructor)")
        self._refuse_dropout(model)
        graphs = list(graphs)
        labels = PT.label_table(graphs, model.pred_input_dim)     # (pred has embedding_dim columns: a label past them is an error)
        dev = self._refuse_device(model)
        heads = self._refuse_layers(model)
        self._build(model, dev, heads, graphs, 1, max_steps)
        self.n_classes = int(model.pred_input_dim)
        self.labels = torch.from_numpy(labels).to(dev)
        self._warm_up_schedule()

    def step(self, with_out=True):
        """gather launch + the encoder's readout row + the loss on it -> (loss, pred, out) of the cursor's entry"""
        from . import post_train as PT
        if gt.dropout_active(self.model):
            raise RuntimeError("%s: dropout became active on the model after the stream was built%s" % (self.NAME, self.EAGER))
        self.gather()
        pred = gt.readout_rows(self.model, self.x, self.g)
        loss = PT.row_loss(pred, self.ids_out, self.labels)
        return loss, pred, (PT.readout_out(self.model, pred) if with_out else None)


# ----------------------------------------------------------------------------- the mini-batch stream (the classification loop)
BATCH_EAGER = ("; use the eager route, MiniBatchStream.eager_loss(ids): gat_triplet.assemble of the resident pieces, gat_triplet.readout_rows, "
               "model.head and model.loss")


def size_records(graphs):
    """int64 [G, 3] of (nr, nnz, k) per graph object — rows with the ghost representative, entries, listed edge-less columns
    (``gat_triplet.pack_host``'s numbers): what the capacity helpers below read of an arena's records, without packing one
    (``schedule_capacity`` in front of the stream's constructor)"""
    out = np.zeros((len(graphs), 3), dtype=np.int64)
    for i, o in enumerate(graphs):
        p = gt.pack_host(o)
        out[i] = (p["nr"], p["nnz"], p["k"])
    return out


def _sizes3(records):
    """(nr, nnz, k) int64 [G, 3] of ``size_records``' rows or of an arena's records [G, 8]"""
    rec = np.asarray(records, dtype=np.int64)
    if rec.ndim != 2 or rec.shape[1] not in (3, REC_WORDS) or rec.shape[0] < 1:
        raise ValueError("records are size_records' [G, 3] or an arena's [G, %d]; got shape %s" % (REC_WORDS, rec.shape))
    return rec if rec.shape[1] == 3 else rec[:, 2:5]


def entry_sums(records, schedule):
    """rows, entries and listed columns of every schedule entry: int64 [T, 3] (a graph counts as often as the entry names it)"""
    return _sizes3(records)[np.asarray(schedule, dtype=np.int64)].sum(axis=1)


def default_caps(records, batch):
    """(row_cap, nnz_cap, iso_cap) no entry of ``batch`` DISTINCT graphs exceeds: the sums of the ``batch`` largest nr / nnz / k over
    the dataset, each on its own (a dataset of fewer graphs: the largest stands in for the missing ones)"""
    s = _sizes3(records)
    return tuple(top_sum(s[:, c], batch) for c in range(3))


def schedule_capacity(records, schedule):
    """the schedule's own maxima -> {row_cap, nnz_cap, iso_cap}, the constructor's keywords: the smallest capacities every entry of
    ``schedule`` fits (never below the dataset's largest piece).  The default capacity has to cover the ``batch`` largest graphs in one
    entry, which a shuffled epoch hardly ever draws; a loop that knows its schedules passes these instead"""
    s3 = _sizes3(records)
    s = np.asarray(schedule)
    s = check_schedule(s, len(s3), s.shape[1] if s.ndim == 2 else 1)
    caps = np.maximum(entry_sums(s3, s).max(axis=0), s3.max(axis=0))
    return {"row_cap": int(caps[0]), "nnz_cap": int(caps[1]), "iso_cap": int(caps[2])}


def _compare(schedule, records, batch, row_cap, nnz_cap, iso_cap):
    s3 = _sizes3(records)
    return compare(schedule, len(s3), batch, lambda s: entry_sums(s3, s), (row_cap, nnz_cap, iso_cap))


def fits_mask(schedule, records, batch, row_cap, nnz_cap, iso_cap):
    """bool [T]: the entry's rows, entries and listed columns lie within the capacities (duplicates inside an entry count as often as
    they appear).  ``check_schedule``'s ValueError for a wrong shape, a wrong dtype or an index out of range"""
    return ~_compare(schedule, records, batch, row_cap, nnz_cap, iso_cap)[2]


def check_fit(schedule, records, batch, row_cap, nnz_cap, iso_cap):
    """-> the checked int32 schedule; ValueError naming the first entry that exceeds a capacity, and the eager route"""
    s, need, over = _compare(schedule, records, batch, row_cap, nnz_cap, iso_cap)
    if over.any():
        k = int(np.argmax(over))
        raise ValueError("schedule entry %d has %d rows, %d entries and %d listed edge-less columns: more than this stream's capacity "
                         "(row_cap %d, nnz_cap %d, iso_cap %d)%s" % (k, need[k, 0], need[k, 1], need[k, 2], int(row_cap), int(nnz_cap),
                                                                      int(iso_cap), BATCH_EAGER))
    return s


class MiniBatchStream(MiniBatchSteps, GatArenaStream):
    """An epoch of the GAT classification loop (Code/sage+gat+diffpool/train.py:104-131 with --method=GAT:
    ``DGATEncoderGraph(final_dim='number_classes')``, ``model.loss(ypred, label)``, clip 2.0, Adam) from ONE hipGraph: the arena of
    ``pack_arena``, a device label table, and per replay the batch gather launch (``tsgnn_gat_batch_gather_f32``,
    csrc/gat_batch_stream.hip: the ``batch`` pieces of "schedule entry number cursor" as one packed batch at the stream's capacities,
    ``label_out`` int64 [batch]), the fused GAT layers and the readout on that batch (``gat_triplet.readout_rows``) and the fused
    head with the cross-entropy folded into its backward (``model.head``, ``model.loss``):

        st = MiniBatchStream(model, graphs, 32, max_steps=len(graphs) // 32)
        gs = GraphedStep(FlatTrainer(model, lr=1e-3, clip=2.0), st.loss())
        for epoch in ...:
            full, rest = minibatch_stream.epoch_schedule(len(graphs), 32, rng)
            st.load(full)
            for _ in range(len(full)): gs.step()
            gs.synchronize()
            ... st.eager_loss(rest) ...                          # the epoch's remainder: an exact batch

    What a batch means: at ``batch`` = 1 this is exactly the reference's loop (its default ``batch_size`` is 1).  At ``batch`` > 1 the
    reference's GAT reads graph 0's features for every graph of the batch (encoders_GAT.py:32, trap T4), so the stream runs the
    project's ``per_graph_features`` extension, as ``gat_triplet.readout_rows`` / ``own_rows`` do for the three graphs of a triplet:
    every graph reads its own rows, ONE batched step equals ``batch`` independent B = 1 reference forwards, and ``loss`` is the
    mean of their ``batch`` cross-entropies.

    ``model``: a bare ``gat_encoders.DGATEncoderGraph`` with ``final_dim != 'output_dim'`` (``ypred = pred_model(readout)`` has
    ``label_dim`` columns); the layer, head-count and dropout refusals of ``TripletStream``, and a head that ``DGATEncoderGraph.head``
    would run through library GEMMs instead of its fused launches is refused too; TypeErrors end in the eager route.  Labels:
    ``post_train.label_table(graphs, model.label_dim)``.  ``row_cap`` / ``nnz_cap`` / ``iso_cap``: the capacities (default: the sums of
    the ``batch`` largest nr / nnz / k over the dataset — any entry of distinct graphs fits; ``schedule_capacity`` gives a
    schedule's own); ``load`` checks every entry against them on the host and refuses, naming the entry, one that does not fit (the
    launch itself writes nothing for such an entry).  ``load(schedule [T, batch])``, ``fits(schedule)``, ``gather``,
    ``step() -> (loss, ypred [batch, label_dim])``, ``loss()`` (the callable for ``GraphedStep``), ``eager_step(ids)`` /
    ``eager_loss(ids)``: the same step on the exact batch of 1..``batch`` resident pieces through ``gat_triplet.assemble``, for the
    epoch's remainder (``minibatch_stream.epoch_schedule``) and entries that do not fit.  ``max_steps`` as ``TripletStream`` (the
    warm-up entry: ``batch`` copies of the smallest graph whose copies fit).  ``mine()`` refuses: an entry names a mini-batch."""

    NAME = "gat_stream.MiniBatchStream"
    EAGER = BATCH_EAGER
    SORT_COLUMN = 2                                                 # (nr: the rows with the ghost representative)

    def __init__(self, model, graphs, batch, row_cap=None, nnz_cap=None, iso_cap=None, max_steps=None):
        from . import post_train as PT
        from .gat_encoders import DGATEncoderGraph
        B = self._batch_in_range(batch)
        if not isinstance(model, DGATEncoderGraph):
            self._refuse("takes a bare gat_encoders.DGATEncoderGraph")
        if model.final_dim == "output_dim":
            self._refuse("takes a model with final_dim != 'output_dim' (train.py's constructor: final_dim = 'number_classes', whose ypred "
                         "has label_dim columns)")
        self._refuse_dropout(model)
        graphs = list(graphs)
        labels = PT.label_table(graphs, model.label_dim)
        dev = self._refuse_device(model)
        heads = self._refuse_layers(model)
        self._refuse_head(model, B, dev)
        ar = pack_arena(graphs, batch=B)                            # (once: the capacities come off its records)
        top = ar.top
        caps = [int(c) if c is not None else d for c, d in zip((row_cap, nnz_cap, iso_cap), default_caps(ar.records, B))]
        if any(c < t for c, t in zip(caps, top)):
            raise ValueError("%s: row_cap %d / nnz_cap %d / iso_cap %d lie below the dataset's largest piece (%d rows, %d entries, %d listed "
                             "edge-less columns)%s" % (self.NAME, caps[0], caps[1], caps[2], top[0], top[1], top[2], self.EAGER))
        self._build(model, dev, heads, graphs, B, max_steps, caps=tuple(caps), arena=ar, tickets=True)
        if self.row_cap * self.arena.ldf >= 1 << 31:
            raise ValueError("%s: %d rows x %d floats reach 2^31 (int32 offsets)%s" % (self.NAME, self.row_cap, self.arena.ldf, self.EAGER))
        self.n_classes = int(model.label_dim)
        self.graphs, self._host_labels = graphs, labels
        self._init_labels(labels)                                   # (label: what mp.cross_entropy takes)
        self._cache = R.cache_for(model)
        self._warm_up_schedule()

    def _refuse_head(self, model, B, dev):
        """``DGATEncoderGraph.head`` on [B, embedding_dim] readout rows must take one of its fused routes (``mp.head2`` for two
        Linears, the W2 = I form for the reference's Identity ``map2_model``): its last branch is library GEMMs without the folded
        cross-entropy, which the stream does not fall back to"""
        from . import gat_encoders as ge
        from . import message_passing as mp
        import torch.nn as nn
        r = torch.empty(B, int(model.pred_input_dim), dtype=torch.float32, device=dev)
        lin1 = model.pred_model
        fused = mp.head2_ok(r, lin1, model.map2_model) or (
            ge.FUSED_HEAD and isinstance(model.map2_model, nn.Identity) and isinstance(lin1, nn.Linear) and r.size(1) % 4 == 0
            and r.size(0) <= 1024 and lin1.out_features <= 256 and lin1.weight.data_ptr() % 16 == 0)
        if not fused:
            self._refuse("needs a head the fused head launches take at %d rows (pred_model a Linear on an embedding_dim that is a "
                         "multiple of 4, label_dim <= 256, map2_model the Identity or a Linear)" % B)

    def _capacity_words(self):
        return "the capacities (row_cap %d, nnz_cap %d, iso_cap %d)" % (self.row_cap, self.nnz_cap, self.iso_cap)

    def _checked(self, schedule):
        return check_fit(schedule, self.arena.records, self.B, self.row_cap, self.nnz_cap, self.iso_cap)

    def fits(self, schedule):
        return fits_mask(schedule, self.arena.records, self.B, self.row_cap, self.nnz_cap, self.iso_cap)

    def gather(self):
        """enqueue (current stream; capturable) the launch that writes the batch and the labels of the cursor's entry and advances the
        cursor"""
        entries, _ = self._loaded(self.NAME)
        ar = self.arena
        nat.call("gat_batch_gather_f32", self.records, ar.n_graphs, self.buf, ar.words, ar.top[0], ar.top[1], ar.top[2], self.labels,
                 entries, self.max_steps, self._sched, self._tickets, self.B, self._desc.ctypes.data, self.ids_out, self.label)

    def _head(self, x, g, label):
        r = gt.readout_rows(self.model, x, g)
        ypred = self.model.head(r)
        return self.model.loss(ypred, label), ypred

    def step(self):
        """gather launch + the encoder's readout rows + the head + the loss -> (loss, ypred [batch, label_dim]) of the cursor's entry"""
        if gt.dropout_active(self.model):
            raise RuntimeError("%s: dropout became active on the model after the stream was built%s" % (self.NAME, self.EAGER))
        return super().step()

    def _gathered(self):
        return self.x, self.g

    # ------------------------------------------------------------------ the eager route
    def eager_step(self, ids):
        """the same step on the exact batch of ``ids`` (1 to ``batch`` graphs): the resident pieces through ``gat_triplet.assemble``
        (one launch per 8 pieces, host-known sizes), the same readout, head and loss -> (loss, ypred)"""
        ids = self._checked_ids(ids)
        if gt.dropout_active(self.model):
            raise RuntimeError("%s: dropout became active on the model after the stream was built" % self.NAME)
        parts = [gt.resident_piece(self.graphs[int(i)], self.device, self._cache) for i in ids]
        x, g = gt.assemble(parts, self.device, self.heads)
        y = torch.from_numpy(self._host_labels[ids].astype(np.int64)).to(self.device)
        return self._head(x, g, y)
