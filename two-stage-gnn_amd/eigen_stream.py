"""EigenGCN triplet stream: a NEW triplet at every replay of ONE hipGraph for ``eigen_triplet.tripletnet`` over an
``eigen_encoders.WavePoolingGcnEncoder`` (Code/eigengcn/train_triplet.py:289-317: ``tripletsampler_tr.sampler()`` -> ``TNet(a, p, n)``
-> margin loss -> clip -> Adam, thousands of times per epoch).

``triplet_stream.TripletStream`` does this for the GraphSage family, ``diffpool_stream.TripletStream`` for DiffPool,
``sag_stream.TripletStream`` for SAGPool and ``gat_stream.TripletStream`` for GAT.  ``tripletnet.batch`` rebuilds an ``EigenBatch``
whose shapes (R_i rows, E_i entries per level graph) are host numbers that change with the triplet, so no captured step can hold its
batch.  Here the dataset's graph objects are packed once into a device-resident arena of the pieces the chunk assembler already
reads (``pack_arena``), an epoch's triplets go up as one index array (``load``), and the step's first launch
(``tsgnn_eigen_triplet_gather_f32``, csrc/eigen_stream.hip) picks the three pieces of "schedule entry number ``cursor``" on the
device, writes the whole three-graph ``EigenBatch`` at capacities of three times the largest piece per level — everything behind the
triplet's own R_i / E_i is inert padding — and advances the cursor.  ``tripletnet.embed``, the encoder, the fused level-0 node and
both tails run unchanged on that batch: its host-side sizes are the capacities, the triplet's own sizes live in the row pointers,
``graph_ptr`` and the bucket pointers on the device.  The one launch that differs is the pooling forward, which also zeroes the
padding rows of the pooled level (``tsgnn_eigen_pool_fwd_cap_f32``): the pooled-level stack forms X^T dY over every row.

No dropout (a padding row must stay a function of nothing); anything the stream does not take is a TypeError that names the eager
drop-in.

The second half of 2stg+ (Code/eigengcn/train_triplet_pre_train.py:170-249: one step of the TRIPLET phase's Adam on the sampler's
anchor at B = 1, ``model.loss(ypred, label)``; the driver's ``model.map_model`` is never read by ``forward``) is ``PostTrainStream`` on the
same machinery at ONE piece per entry (``EigenArenaStream`` holds what the two streams share; ``tsgnn_eigen_anchor_gather_f32``;
``pred_model`` and the cross-entropy in one launch each way, ``post_train.apply_mlp2_ce``), ``post_train_step`` its eager drop-in and
``evaluate_pred`` the driver's ``evaluate()``."""
import numpy as np
import torch

from . import _native as nat
from . import eigen_pool as ep
from . import eigen_triplet as et
from . import resident as R
from .graph import GraphBatch
from .post_train import AnchorSteps
from .triplet_stream import HEAD, Arena, ArenaStream, TripletSteps, check_schedule, schedule_of  # noqa: F401  (the stream's vocabulary)

REC_WORDS = 12         # int32 words of a graph's record: piece offset (words), index, n[0..3], nnz[0..3], 0, 0
LMAX = 4               # level graphs a record holds (max_levels() + 1)
EAGER = "; use the eager drop-in, tripletnet.forward(a, p, n)"


def pack_arena(graphs, L, J, Jf, limit=1 << 31, batch=3):
    """graph objects (``.graph`` = {'adj', 'feats', 'num_nodes', 'adj_pool_i', 'num_nodes_i', 'pool_adj_i_j'} as cross_val.py prepares
    them, or bare dicts) -> ``Arena``.  ValueError, naming the graph's index (and the level where one is at fault), for whatever
    ``check_dict`` / ``pack_host`` reject, for an Nmax, a feature width or (L, J, Jf) that differs from the other graphs', for a level
    adjacency that is not symmetric, for more levels than the assembler takes and for offsets that reach ``limit`` (the records are
    int32).  Host work only: no GPU is touched.  The arena's fields:
      records  int32 [G, 12]   the piece's word offset in ``buf``, the graph's index, n[0..3], nnz[0..3] (unused levels 0), 0, 0
      buf      int32 [words]   every graph's ``eigen_triplet.piece_buffer`` (sections at ``tsgnn_eigen_assemble_layout``'s offsets,
                               piece-local indices), one behind the other, each piece on 16 bytes
      top      (n [L + 1], nnz [L + 1])   the largest of each per level graph over the dataset
      caps     (rows [L + 1], nnz [L + 1])   ``batch`` (3: a triplet; 1: the anchor of the post-training step) times ``top``: no entry
                               needs more, also when one object fills every place (a sampler may draw an anchor as its own
                               negative's positive; the three largest DISTINCT graphs would not cover that)
      nmax, fin, ldf, L, J, Jf   what every graph shares: the padded size, the feature width, the 16-byte row stride of the feature
                               rows, the pooling levels and the pooling / final matrices per level"""
    graphs = list(graphs)
    L, J, Jf = int(L), int(J), int(Jf)
    if not graphs:
        raise ValueError("pack_arena: no graphs")
    if L > et.max_levels():
        raise ValueError("pack_arena: %d pooling levels, the assembler takes up to %d" % (L, et.max_levels()))
    G, nlev = len(graphs), L + 1
    rec = np.zeros((G, REC_WORDS), dtype=np.int64)
    bufs = []
    nmax = fin = ldf = None
    words = 0
    for i, obj in enumerate(graphs):
        d = et.graph_dict(obj)
        try:
            et.check_dict(d, L, J, Jf)
            p = et.pack_host(d, L, J, Jf)
            rows = et.padded_rows_host(d["feats"], p["n"][0])
        except ValueError as e:
            raise ValueError("graph %d: %s" % (i, e)) from None
        f = int(np.asarray(d["feats"]).shape[1])
        if nmax is None:
            nmax, fin, ldf = int(p["nmax"]), f, int(rows.shape[1])
        if int(p["nmax"]) != nmax:
            raise ValueError("graph %d: Nmax = %d differs from the other graphs' %d" % (i, p["nmax"], nmax))
        if f != fin:
            raise ValueError("graph %d: feature width %d differs from the other graphs' %d" % (i, f, fin))
        for lev, c in enumerate(p["graphs"]):
            if not c[3]:
                raise ValueError("graph %d, level %d: the adjacency is not symmetric (a gathered batch has no transposed CSR, and "
                                 "GraphBatch.transposed() builds one from host sizes)" % (i, lev))
        b, _ = et.piece_buffer(p, rows, J)
        n, z = [int(v) for v in p["n"]], [int(c[1].size) for c in p["graphs"]]
        rec[i, 0], rec[i, 1] = words, i
        rec[i, 2:2 + nlev], rec[i, 2 + LMAX:2 + LMAX + nlev] = n, z
        bufs.append(b)
        words += int(b.size)                                                # (a piece's length is a multiple of 4 words)
        if words >= int(limit):
            raise ValueError("graph %d: pack_arena: offsets reach %d (int32 records): %d buffer words" % (i, limit, words))
    top = (tuple(int(v) for v in rec[:, 2:2 + nlev].max(axis=0)), tuple(int(v) for v in rec[:, 2 + LMAX:2 + LMAX + nlev].max(axis=0)))
    caps = (tuple(int(batch) * t for t in top[0]), tuple(int(batch) * t for t in top[1]))
    most = max([(caps[0][0] + nmax) * ldf] + list(caps[1]) + [r * max(J, Jf, 1) for r in caps[0]])
    if most >= int(limit):
        raise ValueError("pack_arena: offsets reach %d (int32 records): a batch of %d + %d rows x %d, %d entries"
                         % (limit, caps[0][0], nmax, ldf, max(caps[1])))
    return Arena(records=rec.astype(np.int32), buf=np.concatenate(bufs), words=words, top=top, caps=caps, nmax=nmax, fin=fin, ldf=ldf,
                 L=L, J=J, Jf=Jf, n_graphs=G, batch=int(batch))


def _convs(model):
    from .dense_encoders import GraphConv
    return [m for m in model.modules() if isinstance(m, GraphConv)]


class EigenArenaStream(ArenaStream):
    """What the EigenGCN streams share, whatever the number ``B`` of graphs a schedule entry names (3: ``TripletStream``; 1:
    ``PostTrainStream``): the model refusals (TypeError ending in the stream's eager drop-in), the arena upload, the allocation, layout
    and views of the persistent ``EigenBatch`` at ``B`` times the largest piece per level, and the gather launch (``GATHER``: its entry
    point)."""

    NAME = "eigen_stream.EigenArenaStream"
    EAGER = EAGER
    GATHER = "eigen_triplet_gather_f32"

    def _check_model(self, model, L):
        """the refusals every EigenGCN stream shares -> the model's device"""
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            self._refuse("runs on the GPU only")
        if not R.RESIDENT:
            self._refuse("needs the resident pieces (resident.RESIDENT is off)")
        if any(c.dropout > 0 for c in _convs(model)):
            self._refuse("takes no dropout in a conv layer (a padding row must stay a function of nothing)")
        if L > et.max_levels():
            self._refuse("takes up to %d pooling levels (the model has %d)" % (et.max_levels(), L))
        return dev

    def _init_arena(self, model, graphs, dev, shape, batch, max_steps):
        """pack and upload the dataset, allocate the batch at ``batch`` times the largest piece per level; ``shape`` = (L, J, Jf)"""
        ar = pack_arena(graphs, *shape, batch=batch)
        if ar.fin != int(model.conv_first.input_dim):
            raise ValueError("%s: the dataset has %d features per node, the model takes %d" % (self.NAME, ar.fin, model.conv_first.input_dim))
        self.row_caps, self.nnz_caps = ar.caps
        self._top = (np.array(ar.top[0], dtype=np.int64), np.array(ar.top[1], dtype=np.int64))
        self._init_protocol(model, dev, batch, ar, max_steps, self._allocate)

    def layout(self, guard=0):
        """(ioff, isz, foff, fsz): ``eigen_triplet.assemble``'s two-buffer layout with R_i, E_i = the capacities; ``guard`` words behind
        every array (tests)"""
        ar, B = self.arena, self.B
        Rc, E, nlev = self.row_caps, self.nnz_caps, ar.L + 1
        isz, fsz = [], []
        for i in range(nlev):                                    # rowptr, col, graph_ptr, row_graph, row_slot, slot_count | val
            isz += [Rc[i] + ar.nmax + 1, max(E[i], 1), B + 1, Rc[i], Rc[i], ar.nmax]
            fsz.append(max(E[i], 1))
        for i in range(ar.L):                                    # cluster_of, bptr, members | coef
            isz += [Rc[i], Rc[i + 1] + B + 1, Rc[i]]
            fsz.append(Rc[i] * ar.J)
        fsz += [Rc[ar.L] * ar.Jf, (Rc[0] + ar.nmax) * ar.ldf]
        ioff = np.concatenate([[0], np.cumsum([et._a4(s + guard) for s in isz])])
        foff = np.concatenate([[0], np.cumsum([et._a4(s + guard) for s in fsz])])
        return ioff, isz, foff, fsz

    def _allocate(self):
        """the persistent batch: every array of the ``EigenBatch``, once, at capacity (two allocations, every array on 16 bytes)"""
        ioff, isz, foff, fsz = self.layout()
        self._ibuf = torch.zeros(int(ioff[-1]), dtype=torch.int32, device=self.device)
        self._fbuf = torch.zeros(int(foff[-1]), dtype=torch.float32, device=self.device)
        self._views(self._ibuf, self._fbuf, ioff, isz, foff, fsz)

    def _views(self, ibuf, fbuf, ioff, isz, foff, fsz):
        """the arrays as views of the two buffers, the launch's description and the ``EigenBatch`` over them (tests hand in guarded
        buffers of their own)"""
        ar, dev, B = self.arena, self.device, self.B
        Rc, E, nmax, L, J, Jf = self.row_caps, self.nnz_caps, ar.nmax, ar.L, ar.J, ar.Jf
        nlev = L + 1
        iv = [ibuf[int(o):int(o) + s] for o, s in zip(ioff, isz)]
        fv = [fbuf[int(o):int(o) + s] for o, s in zip(foff, fsz)]
        d = np.zeros(int(nat.lib().tsgnn_eigen_assemble_header_words()), dtype=np.int64)
        d[0:8] = (B, B, nlev, J, Jf, ar.ldf, nmax, 1)
        d[9], d[10] = fv[-1].data_ptr(), fv[-2].data_ptr() if Jf else 0
        gs = []
        for i in range(nlev):
            d[12 + 2 * i], d[13 + 2 * i] = Rc[i], E[i]
            a = iv[6 * i:6 * i + 6]
            d[20 + 7 * i:27 + 7 * i] = [a[0].data_ptr(), a[1].data_ptr(), fv[i].data_ptr()] + [t.data_ptr() for t in a[2:]]
            g = GraphBatch()
            g.layout, g.B, g.nmax, g.device = "packed", B, nmax, dev
            g.sizes = np.full(B, ar.top[0][i], dtype=np.int64)      # (host-side sizes are capacities; the triplet's own live on the device)
            g.n_rows, g.n_ghost = Rc[i], nmax
            g.rowptr, g.col, g.graph_ptr, g.row_graph, g.row_slot, g.slot_count = a
            g.val, g.nnz, g.symmetric = fv[i], E[i], True           # (pack_arena refused every graph that is not)
            g.capacity = True                                       # what eigen_pool._EigenPool asks of a pooled level
            gs.append(g)
        levels = []
        for i in range(L):
            a = iv[6 * nlev + 3 * i:6 * nlev + 3 * i + 3]
            d[48 + 4 * i:52 + 4 * i] = (a[0].data_ptr(), fv[nlev + i].data_ptr(), a[1].data_ptr(), a[2].data_ptr())
            lv = ep.EigenLevel()
            lv.g, lv.J = gs[i + 1], J
            lv.cluster_of, lv.bptr, lv.members = a
            lv.coef = fv[nlev + i].view(Rc[i], J)
            levels.append(lv)
        eb = ep.EigenBatch(gs[0], levels, fv[-2].view(Rc[L], Jf) if Jf else None, nmax)
        eb._raw = (ibuf, fbuf, ioff, isz, foff, fsz)
        b = et._Triplet()
        b.eb, b.x, b.sizes = eb, fv[-1].view(Rc[0] + nmax, ar.ldf), gs[0].sizes
        self._desc, self.batch, self.eb, self.x = d, b, eb, b.x

    def gather(self):
        """enqueue (current stream; capturable) the launch that writes the batch of the cursor's entry and advances the cursor"""
        entries, ticket = self._loaded(self.NAME)
        ar = self.arena
        nat.call(self.GATHER, self.records, ar.n_graphs, self.buf, ar.words, self._top[0].ctypes.data,
                 self._top[1].ctypes.data, entries, self.max_steps, self._sched, ticket, self._desc.ctypes.data, self.ids_out)


class TripletStream(TripletSteps, EigenArenaStream):
    """``net``: an ``eigen_triplet.tripletnet``; ``graphs``: the dataset's graph objects (they are packed once).  The interface of
    ``triplet_stream.TripletStream``: ``load(schedule)`` (``[T, 3]`` indices into ``graphs``), ``gather``, ``embed``,
    ``loss(criterion, target)`` (the step for ``GraphedStep``: every call, every replay, consumes the next entry), ``position``,
    ``ids_out``, ``len``; with ``max_steps`` the stream starts on the one-entry schedule [0, 0, 0].  TypeError (ending in the eager
    drop-in) for anything that is not an ``eigen_triplet.tripletnet``, a model on the CPU, ``resident.RESIDENT`` off, a conv layer
    with dropout > 0, more pooling levels than the assembler takes; ValueError for a dataset whose feature width is not the model's
    (and whatever ``pack_arena`` refuses)."""

    NAME = "eigen_stream.TripletStream"

    def __init__(self, net, graphs, max_steps=None):
        if not isinstance(net, et.tripletnet):
            self._refuse("takes an eigen_triplet.tripletnet")
        model = net.model
        dev = self._check_model(model, net.L)
        self.net = net
        self._init_arena(model, graphs, dev, (net.L, net.J, net.Jf), 3, max_steps)
        self._warm_up_schedule()

    def embed(self):
        """gather + the encoder on the gathered batch + the triplet tail -> (dist_p, dist_n, embed_a, embed_p, embed_n), as
        ``tripletnet.forward`` returns"""
        if self.model.training and any(c.dropout > 0 for c in _convs(self.model)):
            raise RuntimeError("%s: dropout became active on the model after the stream was built%s" % (self.NAME, EAGER))
        self.gather()
        return self.net.embed(self.batch)


# ----------------------------------------------------------------------------- the post-training phase of 2stg+ (streamed)
POST_EAGER = "; use the eager drop-in, eigen_stream.post_train_step(model, graph)"


class PostTrainStream(AnchorSteps, EigenArenaStream):
    """An epoch of EigenGCN post-training steps (Code/eigengcn/train_triplet_pre_train.py:192-247: one optimiser step on the sampler's
    ANCHOR at B = 1, ``loss = model.loss(model(...), label)``) from ONE hipGraph: the arena of ``pack_arena(..., batch=1)``, a device
    label table, and per replay the anchor gather launch (``tsgnn_eigen_anchor_gather_f32``: the whole one-graph ``EigenBatch`` of
    "schedule entry number cursor" at capacities of the largest piece per level), ``model(x, eb, readout_only=True)`` under per-graph
    statistics and ``pred_model`` with the cross-entropy in one launch each way (``tsgnn_posttrain_mlp2_ce_*``), whose label is
    ``labels[ids_out[0]]`` read on the device.

    ``model``: a bare ``WavePoolingGcnEncoder`` (what ``TripletStream`` takes under its ``tripletnet``); a ``map_model`` the caller
    installed, as the reference does, is never read.  Labels: ``graph.graph['label']`` against ``label_dim``
    (``post_train.label_table``).  ``load(anchors)``: [T] or [T, 1] indices into ``graphs`` (``schedule_of(sampler, graphs)[:, :1]`` is
    the reference's epoch); ``step()`` -> (loss, ypred); ``step_loss()`` is the callable for ``GraphedStep``.  The reference steps
    the TRIPLET phase's Adam here: hand ``step_loss()`` to that phase's own ``FlatTrainer``, whose moments continue.

    COMPOSED, not fused: a one-layer ``pred_model``, or one outside ``tsgnn_posttrain_mlp2_ce_supported``, runs ``pred_model`` as torch
    modules and ``mp.cross_entropy`` on a device label written from ``labels[ids_out]`` (an index launch and a cast per step)."""

    NAME = "eigen_stream.PostTrainStream"
    EAGER = POST_EAGER
    GATHER = "eigen_anchor_gather_f32"

    def __init__(self, model, graphs, max_steps=None):
        from . import post_train as PT
        from .eigen_encoders import WavePoolingGcnEncoder
        if type(model) is not WavePoolingGcnEncoder:
            self._refuse("takes a bare eigen_encoders.WavePoolingGcnEncoder")
        shape = et.model_shape(model)
        dev = self._check_model(model, shape[0])
        graphs = list(graphs)
        table = PT.label_table(graphs, int(model.label_dim))
        self._init_arena(model, graphs, dev, shape, 1, max_steps)
        self.n_classes = int(model.label_dim)
        self.labels = torch.from_numpy(table).to(dev)
        self._warm_up_schedule()

    def step(self):
        """gather launch + the encoder's readout row + ``pred_model`` and the loss -> (loss, ypred) of the cursor's entry"""
        from . import post_train as PT
        if self.model.training and any(c.dropout > 0 for c in _convs(self.model)):
            raise RuntimeError("%s: dropout became active on the model after the stream was built%s" % (self.NAME, self.EAGER))
        self.gather()
        with R.per_graph_statistics(self.model):
            r = self.model(self.x, self.eb, readout_only=True)
        return PT.apply_mlp2_ce(self.model, r, self.ids_out, self.labels)


# ----------------------------------------------------------------------------- the post-training phase of 2stg+ (eager)
def post_train_step(model, graph):
    """forward of the reference's post-training step (Code/eigengcn/train_triplet_pre_train.py:192-247: ``ypred = model(...)`` on the
    sampler's ANCHOR at B = 1 under ``model.train()``, ``loss = model.loss(ypred, label)`` = ``F.cross_entropy`` over ``label_dim``
    columns) on one graph object (or bare ``.graph`` dict) -> (loss, ypred); the caller runs ``backward`` and the optimiser — the
    reference steps the TRIPLET phase's Adam (its moments and step count continue, with its lr, weight decay and clip), so hand this
    loss to that ``FlatTrainer``, not to a new one.  A ``map_model`` the caller installed (the reference's dead ``pred_model``) is
    never read.

    The graph's resident piece (the model's ``ResidentCache``, shared with ``eigen_triplet.tripletnet`` and ``embed_dataset``) goes
    through ``eigen_triplet.assemble`` at B = 1, the encoder runs under per-graph statistics up to its readout row, and
    ``pred_model`` = Linear - ReLU - Linear with the loss is one launch each way (``post_train.apply_mlp2_ce``); a one-layer
    ``pred_model``, or one outside ``tsgnn_posttrain_mlp2_ce_supported``, is ``pred_model`` + ``mp.cross_entropy`` composed."""
    from . import post_train as PT
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError(R.GPU_ONLY)
    L, J, Jf = et.model_shape(model)
    d = et.graph_dict(graph)
    label = PT._label_of(d)
    if not 0 <= label < int(model.label_dim):
        raise ValueError("label %d lies outside [0, %d)" % (label, int(model.label_dim)))
    if R.RESIDENT and L <= et.max_levels():
        x, eb = et.assemble([et.resident_graph(graph, dev, R.resident_cache(model), L, J, Jf, check=True)], dev)
    else:
        et.check_dict(d, L, J, Jf)
        eb, feats, _ = et.to_device(et.pack_host(d, L, J, Jf), d["feats"], dev)
        x = torch.cat([feats, R.ghost_zeros(eb.nmax, feats.size(1), dev)])
    with R.per_graph_statistics(model):
        r = model(x, eb, readout_only=True)
    return PT.apply_mlp2_ce(model, r, PT._const_i32(dev, 0), PT._const_i32(dev, label))


def predict_pred(graphs, model, chunk=None):
    """class index per graph, int32 on the model's device: the arg-max (a tie to the lowest class) of the graph's
    ``two_stage.embed_dataset`` row, which for a ``WavePoolingGcnEncoder`` is ``ypred`` of the eval-mode B = 1 call"""
    from . import two_stage as TS
    z = TS.embed_dataset(model, graphs, chunk)
    if int(z.size(0)) == 0:
        return torch.zeros(0, dtype=torch.int32, device=z.device)
    return (z == z.max(dim=1, keepdim=True).values).int().argmax(dim=1).int()      # (the first maximum: the lowest class)


def evaluate_pred(graphs, model, chunk=None):
    """the phase's ``evaluate()`` (Code/eigengcn/train_triplet_pre_train.py:30-90: the arg-max of ``ypred`` against the label) ->
    {'prec' (macro), 'recall' (macro), 'acc', 'F1' (micro)} through ``two_stage.confusion_matrix`` / ``metrics_from_confusion``.
    ``graphs``: a ``{class: [graphs]}`` dictionary (iteration order kept) or a sequence; ONE copy of the predictions to the host."""
    from . import two_stage as TS
    graphs = TS._flatten(graphs)
    y = TS._labels(graphs).reshape(-1)
    pred = predict_pred(graphs, model, chunk).cpu().numpy().astype(np.int64)
    labels = np.unique(np.concatenate([y.astype(np.int64), pred]))
    return TS.metrics_from_confusion(TS.confusion_matrix(y, pred, labels))
