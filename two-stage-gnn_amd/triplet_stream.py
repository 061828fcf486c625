"""Triplet stream: a NEW triplet at every replay of ONE hipGraph, gathered on the device (train_triplet.py:247-287: the reference's
inner loop is ``tripletsampler_tr.sampler()`` -> ``TNet(a, p, n)`` -> margin loss -> clip -> Adam, thousands of times per epoch).

``tripletnet.forward`` assembles its batch on the host side of every step (``torch.cat`` of resident pieces, ``GraphBatch.from_csr``,
row maps, the lazily built neighbour table): ~25 eager launches that no hipGraph can hold, because the batch's shape changes with
the triplet.  Here the whole dataset is packed once into a device-resident ARENA (``pack_arena``), an epoch's triplets go up as one
index array (``TripletStream.load``), and the step's first launch (``tsgnn_triplet_gather_f32``, csrc/triplet_stream.hip) writes the
capacity-padded batch (``ingest.CapacityBatch``) of "schedule entry number ``cursor``" and advances the cursor.  One captured step,
replayed T times, trains the epoch with no host work per step beyond the replay.

For the GraphSage-family step (``triplet.tripletnet`` over a ``GcnEncoderGraph`` whose conv stack runs as the fused node under
per-graph statistics); DiffPool, SAGPool, GAT and EigenGCN have streams of their own on this module's protocol (``diffpool_stream``,
``sag_stream``, ``gat_stream``, ``eigen_stream``).  The protocol — the ``[HEAD | schedule]`` buffer, the cursor, the ticket counters —
is owned here on the host (``HEAD``, ``TICKET_WORDS``, ``ArenaStream.load``) and by csrc/stream_protocol.h on the device.

``ArenaStream`` is that protocol on the host and nothing else: every family's stream derives from it.  ``SageArenaStream`` adds the
GraphSage family's capacity batch and gather launch, whatever the number of graphs a schedule entry names; ``TripletStream`` (three),
``post_train.PostTrainStream`` (one: the anchor of the 2stg+ post-training step), ``minibatch_stream.MiniBatchStream`` (1..128) and the
two DiffPool streams are its users.  ``TripletSteps`` is the step every family's triplet stream shares.
"""
import numpy as np
import torch

from . import _native as nat
from . import resident as R

HEAD = 8               # int32 words in front of the schedule: cursor and T (two int64), the ticket counter, 3 spare
TICKET_WORDS = 33 * 32   # the sharded ticket of the mini-batch launches: 32 shards and the top, each on 128 bytes of its own
REC_WORDS = 8          # int32 words of a graph's record: n, nnz, ntail, first row, first entry, first tail entry, index, 0


class Arena:
    """host arrays of a packed dataset: a record of named fields, whatever the family (each ``pack_arena`` says which its arena
    carries).  Every arena has ``records`` int32 [G, words], ``buf`` int32 [words], ``n_graphs`` and ``batch``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _graph_dict(obj):
    return obj if isinstance(obj, dict) else obj.graph


def _align4(n):
    return (int(n) + 3) & ~3


def pack_arena(graphs, nmax, ell_w=16, batch=3, limit=1 << 31):
    """graph objects (``.graph`` = {'adj', 'feats', 'num_nodes', ...} as cross_val.split_train_val prepares them, or bare dicts) ->
    ``Arena``.  ValueError, naming the graph's index, for whatever the fused per-graph stack cannot take: num_nodes outside 1..nmax, a
    weight other than 0 / 1 in adj[:n, :n], an adjacency that is not symmetric, feature widths that differ; and for offsets that
    reach ``limit`` (the records are int32).  The arena's fields:
      records  int32 [G, 8]          n, nnz, ntail, first row, first entry, first tail entry, the graph's index, 0
      buf      int32 [words]         sections ``rowptr`` | ``col`` | ``tail_ptr`` | ``tail_col`` at the word offsets ``off[...]`` (each on
                                     16 bytes); graph i's n + 1 row pointers (graph-local) start at ``first row + i``, its tail
                                     pointers likewise
      feats    float32 [nodes, ld]   ld = fin rounded up to 4, zero in the pad columns
      caps     (rows, nnz, tail)     ``batch`` times the largest n / nnz / ntail: no batch of that many graphs needs more, also when
                                     one object fills several of its places (a sampler may draw an anchor as its own negative's
                                     positive; the sum of the ``batch`` largest DISTINCT graphs would not cover that)
      largest  the largest n
    and, from ``minibatch_stream.pack_arena_tu`` / its graph-object route only: ``labels`` int32 [G] (the graphs' classes) and
    ``node_label`` int32 [nodes] or None; ``feats`` is None where the gather launch writes one-hot rows from ``node_label``"""
    if ell_w not in (4, 8, 16):
        raise ValueError("ell_w must be 4, 8 or 16")
    graphs = list(graphs)
    if not graphs:
        raise ValueError("pack_arena: no graphs")
    G, nmax = len(graphs), int(nmax)
    rec = np.zeros((G, REC_WORDS), dtype=np.int64)
    rps, cols, tps, tcs, fts = [], [], [], [], []
    fin = None
    row0 = ent0 = tail0 = 0
    for i, obj in enumerate(graphs):
        d = _graph_dict(obj)
        n = int(d["num_nodes"])
        a = np.asarray(d["adj"])
        if not 1 <= n <= nmax:
            raise ValueError("graph %d: num_nodes = %d lies outside 1..%d" % (i, n, nmax))
        if a.ndim != 2 or a.shape[0] < n or a.shape[1] < n:
            raise ValueError("graph %d: adj must hold [:num_nodes, :num_nodes]" % i)
        rp, c, v, sym = R.dense_csr_host(a, n)
        if v.size and not bool((v == 1.0).all()):
            raise ValueError("graph %d: adj[:n, :n] carries a weight other than 0 / 1 (the gather products take unit weights)" % i)
        if not sym:
            raise ValueError("graph %d: adj[:n, :n] is not symmetric" % i)
        f = np.asarray(d["feats"], dtype=np.float32)
        if f.ndim != 2 or f.shape[0] < n:
            raise ValueError("graph %d: feats must be [>= num_nodes, fin]" % i)
        if fin is None:
            fin = int(f.shape[1])
        elif int(f.shape[1]) != fin:
            raise ValueError("graph %d: feature width %d differs from the other graphs' %d" % (i, f.shape[1], fin))
        deg = np.diff(rp).astype(np.int64)
        over = np.maximum(deg - ell_w, 0)
        tp = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(over, out=tp[1:])
        # the entries beyond the first ell_w of each row, row after row (what tsgnn_host_collate_compact computes per batch)
        k = np.arange(c.size, dtype=np.int64) - np.repeat(rp[:-1].astype(np.int64), deg)
        tc = c[k >= ell_w]
        rec[i] = (n, c.size, tc.size, row0, ent0, tail0, i, 0)
        rps.append(rp.astype(np.int64)); cols.append(c.astype(np.int64)); tps.append(tp); tcs.append(tc.astype(np.int64))
        fts.append(f[:n])
        row0 += n; ent0 += c.size; tail0 += tc.size
    sec = {"rowptr": row0 + G, "col": ent0, "tail_ptr": row0 + G, "tail_col": tail0}
    off, o = {}, 0
    for name in ("rowptr", "col", "tail_ptr", "tail_col"):
        off[name] = o
        o += _align4(max(sec[name], 1))
    ld = (fin + 3) // 4 * 4
    if max(o, row0 + G, row0 * ld) >= int(limit):
        raise ValueError("pack_arena: offsets reach %d (int32 records): %d buffer words, %d nodes" % (limit, o, row0))
    buf = np.zeros(o, dtype=np.int32)
    for name, parts in (("rowptr", rps), ("col", cols), ("tail_ptr", tps), ("tail_col", tcs)):
        flat = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        buf[off[name]:off[name] + flat.size] = flat
    feats = np.zeros((row0, ld), dtype=np.float32)
    feats[:, :fin] = np.concatenate(fts)
    top = lambda col_: int(batch) * int(rec[:, col_].max())
    return Arena(records=rec.astype(np.int32), buf=buf, off=off, words=o, feats=feats, fin=fin, ld=ld, nmax=nmax, ell_w=int(ell_w),
                 batch=int(batch), caps=(top(0), top(1), top(2)), largest=int(rec[:, 0].max()), n_graphs=G, total_nodes=row0)


def check_schedule(schedule, n_graphs, batch=3):
    """int array [T, batch] of indices into the dataset -> contiguous int32 copy; ValueError for a wrong shape, an empty schedule, a
    negative index or an index >= n_graphs (the kernel trusts what ``load`` uploads)"""
    s = np.asarray(schedule)
    if s.ndim != 2 or s.shape[1] != batch or s.shape[0] < 1:
        raise ValueError("a schedule is an integer array [T, %d] with T >= 1; got shape %s" % (batch, s.shape))
    if not np.issubdtype(s.dtype, np.integer):
        raise ValueError("a schedule holds integer indices; got %s" % s.dtype)
    if int(s.min()) < 0 or int(s.max()) >= n_graphs:
        raise ValueError("schedule indices must lie in [0, %d); got [%d, %d]" % (n_graphs, int(s.min()), int(s.max())))
    return np.ascontiguousarray(s, dtype=np.int32)


def schedule_of(sampler, graphs):
    """drains a TripletSampler-shaped object (triplet_sampler.py: ``shuffle()``, ``end()``, ``sampler()`` -> {'anchor', 'pos', 'neg'})
    into the epoch's index array [T, 3]: every sampled object is looked up in ``graphs`` by identity"""
    index = {id(g): i for i, g in enumerate(graphs)}
    rows = []
    sampler.shuffle()
    while not sampler.end():
        s = sampler.sampler()
        try:
            rows.append([index[id(s[k])] for k in ("anchor", "pos", "neg")])
        except KeyError:
            raise ValueError("schedule_of: triplet %d holds an object that is not in `graphs`" % len(rows)) from None
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


class ArenaStream:
    """The stream protocol and nothing else, whatever the encoder family and whatever the number ``B`` of graphs a schedule entry names:
    the uploads of a packed dataset, the ``[HEAD | schedule]`` buffer with cursor and ticket counter, ``load``, ``mine``, ``position``
    and the views of the loaded schedule every ``gather()`` hands to its launch (``_loaded``).  A family's stream passes its model
    refusals (``_refuse``: a TypeError that starts with ``NAME`` and ends in ``EAGER``, where the caller's eager drop-in is), packs its
    arena and calls ``_init_protocol``, handing it the allocation of the capacity batch its gather launch writes; ``SageArenaStream`` below is the
    GraphSage family's."""

    NAME = "ArenaStream"
    EAGER = ""

    def _refuse(self, what):
        raise TypeError("%s %s%s" % (self.NAME, what, self.EAGER))

    def _init_protocol(self, model, device, batch, arena, max_steps, allocate, tickets=False):
        """the state every family's stream has: ``model``, ``device``, ``B`` and ``arena``, then ``allocate()`` (the family's capacity
        batch and the refusals that need it: device memory is laid out batch first, and a model refused there uploads nothing), the
        arena's uploads (``feats`` where the arena carries a table), the index output of the gather launch, the empty schedule and,
        with ``tickets``, the sharded ticket counters of a mini-batch launch"""
        self.model, self.device, self.B, self.arena = model, device, int(batch), arena
        allocate()
        self.records = torch.from_numpy(arena.records).to(device)
        self.buf = torch.from_numpy(arena.buf).to(device)
        feats = getattr(arena, "feats", None)
        self.feats = torch.from_numpy(feats).to(device) if feats is not None else None
        self.ids_out = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.max_steps = int(max_steps) if max_steps is not None else None
        # int32 [HEAD + max_steps * B]: {cursor, T} as two int64, the ticket counter (+ 3 spare words), then the schedule
        self._sched = self._host = self._parts = None
        self.T = 0
        self._tickets = torch.zeros(TICKET_WORDS, dtype=torch.int32, device=device) if tickets else None

    def _warm_up_schedule(self):
        """with ``max_steps``: the one-entry schedule of graph 0, so that a ``GraphedStep`` can be built before the first epoch's exists"""
        if self.max_steps is not None:
            if self.max_steps < 1:
                raise ValueError("max_steps must be at least 1")
            self.load(np.zeros((1, self.B), dtype=np.int64))

    def __len__(self):
        return self.T

    def _checked(self, schedule):
        return check_schedule(schedule, self.arena.n_graphs, self.B)

    def load(self, schedule):
        """validate on the host, ONE host-to-device copy ({cursor = 0, T, ticket counter = 0, schedule}), returns T.  An epoch
        boundary: it waits for the steps already enqueued (they read the buffer it overwrites).  The ticket counter goes up with it, so
        a launch that was ever cut short cannot leave the cursor stuck for the next epoch; a stream that keeps sharded ticket counters
        in a tensor of its own (``_tickets``, ``TICKET_WORDS``) has them zeroed here too."""
        s = self._checked(schedule)
        T = int(s.shape[0])
        if self._sched is None:
            if self.max_steps is None:
                self.max_steps = T
            words = HEAD + self.max_steps * self.B
            self._host = torch.zeros(words, dtype=torch.int32).pin_memory()
            self._sched = torch.zeros(words, dtype=torch.int32, device=self.device)
            self._parts = (self._sched[HEAD:], self._sched[4:HEAD])           # (made once: every later load keeps the buffer)
        if T > self.max_steps:
            raise ValueError("a schedule of %d entries exceeds this stream's buffer of %d (max_steps: captured steps hold its address)"
                             % (T, self.max_steps))
        torch.cuda.synchronize(self.device)
        h = self._host.numpy()
        h[:4].view(np.int64)[:] = (0, T)
        h[4:HEAD] = 0
        h[HEAD:HEAD + T * self.B] = s.reshape(-1)
        n = HEAD + T * self.B
        self._sched[:n].copy_(self._host[:n])
        if self._tickets is not None:
            self._tickets.zero_()
            torch.cuda.current_stream(self.device).synchronize()     # (a GraphedStep replays on a stream of its own)
        self.T = T
        return T

    def _loaded(self, name=None):
        """what every ``gather()`` starts with: RuntimeError before the first ``load``, else the views of the schedule buffer its launch
        takes -> (the entries behind ``HEAD``, the ticket words ``[4:HEAD]``).  ``name``: what the error starts with (default: the
        class's name)"""
        if self._sched is None:
            raise RuntimeError("%s: load(schedule) before the first step" % (name or type(self).__name__))
        return self._parts

    def mine(self, emb, index, hardness, count=False):
        """hard / semi-hard negative mining of the LOADED schedule, in place on the device (``mining.mine_negatives`` on
        ``self._sched[HEAD:HEAD + 3 T]`` viewed as [T, 3]): ``emb`` = ``two_stage.embed_dataset``'s rows of this stream's graphs,
        ``index`` = ``mining.class_index(sampler.graphs, graphs)``, ``hardness`` 0 nothing / 0.5 semi-hard / any other positive value
        hardest.  ``count=True`` -> a one-element int32 device tensor holding the number of entries whose negative changed (else None).

        An epoch boundary, ordered as ``load``'s copy is, by synchronising: a ``GraphedStep`` replays on a stream of its own and
        does not wait for the caller's, so this waits for the device before the launch (no replay still reads the entries it
        rewrites) and for the launch after it (every later replay, on whichever stream, finds the mined schedule).  The launch
        itself runs on the current stream, behind the ``embed_dataset`` that produced ``emb``.

        RuntimeError before ``load``, on a stream whose entries are not triplets (``post_train.PostTrainStream``), and for
        embeddings with fewer rows than the arena has graphs."""
        from . import mining
        name = type(self).__name__
        if self._sched is None or self.T < 1:
            raise RuntimeError("%s: load(schedule) before mine()" % name)
        if self.B != 3:
            raise RuntimeError("%s: a schedule entry names %d graph(s), not a triplet: there is no negative to mine" % (name, self.B))
        if emb.dim() != 2 or emb.size(0) < self.arena.n_graphs:
            raise RuntimeError("%s: embeddings of shape %s do not cover the arena's %d graphs" % (name, tuple(emb.shape), self.arena.n_graphs))
        if index.n_graphs != self.arena.n_graphs:
            raise ValueError("%s: the class index was built over %d graphs, the arena holds %d" % (name, index.n_graphs, self.arena.n_graphs))
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device) if count else None
        if mining.mode_of(hardness) == 0:
            return cnt
        torch.cuda.synchronize(self.device)
        mining.mine_negatives(emb, self._sched[HEAD:HEAD + 3 * self.T].view(self.T, 3), index, hardness, n_changed=cnt)
        torch.cuda.current_stream(self.device).synchronize()
        return cnt

    def position(self):
        """the cursor: entries consumed since ``load``.  Waits for everything enqueued on the device, whichever stream the steps
        were replayed on (a ``GraphedStep`` has a stream of its own); for tests and epoch boundaries"""
        if self._sched is None:
            return 0
        torch.cuda.synchronize(self.device)
        return int(self._sched[:2].cpu().numpy().view(np.int64)[0])


class TripletSteps:
    """the step of a triplet stream, over the family's ``embed()``"""

    def loss(self, criterion, target):
        """-> callable for ``GraphedStep``: ``embed()`` (the gather launch, the encoder on the gathered batch, the triplet tail) +
        ``criterion(dist_p, dist_n, target)``; every call (every replay) consumes the next entry"""
        def step():
            out = self.embed()
            return criterion(out[0], out[1], target)
        return step


class SageArenaStream(ArenaStream):
    """What the GraphSage-family streams share, whatever the number ``batch`` of graphs a schedule entry names (3: ``TripletStream``
    and ``diffpool_stream.TripletStream``; 1: the anchor of the 2stg+ post-training step, ``post_train.PostTrainStream``; 1..128:
    ``minibatch_stream.MiniBatchStream``): the eligibility checks, the capacity-padded batch (``ingest.CapacityBatch``) and the gather
    launch that writes it.  ``model``: a plain ``GcnEncoderGraph`` with concat and bn (``TAKES``) whose conv stack runs as the fused
    per-graph node on the gathered batch.  The two checks are methods (``_model_ok``, ``_stacks_ok``): a stream for another encoder
    family (``diffpool_stream.TripletStream``) overrides them.  ``pack``: a callable -> (``Arena``, row capacity, tail capacity) in
    place of ``pack_arena(graphs, ...)`` and the arena's bounds, run once the model and its device have passed
    (``minibatch_stream.MiniBatchStream``, whose ``load`` checks every entry against the capacities).  A feature table the arena does
    not carry (``arena.feats`` None) is not uploaded."""

    TAKES = "takes a GcnEncoderGraph with concat and bn"

    def __init__(self, model, graphs, batch, nmax=None, max_steps=None, pack=None, tickets=False):
        from .ingest import ELL_W
        if not self._model_ok(model):
            self._refuse(self.TAKES)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            self._refuse("runs on the GPU only")
        if pack is None:
            graphs = list(graphs)
            if nmax is None:
                nmax = int(np.asarray(_graph_dict(graphs[0])["adj"]).shape[0])
            ar = pack_arena(graphs, nmax, ELL_W, batch=int(batch))
            rows, _, tail = ar.caps
        else:
            ar, rows, tail = pack()
        self._init_protocol(model, dev, batch, ar, max_steps, lambda: self._allocate(rows, tail), tickets)

    def _allocate(self, rows, tail):
        """the capacity-padded batch the gather launch writes, and the model's check on it"""
        from .ingest import CapacityBatch
        ar = self.arena
        self.row_cap = (int(rows) + 31) // 32 * 32
        self.tail_cap = _align4(max(int(tail), 1))
        ghost = min(ar.nmax, ar.largest + 1)
        # (edge_cap: the compact staging layout's CSR columns, which this path never fills)
        self.batch = CapacityBatch(self.B, ar.nmax, self.row_cap, 4, ar.fin, self.device, ghost_slots=ghost, tail_cap=self.tail_cap)
        self.g, self.x = self.batch.g, self.batch.x
        if not self._stacks_ok(self.model):
            raise TypeError("%s: the model's conv stack does not run as the fused per-graph node on this dataset%s" % (self.NAME, self.EAGER))

    def _model_ok(self, model):
        """the model check, before anything is packed (a subclass for another encoder family overrides both checks)"""
        from .dense_encoders import GcnEncoderGraph
        return type(model) is GcnEncoderGraph and bool(model.concat) and bool(model.bn)

    def _stacks_ok(self, model):
        """... and on the gathered batch (self.g, self.x, self.arena exist): do the model's stacks run as the fused per-graph node?"""
        from . import dense_encoders as E, sage_stack
        convs = model.conv_stack()
        return bool(sage_stack.eligible(self.g, convs, model.bn, self.x) and E.per_graph_node_ok(self.g, convs)
                    and convs[0].input_dim == self.arena.fin)

    def gather(self):
        """enqueue (current stream; capturable) the launch that writes the batch of the cursor's entry and advances the cursor"""
        entries, ticket = self._loaded()
        ar, g, b = self.arena, self.g, self.batch
        ell, ell_w, (tail_ptr, tail_col) = g._ell
        nat.call("triplet_gather_f32", self.records, ar.n_graphs, self.buf, ar.off["rowptr"], ar.off["col"], ar.off["tail_ptr"],
                 ar.off["tail_col"], ar.words, self.feats, ar.ld, ar.caps[0], ar.caps[2], entries, self.max_steps, self._sched,
                 ticket, self.B, ar.nmax, self.row_cap, self.tail_cap, ell_w, g.graph_ptr, g.slot_count, g.row_graph, g.row_slot,
                 ell, tail_ptr, tail_col, b.ell_slots, b.tail_slots, self.x, self.x.stride(0), self.ids_out)


class TripletStream(TripletSteps, SageArenaStream):
    """``net``: a ``triplet.tripletnet`` over a ``GcnEncoderGraph``; ``graphs``: the dataset's graph objects.  Packs and uploads the
    arena once.  ``load(schedule)`` uploads an epoch's triplets ([T, 3] indices into ``graphs``) and sets the cursor to 0;
    ``loss(criterion, target)`` is the step for ``GraphedStep``: every call (every replay) consumes the next entry.  The schedule
    buffer is sized by ``max_steps`` (default: the first schedule loaded): a captured step holds its address.  With ``max_steps`` the
    stream starts on the one-entry schedule [0, 0, 0], so a ``GraphedStep`` can be built (its warm-up steps run) before the first epoch's
    schedule exists."""

    NAME = "TripletStream"
    TAKES = "takes a tripletnet over a GcnEncoderGraph with concat and bn"
    EAGER = "; use the eager drop-in, tripletnet.forward(a, p, n)"

    def __init__(self, net, graphs, nmax=None, max_steps=None):
        super().__init__(getattr(net, "model", None), graphs, 3, nmax, max_steps)
        self.net = net
        self._warm_up_schedule()

    def embed(self):
        """gather + the model on the gathered batch -> (dist_p, dist_n, embed_a, embed_p, embed_n), as ``tripletnet.forward`` returns"""
        self.gather()
        return self.net._embed(self.x, self.g, None, self.x)
