"""Hard and semi-hard negative mining for the triplet streams, on the device (the reference's ``TripletSampler.sampler(embed,
hardness)`` / ``exhaust_sample(embed, hardness)``: Code/sage+gat+diffpool/triplet_sampler.py:51-77, word for word in the other three
sampler files).

The reference mines while it samples, one ``np.linalg.norm`` call per (anchor, candidate) pair on the host.  Hardness consumes no
random numbers, so the mined epoch is the DRAWN epoch with column 2 rewritten: the streams upload the drawn schedule
(``triplet_stream.schedule_of`` + ``ArenaStream.load``), ``two_stage.embed_dataset`` leaves the embeddings on the device, and one
launch between them (``tsgnn_mine_negatives_f32``, csrc/mine.hip) rewrites the negatives where the gather kernels read them:

    emb = two_stage.embed_dataset(net, graphs)
    stream.load(schedule_of(sampler, graphs))
    stream.mine(emb, class_index(sampler.graphs, graphs), hardness)
    # T replays

Semantics, on exact squared distances d2(a, j) = sum_d (x_a,d - x_j,d)^2 in difference form.  The class of an entry's drawn negative
is the negative class; its candidates are that class's list, in the SAMPLER'S list order (after the epoch's ``shuffle()``).
  hardness == 0.5   semi-hard: the first candidate in list order with d(a, j) < d(a, pos); none: the drawn negative stays
  other positive    hardest: start from the drawn negative, walk the candidates in list order, take one only when it is strictly
                    closer than the best so far (the drawn negative wins a tie for the minimum; among other tied candidates the
                    earliest list position wins)
  0 (or negative)   nothing happens (the reference's ``if hardness > 0``)
"""
import numpy as np
import torch

from . import _native as nat

SEMI_HARD, HARDEST = 1, 2


def mode_of(hardness):
    """the reference's dispatch: 0 -> nothing, 1 -> semi-hard (hardness == 0.5), 2 -> hardest (any other positive hardness)"""
    h = float(hardness)
    if not h > 0:
        return 0
    return SEMI_HARD if h == 0.5 else HARDEST


class ClassIndex:
    """``class_index``'s result.  Host arrays, all int32:
      class_of   [n_graphs]        class index (position of the class in the dictionary) of every graph; -1 for a graph no list holds
      class_ptr  [n_classes + 1]   class c's candidates are members[class_ptr[c] : class_ptr[c + 1]]
      members    [class_ptr[-1]]   dataset indices, each class in the sampler's list order
    ``keys``: the dictionary's keys in class order.  ``on(device)``: the three arrays as device tensors (uploaded once per device,
    without a host synchronisation)."""

    def __init__(self, class_of, class_ptr, members, keys):
        self.class_of = np.ascontiguousarray(class_of, dtype=np.int32)
        self.class_ptr = np.ascontiguousarray(class_ptr, dtype=np.int32)
        self.members = np.ascontiguousarray(members, dtype=np.int32)
        self.keys = list(keys)
        self.n_graphs, self.n_classes = int(self.class_of.size), int(self.class_ptr.size) - 1
        self._dev = {}

    def on(self, device):
        device = torch.device(device)
        if device not in self._dev:
            from .two_stage import _upload
            # (members is never empty-pointer: an all-empty dictionary still gets one word behind the pointer)
            mem = self.members if self.members.size else np.zeros(1, dtype=np.int32)
            self._dev[device] = tuple(_upload(a, device) for a in (self.class_of, self.class_ptr, mem))
        return self._dev[device]


def class_index(classes, graphs):
    """``classes``: a ``{class: [graph objects]}`` dictionary (what the dense-family samplers hold as ``.graphs``, what the SAGPool
    sampler builds from ``data.y``); ``graphs``: the dataset the schedule's indices point into.  Every listed object is looked up in
    ``graphs`` by identity, as ``triplet_stream.schedule_of`` does.  -> ``ClassIndex``.

    Call it AFTER ``schedule_of`` has drained the sampler: ``shuffle()`` reorders the lists in place, and the mined choice depends
    on the list order (the first qualifying candidate; the earliest among equals).

    ValueError, naming the object, for one that is not in ``graphs`` and for a graph listed in two classes (or twice in one); and
    for fewer than two classes.  A class whose list is empty is allowed: it can never be a negative class (``class_of`` comes from the
    lists, so no schedule entry can name it)."""
    keys = list(classes.keys())
    if len(keys) < 2:
        raise ValueError("class_index: mining needs at least two classes; got %d" % len(keys))
    where = {id(g): i for i, g in enumerate(graphs)}
    class_of = np.full(len(where), -1, dtype=np.int32)
    ptr, members = [0], []
    for c, k in enumerate(keys):
        for pos, g in enumerate(classes[k]):
            i = where.get(id(g))
            if i is None:
                raise ValueError("class_index: class %r, position %d: %r is not in `graphs`" % (k, pos, g))
            if class_of[i] >= 0:
                raise ValueError("class_index: graph %d (%r) is listed in class %r and again in class %r"
                                 % (i, g, keys[int(class_of[i])], k))
            class_of[i] = c
            members.append(i)
        ptr.append(len(members))
    return ClassIndex(class_of, np.asarray(ptr), np.asarray(members, dtype=np.int32), keys)


def _pairs_d2(A, C):
    """[n, E] x [m, E] -> [n, m] squared distances in difference form"""
    return ((A[:, None, :] - C[None, :, :]) ** 2).sum(-1)


def mine_negatives_torch(emb, schedule, index, hardness, block=256):
    """the kernel's semantics as a torch composition, for CPU tensors and for shapes ``tsgnn_mine_supported`` refuses: difference-
    form distances, and the list-order / first-wins rules spelled out through list positions (``torch.argmin``'s choice among equals
    is not the reference's).  -> the mined negatives, int32 [T] on ``schedule``'s device; ``schedule`` is not written.  Indices are
    clamped into their tables, as the kernel clamps them."""
    mode = mode_of(hardness)
    dev = schedule.device
    s = schedule.long()
    if mode == 0:
        return s[:, 2].int()
    G = index.n_graphs
    class_of = torch.as_tensor(index.class_of, device=dev).long()
    members = torch.as_tensor(index.members, device=dev).long().clamp(0, G - 1)
    X = emb.to(dev).float()
    a, p, n = (s[:, k].clamp(0, G - 1) for k in range(3))
    cls = class_of[n].clamp(0, index.n_classes - 1)
    out = n.clone()
    total = int(index.class_ptr[-1])
    for c in range(index.n_classes):
        lo = min(max(int(index.class_ptr[c]), 0), total)
        hi = min(max(int(index.class_ptr[c + 1]), lo), total)
        sel = torch.nonzero(cls == c).reshape(-1)
        if hi == lo or sel.numel() == 0:
            continue
        cand = members[lo:hi]
        C = X[cand]
        place = torch.arange(hi - lo, device=dev)
        none = hi - lo
        for i in range(0, sel.numel(), block):
            e = sel[i:i + block]
            A = X[a[e]]
            D = _pairs_d2(A, C)
            if mode == HARDEST:
                qual = D < ((A - X[n[e]]) ** 2).sum(-1)[:, None]                  # strictly closer than the drawn negative
                Dq = torch.where(qual, D, torch.full_like(D, float("inf")))
                first = torch.where(qual & (Dq == Dq.min(1, keepdim=True).values), place, none).min(1).values
            else:
                qual = D < ((A - X[p[e]]) ** 2).sum(-1)[:, None]
                first = torch.where(qual, place, none).min(1).values
            hit = first < none
            out[e] = torch.where(hit, cand[first.clamp(max=none - 1)], out[e])
    return out.int()


def kernel_ok(emb, index):
    """does ``tsgnn_mine_negatives_f32`` take these embeddings?  (device rows of at most 1024 columns)"""
    return bool(emb.is_cuda and nat.lib().tsgnn_mine_supported(int(emb.size(1)), index.n_classes))


def _check(emb, schedule, index):
    if emb.dim() != 2 or emb.size(0) < index.n_graphs or emb.size(1) < 1:
        raise ValueError("emb must be [>= %d graphs, E >= 1]; got %s" % (index.n_graphs, tuple(emb.shape)))
    if schedule.dim() != 2 or schedule.size(1) != 3 or schedule.size(0) < 1 or schedule.dtype != torch.int32 \
            or not schedule.is_contiguous():
        raise ValueError("a schedule is a contiguous int32 tensor [T, 3] with T >= 1; got %s %s" % (schedule.dtype, tuple(schedule.shape)))
    if schedule.device != emb.device:
        raise ValueError("emb and schedule must live on one device; got %s and %s" % (emb.device, schedule.device))


def mine_negatives(emb, schedule, index, hardness, n_changed=None):
    """rewrite column 2 of ``schedule`` (int32 [T, 3] view, device) IN PLACE with the mined negatives; columns 0 and 1 stay.
    ``emb``: [G, E] float32 device tensor (``two_stage.embed_dataset``'s output; made kernel-ready through ``two_stage._rows16``);
    ``index``: ``class_index``'s result; ``hardness``: 0 nothing, 0.5 semi-hard, any other positive value hardest.  ``n_changed``
    (optional): an int32 device tensor of one element that the number of entries whose negative changed is ADDED to.

    One launch enqueued on the current stream: no synchronisation, no device-to-host copy (the class tables go up once per
    ``index`` and device, pinned and non-blocking).  CPU tensors, and embeddings wider than ``tsgnn_mine_supported`` takes, go
    through ``mine_negatives_torch``.  -> ``schedule``"""
    mode = mode_of(hardness)
    _check(emb, schedule, index)
    if mode == 0:
        return schedule
    if not kernel_ok(emb, index):
        mined = mine_negatives_torch(emb, schedule, index, hardness)
        if n_changed is not None:
            n_changed += (mined != schedule[:, 2]).sum().to(n_changed.dtype)
        schedule[:, 2] = mined
        return schedule
    from .two_stage import _rows16
    if n_changed is not None and (n_changed.dtype != torch.int32 or n_changed.numel() != 1 or n_changed.device != emb.device):
        raise ValueError("n_changed is an int32 tensor of one element on the embeddings' device")
    x = _rows16(emb.detach())
    class_of, class_ptr, members = index.on(emb.device)
    nat.call("mine_negatives_f32", x, x.stride(0), index.n_graphs, x.size(1), class_of, class_ptr, members, index.n_classes, schedule,
             schedule.size(0), mode, n_changed)
    return schedule
