"""The datasets, models, schedules and the numpy restatement the GAT mini-batch stream's tests share (tests/test_gat_minibatch_host.py,
tests/test_gpu_gat_minibatch.py).  TEST INFRASTRUCTURE: no project kernel.

Datasets (graph objects as ``gat_triplet.pack_host`` reads them, each with a label in [0, 3)):
  mb3 / mb8   160 graphs at Nmax 12, n cycling 1 .. 12 (n = 1; n = Nmax: no ghost representative) over the kinds of
              ``gat_stream_util.ASM_GRAPHS`` (directed, symmetric and edge-less graphs; 11 kinds against 12 sizes, so the first 132
              graphs hold every pair), fin 3 (ldf 4) and fin 8 (ldf 8)
  big         ``gat_stream_util``'s four graphs at Nmax 320, n = 40, 130, 250, 320, whose ``x`` (and, for the largest, whose entry arrays)
              span several 2,048-word chunks of the gather launch
Schedules (``schedule(name, B)``): entry 0 names B distinct graphs, entry 1 B small graphs (what the previous gather left must be
inert), entry 2 is drawn with repetition, entry 3 is entry 0 reversed.
Model: ``DGATEncoderGraph(final_dim='number_classes')``, hidden 8, embedding 8, 3 classes, 2 layers x heads [2, 2].

``launch_np`` restates ``tsgnn_gat_batch_gather_f32``: EVERY word of every array at capacity, the words the launch leaves alone
included (they keep the caller's fill pattern)."""
import numpy as np
import torch

import gat_stream_util as U
import test_gat_triplet_host as H

NMAX = U.NMAX_SMALL
N_GRAPHS = 160
N_CLASSES = 3
FIN = {"mb3": 3, "mb8": 8, "big": 8}
HEADS = [2, 2]
BIG_SCHEDULES = {3: np.array([[3, 2, 1], [0, 0, 1], [1, 3, 0], [0, 2, 0]], dtype=np.int64),
                 5: np.array([[3, 2, 1, 0, 2], [0, 0, 1, 0, 0], [1, 3, 0, 2, 3]], dtype=np.int64)}
INT_NAMES = ["rowptr", "rowptr_t", "col", "col_t", "src_e_t", "inv", "graph_ptr", "row_graph", "row_slot", "iso_idx", "iso_ptr"]

_DATA = {}


def dataset(name):
    """-> the labelled graph objects (built once per process; treat as read-only)"""
    if name not in _DATA:
        if name == "big":
            _DATA[name] = U.dataset("big")                      # (labels b % 2)
        else:
            kinds = [k for _, k in U.ASM_GRAPHS]
            objs = []
            for i in range(N_GRAPHS):
                o = H.make_obj(700 + i, i % NMAX + 1, nmax=NMAX, fin=FIN[name], kind=kinds[i % len(kinds)])
                o.graph["label"] = (i * 7 + i // 5) % N_CLASSES
                objs.append(o)
            _DATA[name] = objs
    return _DATA[name]


def labels(name):
    return np.array([int(o.graph["label"]) for o in dataset(name)], dtype=np.int32)


def model(name, mode="eval", dev="cuda", dropouts=None, final_dim="number_classes"):
    """the seeded encoder of a dataset: equal parameters at every call"""
    from two_stage_gnn_amd import gat_encoders as G
    torch.manual_seed(23)
    m = G.DGATEncoderGraph(FIN[name], 8, 8, N_CLASSES, None, num_layers=2, num_heads=list(HEADS), neg_input_slopes=[0.2, 0.2],
                           dropouts=dropouts or [0.0, 0.0], final_dim=final_dim)
    return m.to(dev).train(mode == "train")


def schedule(name, B):
    if name == "big":
        return BIG_SCHEDULES[B]
    rng = np.random.default_rng(1000 + B)
    first = rng.permutation(N_GRAPHS)[:B]
    order = rng.permutation(N_GRAPHS)
    small = order[np.argsort(order % NMAX, kind="stable")][:B]  # the B graphs of the fewest nodes (distinct: they fit the default capacity)
    return np.stack([first, small, rng.integers(0, N_GRAPHS, B), first[::-1]]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the restatement
def _a4(v):
    return (int(v) + 3) // 4 * 4


def pieces(objs):
    """(records int64 [G, 8], per graph a dict of the piece's nine sections) from ``gat_stream_util.restate``'s buffers and a layout
    written out here: nine sections, each rounded up to 4 words"""
    rec, bufs = U.restate(objs)
    out = []
    for r, buf in zip(rec, bufs):
        nr, nnz, k = int(r[2]), int(r[3]), int(r[4])
        ldf = (buf.size - 2 * _a4(nr + 1) - 4 * _a4(nnz) - 2 * _a4(k)) // max(nr, 1)
        lens = [nr + 1, nr + 1, nnz, nnz, nnz, nnz, k, k, nr * ldf]
        names = ["rowptr", "rowptr_t", "col", "col_t", "src_e_t", "inv", "iso_rows", "iso_w", "x"]
        o, p = 0, {"ldf": ldf}
        for nm, ln in zip(names, lens):
            p[nm] = buf[o:o + ln]
            o += _a4(ln)
        assert o == buf.size
        out.append(p)
    return rec, out


def sizes_of(row_cap, nnz_cap, iso_cap, B, ldf, heads):
    """the arrays' lengths as ``GatArenaStream._allocate`` lays them out -> (isz, fsz, float names)"""
    E, I = max(nnz_cap, 1), max(iso_cap, 1)
    isz = [row_cap + 1, row_cap + 1, E, E, E, E, B + 1, row_cap, row_cap, I, B + 1]
    fsz = [row_cap, I, row_cap * ldf] + [row_cap * h for h in heads]
    return isz, fsz, ["row_mult", "iso_w", "x"] + ["iso_cols%d" % h for h in heads]


def launch_np(rec, per, labels_, ids, row_cap, nnz_cap, iso_cap, ldf, heads, ifill=-1, ffill=0x7FC0BEEF):
    """one launch of ``tsgnn_gat_batch_gather_f32`` on entry ``ids`` -> {array: int32 bit view at capacity, 'ids' int32 [B], 'label'
    int64 [B]}; words the launch does not write hold ``ifill`` (integer arrays) / ``ffill`` (float arrays, as bits).  An entry that does
    not fit writes nothing at all"""
    B = len(ids)
    isz, fsz, fnames = sizes_of(row_cap, nnz_cap, iso_cap, B, ldf, heads)
    out = {nm: np.full(n, ifill, dtype=np.int32) for nm, n in zip(INT_NAMES, isz)}
    out.update({nm: np.full(n, ffill, dtype=np.int64).astype(np.uint32).view(np.int32) for nm, n in zip(fnames, fsz)})
    out["ids"] = np.full(B, ifill, dtype=np.int32)
    out["label"] = np.full(B, ifill, dtype=np.int64)
    nr = rec[ids, 2]
    nnz = rec[ids, 3]
    ks = rec[ids, 4]
    row0, e0, i0 = (np.concatenate([[0], np.cumsum(v)]) for v in (nr, nnz, ks))
    R, E, I = int(row0[-1]), int(e0[-1]), int(i0[-1])
    if R > row_cap or E > nnz_cap or I > iso_cap:
        return out
    f32 = lambda a: np.asarray(a, dtype=np.float32).view(np.int32)
    x = out["x"].reshape(row_cap, ldf)
    for y, g in enumerate(ids):
        p, n, mult = per[g], int(rec[g, 1]), int(rec[g, 5])
        a, b, e, i = int(row0[y]), int(row0[y + 1]), int(e0[y]), int(i0[y])
        last = y == B - 1
        out["rowptr"][a:b + last] = p["rowptr"][:b - a + last] + e
        out["rowptr_t"][a:b + last] = p["rowptr_t"][:b - a + last] + e
        out["col"][e:e + nnz[y]] = p["col"] + a
        out["col_t"][e:e + nnz[y]] = p["col_t"] + a
        out["src_e_t"][e:e + nnz[y]] = p["src_e_t"] + e
        out["inv"][e:e + nnz[y]] = p["inv"] + e
        x[a:b] = p["x"].reshape(b - a, ldf)
        m = np.where(np.arange(b - a) < n, 1.0, float(mult)).astype(np.float32)
        out["row_mult"][a:b] = f32(m)
        out["row_graph"][a:b] = y
        out["row_slot"][a:b] = np.arange(b - a)
        w = np.where(np.diff(p["rowptr_t"]) == 0, m, np.float32(0.0)).astype(np.float32)
        for h in heads:
            out["iso_cols%d" % h].reshape(row_cap, h)[a:b] = f32(w)[:, None]
        out["graph_ptr"][y], out["iso_ptr"][y] = a, i
        out["iso_idx"][i:i + ks[y]] = p["iso_rows"] + a
        out["iso_w"][i:i + ks[y]] = p["iso_w"]
        out["ids"][y] = g
        out["label"][y] = labels_[g]
    out["graph_ptr"][B], out["iso_ptr"][B] = R, I
    out["rowptr"][R + 1:] = E                                  # the padding: empty rows both ways, +0 everywhere, the last graph
    out["rowptr_t"][R + 1:] = E
    out["row_mult"][R:] = 0
    out["row_graph"][R:] = B - 1
    out["row_slot"][R:] = 0
    x[R:] = 0
    for h in heads:
        out["iso_cols%d" % h][R * h:] = 0
    return out
