"""The GraphSage-style conv stack of GcnEncoderGraph (encoders.py:177-217) as ONE autograd node with a minimal launch
sequence (the b = 32 shape is bound by launch boundaries and per-kernel latency chains).

  forward, layer 0   : gather_rowgemm (aggregate + .W + bias + L2 normalise; z kept for dW)  -> slot_bn_fwd (ReLU + slot BN)
  forward, layer l>0 : sage_layer_fwd (the same product || max-readout partial of the layer's input)  [-> slot_bn_fwd]
  forward, tail      : readout_head_fwd (last layer's readout from its rows + decode of the others + both nn.Linear), or
                       readout_partial + readout_decode_layers when the head is not part of the node
  backward           : [head2_bwd ->] per layer slot_post_bwd (readout scatter + BN + ReLU + normalise backward -> dU), then
                       sage_layer_bwd (dW/db slabs || dX = (A dU) W^T) for hidden layers / linear_wgrad slabs for layer 0,
                       ONE slab reduction for all layers (straight into the trainer's flat gradient bucket when installed)

The node's forward and backward are drivers over these stages (DESIGN.md has the map from stage to launch group):

  forward  : _Fwd (set-up) -> _fused_bn_workspace ? _forward_fused_bn : _forward_layers (_layer_product, _layer_post) -> _forward_tail
  backward : _head_backward -> per layer _layer_du, then _spend_du (merged launch, else slabs and the dX product) -> one WgradSets.close()

Ghost rows: they aggregate nothing, so the products skip them and a filler block writes their constant output;
only the ghost slots up to the largest graph can influence anything, so the slot kernels run on those.

Used when the batch qualifies (slot-BN on, sum aggregation without self term, <= 128 graphs, widths <= 128); any other
configuration runs the operator-by-operator path in dense_encoders.py: same results, more launches.  Every fusion has a switch
(environment / module attribute) that selects the launch sequence it replaces.
"""
import contextlib
import os
from collections import namedtuple

import numpy as np
import torch

from . import _native as nat
from . import message_passing as mp


def eligible(g, convs, bn, x):
    """may this stack run as the fused node?  (the whole answer: shapes, layout, and the library's word on the slot kernels)"""
    if not bn or g.B > 128 or len(convs) < 2:
        return False
    hid = convs[0].output_dim
    for i, c in enumerate(convs):
        if c.add_self or not c.normalize_embedding or c.dropout > 0.001:
            return False
        if c.output_dim % 4 or c.output_dim > 128:
            return False
        if i < len(convs) - 1 and c.output_dim != hid:
            return False
    if not (x.dim() == 2 and x.size(1) % 4 == 0 and x.is_cuda and x.stride(0) % 4 == 0):
        return False
    # (host-only query: the slot kernels take B graphs at the first and the last layer's width)
    return all(bool(nat.lib().tsgnn_slot_fused_supported(g.B, c.output_dim)) for c in (convs[0], convs[-1]))


def _aggregate_raw(g, x, transposed=False, rows=None):
    """rows: produce only the first `rows` output rows (ghost rows aggregate nothing and, on the fused path, nobody reads
    their aggregate: the products leave them out)."""
    n = g.total_rows if rows is None else rows
    if g.val is None and mp.ell_ok(x) and g.total_rows <= mp.ELL_MAX_ROWS and (not transposed or g.symmetric):
        return mp.spmm_ell(g, x, rows=n)
    rp, col, val = g.transposed() if transposed else (g.rowptr, g.col, g.val)
    return mp.spmm_raw(rp, col, val, x, n)


FUSED_TAIL = os.environ.get("TSGNN_FUSED_TAIL", "1") != "0"        # last readout + decode + the two Linear layers in one launch
MERGED_FWD = os.environ.get("TSGNN_MERGED_FWD", "1") != "0"        # a layer's product + the readout partial of its input in one launch
MERGED_BWD = os.environ.get("TSGNN_MERGED_BWD", "1") != "0"        # weight-gradient slabs + input-gradient product in one launch
GATHER_MAX_ROWS = int(os.environ.get("TSGNN_GATHER_MAX_ROWS", 65536))   # above: stand-alone row-batched aggregation + lean product
GATHER_FUSED = os.environ.get("TSGNN_GATHER_FUSED", "1") != "0"     # aggregate inside the `.W` product when the neighbour table has no CSR tail
EPILOGUE_READOUT = os.environ.get("TSGNN_EPILOGUE_READOUT", "1") != "0"   # the last layer's max readout in its product's epilogue
LAST_LAYER_ROWS = os.environ.get("TSGNN_LAST_LAYER_ROWS", "1") != "0"     # the last layer's dU from a row-parallel kernel
RO_MAP = os.environ.get("TSGNN_RO_MAP", "1") != "0"                       # readout blocks placed on the XCD that holds their graph's rows
FUSED_BN = os.environ.get("TSGNN_FUSED_BN", "1") != "0"                   # slot batch-norm without launches of its own (statistics in the
                                                                          # producing product's epilogue, normalisation in the consumers)
# layer 0: dU and its weight-gradient slabs in ONE launch, dU kept in LDS (tsgnn_slot_post_wgrad_f32).  Correct (tests run it) and one
# launch less, but measured SLOWER than the two launches it replaces (DD b32: 12.7 us at one slot per workgroup + 10.7 us for the
# reduction of 399 slabs, 15.3 + 5.1 at two slots, against 6.7 + 7.8 + 4.2): a slot is a full latency chain, and the slabs are per
# workgroup.  Off by default.
SLOT_WGRAD = os.environ.get("TSGNN_SLOT_WGRAD", "0") != "0"
HEAD_DU = os.environ.get("TSGNN_HEAD_DU", "1") != "0"                     # ... computed by extra workgroups of the head's backward launch


# the fused layer launches gather their row panels from the batch's packed neighbour schedule (every neighbour row asked for in ONE round
# trip, GraphBatch.gather_schedule) instead of the fixed-width table (neighbours 9-16 in a second dependent phase)
GATHER_SCHED = os.environ.get("TSGNN_GATHER_SCHED", "1") != "0"
GATHER_SCHED_L0 = os.environ.get("TSGNN_GATHER_SCHED_L0", "1") != "0"    # ... layer 0's launch too (0: only the hidden layers' four)
# layer 0's launch takes its weight operands straight from W (no LDS stage; csrc/rowgemm_body.h BDIR).  0: W staged through LDS
# (tsgnn_gather_rowgemm_st_mode_f32 at b_mode = 1): the same result bit for bit, for A/B measurements and the tests
L0_DIRECT_B = os.environ.get("TSGNN_L0_DIRECT_B", "1") != "0"
DU_MAP = os.environ.get("TSGNN_DU_MAP", "1") != "0"             # exact batches: the head backward's dU workgroups listed by the host
SLABS_BESIDE = os.environ.get("TSGNN_SLABS_BESIDE", "1") != "0"
NSLAB_MAX = int(os.environ.get("TSGNN_NSLAB_MAX", "0"))
_ncu = {}


def _cu_count(dev):
    if dev not in _ncu:
        _ncu[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return _ncu[dev]


def _slabs_beside_panels(nslab, rps, need, rows, K, N, dev, panel_units):
    """The merged backward launch hosts two slab blocks per slab AND one block per 32-row panel; a CU keeps two of these blocks
    (registers).  The plan sizes the slabs to one block per CU, which is right while the panels fit the CUs too; with more
    panels than CUs the launch would need a THIRD block on some CUs, which waits for a free slot (DD seed 6, 288 panels:
    13.7 -> 18.2 us).  Fewer, longer slabs keep the launch at two blocks per CU."""
    if not SLABS_BESIDE or nslab <= 0:
        return nslab, rps, need
    if NSLAB_MAX and nslab > NSLAB_MAX:                         # (experiment knob: fewer, longer slabs)
        rps = (-(-rows // NSLAB_MAX) + 7) // 8 * 8
        nslab = -(-rows // rps)
        need = nslab * (K + 1) * N
    ncu = _cu_count(dev)
    npan = int(nat.lib().tsgnn_panel_blocks(int(rows), int(panel_units)))   # (32-row panels, or units for the rows beyond one panel per CU)
    if npan <= ncu or 2 * nslab + npan <= 2 * ncu:
        return nslab, rps, need
    cap = max(32, (2 * ncu - npan) // 2)
    rps = -(-rows // cap)
    rps = (rps + 7) // 8 * 8
    nslab = -(-rows // rps)
    return nslab, rps, nslab * (K + 1) * N


def _gather_ok(g, x):
    return bool(GATHER_FUSED and g.val is None and mp.ell_ok(x) and g.total_rows <= GATHER_MAX_ROWS)


def _gather_sched(g, slots=False, layer0_k=0, fill=0):
    """(schedule, ell_w code) for a fused layer launch on g, or (None, 0): the launch takes the neighbour table.  layer0_k: the launch
    is tsgnn_gather_rowgemm_st_f32 at this K (fill = its fill_rows); else a hidden layer's forward (slots: ids carry the slot) /
    backward launch.  The library names the kernel's shape, the batch packs (and caches) the schedule for it."""
    if not GATHER_SCHED:
        return None, 0
    code = int(nat.lib().tsgnn_gather_sched_slots(int(g.n_rows), int(fill), int(layer0_k), int(g.panel_units), 1 if layer0_k else 0))
    if not code:
        return None, 0
    sched = g.gather_schedule((16, 24) if code == 24 else (8, 32), slots=slots)
    return (sched, code) if sched is not None else (None, 0)


# Per-graph statistics (B = 1 semantics: the 2stg triplet step runs anchor / positive / negative as one batch in which every graph
# keeps the batch-norm statistics it would have alone, tripletnet.py:36-38): the slot batch-norm degenerates to a per-row layer norm,
# so the two slot launches of a hidden layer are replaced by their row-local counterparts (tsgnn_row_ln_fwd_f32 forward,
# tsgnn_row_post_bwd_f32 backward) and everything else of the stack — aggregation inside the products, the readout partials riding
# in the next layer's launch, merged weight-gradient / input-gradient launches, one reduction for all layers — stays.  The node-feature
# form (`nodes`) runs the same way: the normalised rows go straight into the layer's column block, and the backward is
# tsgnn_row_post_nodes_bwd_f32 (the block's own gradient in place of the readout pair).  Selected by
# the caller around the node's forward (`with per_graph_stats(True):`); the statistics without launches of their own (FUSED_BN)
# are per slot across graphs and are not used in this mode.
_PER_GRAPH = [False]
_IMG_FLOATS = 16384        # one fragment-major weight image (tsgnn_sage_conv_pack_f32): [4 waves][16 steps][64 lanes] float4
_IMG_LAYERS = 4            # hidden layers whose two images one launch's pack riders write (8 images)
_Saved = namedtuple("_Saved", "z v rinv mean rstd lean")      # what a layer leaves for the backward (lean: z has the real rows only)


@contextlib.contextmanager
def per_graph_stats(on=True):
    prev, _PER_GRAPH[0] = _PER_GRAPH[0], bool(on)
    try:
        yield
    finally:
        _PER_GRAPH[0] = prev


def _neighbours(g, sched=None, width=0, table=None):
    """(table, width, tail_ptr, tail_col): the neighbour operands of a gather launch on g.  sched / width: a packed schedule
    (_gather_sched) goes in the table's place, without a tail; table: (table, tail_col) of g.ell_slots() in place of the plain ids."""
    ell, ell_w, tail = g.ell()
    if sched is not None:
        return sched, width, None, None
    tp, tc = tail if tail is not None else (None, None)
    return (ell, ell_w, tp, tc) if table is None else (table[0], ell_w, tp, table[1])


class _Fwd:
    """one forward's set-up (operands, ghost slots, output buffers) and the state its layers hand on: pending_ro = (y, packed
    segment) of a readout that rides in the next layer's launch, off = the layer's offset in `packed`, last_ro_done"""

    def __init__(s, x0, g, has_bias, nodes, params):
        s.g, s.nodes, L = g, nodes, len(params) // 2
        Ws = s.Ws = [params[2 * l].contiguous() for l in range(L)]
        bs = s.bs = [params[2 * l + 1] if has_bias else None for l in range(L)]
        R, B, dev = g.total_rows, g.B, x0.device
        Fh, Fl = Ws[0].size(1), Ws[-1].size(1)
        s.L, s.Fh, s.Fl, s.dev = L, Fh, Fl, dev
        s.total = B * ((L - 1) * Fh + Fl)
        # cleared by the first slot_bn_fwd launch; Fl spare words behind the last layer's segment take the readout of the dummy
        # graph that the padding rows of a capacity-padded batch (ingest.py) belong to: never cleared, never read
        s.packed = torch.empty(s.total + Fl, dtype=torch.int64, device=dev) if not nodes else None
        s.cat = torch.empty(R, (L - 1) * Fh + Fl, dtype=torch.float32, device=dev) if nodes else None
        x = s.x = mp._check(x0, R)
        # Ghost slots actually needed.  Every graph's padded rows at slots >= the largest graph are bitwise identical in
        # every layer (same bias row, same statistics), the max readout breaks ties towards the smallest row, and nothing
        # aggregates from a ghost row: only slots [0, max_size] can influence an output or a gradient.  The slot kernels,
        # the filler and the bias gradient therefore run on  gs = min(nmax, max_size + 1)  ghost rows (half of nmax on DD).
        # (nodes = 1, the unmasked node output: every ghost row is part of the result)
        gs = g.n_ghost
        if nodes != 1 and g.n_ghost > 0 and x.stride(0) % 4 == 0 and all(
                Ws[l].size(1) % 4 == 0 and Ws[l].data_ptr() % 16 == 0 and (bs[l] is None or bs[l].data_ptr() % 16 == 0) for l in range(L)):
            # (capacity-padded batches keep one shape for every batch: a fixed bound instead of this batch's largest graph)
            fixed = getattr(g, "ghost_slots_fixed", None)
            gs = min(g.nmax, (int(fixed) if fixed is not None else int(g.sizes.max()) + 1))
        s.gs, (s.sn, s.sg) = gs, ((gs, gs) if g.n_ghost else (g.nmax, 0))      # (slots, ghost rows) handed to the slot kernels
        s.keep, s.pending_ro, s.off, s.last_ro_done = [], None, 0, False


def _fused_bn_workspace(s, head, per_graph):
    """the batch's workspace (GraphBatch.bn_workspace, cleared if an earlier forward left it dirty) when the stack runs with slot
    batch-norm inside its products (_forward_fused_bn), else None"""
    g, x, Ws, bs, L, Fh, Fl, sn = s.g, s.x, s.Ws, s.bs, s.L, s.Fh, s.Fl, s.sn
    if not (FUSED_BN and not per_graph and head is not None and not s.nodes and L >= 2 and g.n_ghost == g.nmax and sn == s.sg and sn <= 1024
            and Fh == 128 and Fl == 128 and Ws[0].size(0) <= 128 and x.size(1) % 4 == 0 and MERGED_FWD and EPILOGUE_READOUT
            and _gather_ok(g, x) and all(Ws[l].size(0) == 128 and Ws[l].stride(0) % 4 == 0 for l in range(1, L))
            and all(Ws[l].data_ptr() % 16 == 0 and (bs[l] is None or bs[l].data_ptr() % 16 == 0) for l in range(L))
            and mp.rowgemm_ok(x, x.stride(0), Ws[0], Ws[0].stride(0), Ws[0].size(0), Fh, False)
            and head[0].size(0) <= 128 and (L - 1) * Fh + Fl <= 2048 and g.row_graph is not None) or g.ell_slots() is None:
        return None
    bnf = g.bn_workspace(g.B, L, Fh, Fl, sn)
    if bnf["dirty"]:
        bnf["sums"].zero_(); bnf["ghost"].zero_(); bnf["packed"].zero_()
    bnf["dirty"] = True
    return bnf


def _forward_fused_bn(s, bnf):
    """slot batch-norm without launches of its own (L launches for the conv stack instead of 2L - 1): gather_rowgemm_st, then one
    sage_layer_fwd_bn per hidden / last layer.  -> (saved, w_img, pack_desc)"""
    g, x, Ws, bs, L, Fh, dev, gs, sn, packed = s.g, s.x, s.Ws, s.bs, s.L, s.Fh, s.dev, s.gs, s.sn, s.packed
    R, B, sums, ghost = g.total_rows, g.B, bnf["sums"], bnf["ghost"]
    ro_map, ro_ch = g.readout_map(sn, gs) if RO_MAP else (None, 0)
    # fragment-major images of the hidden layers' weights (forward and input-gradient orientation), written by extra workgroups
    # of layer 0's launch from the parameters THIS call uses: the later launches read W from them instead of staging it through
    # LDS.  One buffer per call, nothing cached: parameters are also rewritten behind autograd's back (restored snapshots).
    w_img = pack_desc = None
    if 1 <= L - 1 <= _IMG_LAYERS:
        w_img = torch.empty(2 * (L - 1), _IMG_FLOATS, dtype=torch.float32, device=dev)
        pack_desc = np.empty(1 + 12 * (L - 1), dtype=np.int64)
        pack_desc[0] = 2 * (L - 1)
        for l in range(1, L):
            for kn in (1, 0):                        # image 2 (l - 1): forward (w[k][n]); 2 (l - 1) + 1: input gradient
                t = 2 * (l - 1) + (1 - kn)
                pack_desc[1 + 6 * t:7 + 6 * t] = (Ws[l].data_ptr(), Ws[l].stride(0), 128, 128, kn, w_img[t].data_ptr())
        bnf["pack_desc"] = pack_desc                 # (recorded launches are replayed by address: the last descriptor stays valid)
    sch0, sch0_w = _gather_sched(g, layer0_k=Ws[0].size(0), fill=gs) if GATHER_SCHED_L0 else (None, 0)
    schs, schs_w = _gather_sched(g, slots=True)
    saved = []
    for l in range(L):
        K, N = Ws[l].size(0), Ws[l].size(1)
        v = torch.empty(R, N, dtype=torch.float32, device=dev)
        rinv = torch.empty(R, dtype=torch.float32, device=dev)
        z = torch.empty(R, x.size(1) if l == 0 else Fh, dtype=torch.float32, device=dev)
        s_out, g_out = (sums[l * 2 * sn:(l + 1) * 2 * sn], ghost[2 * l:2 * l + 2]) if l < L - 1 else (None, None)
        if l == 0:
            a0 = (*_neighbours(g, sch0, sch0_w), x, x.stride(0), Ws[0], Ws[0].stride(0), bs[0], v, v.stride(0), rinv, z, z.stride(0), g.n_rows,
                  K, N, gs, g.row_slot, s_out, g_out, int(g.panel_units), pack_desc.ctypes.data if pack_desc is not None else None)
            name, mode = ("gather_rowgemm_st_f32", ()) if L0_DIRECT_B else ("gather_rowgemm_st_mode_f32", (1,))     # (b_mode 1: W through LDS)
            nat.call(name, *a0, *mode)
        else:
            p, last = saved[l - 1], l == L - 1
            nat.call("sage_layer_fwd_bn_f32", *_neighbours(g, schs, schs_w, table=g.ell_slots()), p.v, p.v.stride(0), Ws[l], Ws[l].stride(0),
                     bs[l], v, v.stride(0), rinv, z, z.stride(0), g.n_rows, K, gs, g.graph_ptr, g.slot_count, B, sn, s.sg,
                     packed[(l - 1) * B * Fh:(l - 1) * B * Fh + B * Fh], packed[l * B * Fh:l * B * Fh + (B + 1) * N] if last else None,
                     g.row_graph, sums[(l - 1) * 2 * sn:l * 2 * sn], ghost[2 * (l - 1):2 * l], p.mean, p.rstd, None if last else g.row_slot,
                     s_out, g_out, ro_map, ro_ch, int(g.panel_units), w_img[2 * (l - 1)] if w_img is not None else None)
        mean = torch.empty(g.nmax, dtype=torch.float32, device=dev) if l < L - 1 else None     # written by the NEXT launch's readout blocks
        rstd = torch.empty(g.nmax, dtype=torch.float32, device=dev) if l < L - 1 else None
        saved.append(_Saved(z, v, rinv, mean, rstd, True))
    s.last_ro_done = True
    return saved, w_img, pack_desc


def _layer_product(s, l, x, v, rinv):
    """layer l's aggregation + `.W` + bias + L2 normalise into (v, rinv), by the first of five launch forms that takes it -> (z, lean)"""
    g, W, b, gs, sn, sg = s.g, s.Ws[l], s.bs[l], s.gs, s.sn, s.sg
    R, B, K, N = g.total_rows, g.B, W.size(0), W.size(1)
    # Ghost rows aggregate nothing (z = 0): their output is the normalised bias, written by a filler block, and
    # their z is neither produced nor read (255 row panels + 1 filler = one block per CU on the DD batch).
    lean = (g.n_ghost > 0 and x.stride(0) % 4 == 0 and N % 4 == 0 and W.data_ptr() % 16 == 0 and (b is None or b.data_ptr() % 16 == 0))
    fused = lean and N <= 128 and _gather_ok(g, x) and mp.rowgemm_ok(x, x.stride(0), W, W.stride(0), K, N, False)
    if fused and MERGED_FWD and s.pending_ro is not None and K == 128 and N == 128 and x.size(1) == 128 and W.stride(0) % 4 == 0:
        # (1) this layer's product and the max-readout partial of its input (the previous layer's output) in one launch
        z = torch.empty(R, x.size(1), dtype=torch.float32, device=s.dev)
        a = (*_neighbours(g), x, x.stride(0), W, W.stride(0), b, v, v.stride(0), rinv, z, z.stride(0), g.n_rows, K, gs, g.graph_ptr, B, sn, sg,
             s.pending_ro[1])
        if EPILOGUE_READOUT and l == s.L - 1 and not s.nodes and l > 0 and (not g.n_ghost or gs > 0):
            # last layer: no slot batch-norm follows, so its own max readout is folded into the product's epilogue
            # (packed was cleared by layer 0's slot_bn_fwd launch): no pass over v for it
            nat.call("sage_layer_fwd_ro_f32", *a, s.packed[s.off:s.off + (B + 1) * N], g.row_graph)
            s.last_ro_done = True
        else:
            nat.call("sage_layer_fwd_f32", *a)
        s.pending_ro = None
        return z, lean
    if s.pending_ro is not None:                        # the input's readout partial rides with nobody: a launch of its own
        y, pk = s.pending_ro
        nat.call("readout_partial_f32", g.graph_ptr, B, sn, g.n_rows, sg, y, y.stride(0), y.size(1), pk)
    s.pending_ro = None
    if fused:
        # (2) aggregation fused into the product: the neighbour rows are summed while the A panel is staged
        nb = _neighbours(g)
        z = torch.empty(R, x.size(1), dtype=torch.float32, device=s.dev)
        nat.call("gather_rowgemm_f32", *nb, x, x.stride(0), W, W.stride(0), 0, b, v, v.stride(0), rinv, z, z.stride(0), g.n_rows, K, N, 1, gs)
        return z, lean
    z = _aggregate_raw(g, x, rows=g.n_rows if lean else None)
    ok = mp.rowgemm_ok(z, z.stride(0), W, W.stride(0), K, N, False)
    if lean and ok:                                     # (3) row-panel product of the real rows + the ghost rows' filler
        nat.call("rowgemm_f32", z, z.stride(0), W, W.stride(0), 0, b, v, v.stride(0), rinv, g.n_rows, K, N, 1, gs)
        return z, True
    if lean:
        z[g.n_rows:].zero_()
    if ok:                                              # (4) row-panel product of every row
        nat.call("rowgemm_f32", z, z.stride(0), W, W.stride(0), 0, b, v, v.stride(0), rinv, R, K, N, 1, 0)
    else:                                               # (5) any shape
        nat.call("linear_l2norm_f32", z, z.stride(0), W, W.stride(0), b, v, v.stride(0), rinv, R, K, N, 1)
    return z, False


def _layer_post(s, l, v, per_graph, head):
    """what follows layer l's product: ReLU + the row layer norm (per-graph statistics) or the slot batch-norm for l < L - 1 — their
    readout rides in the next layer's launch —, the readout partial for the last layer.  -> (mean, rstd, y: the next layer's input)"""
    g, R, B, N, L, Fh, nodes, sn, sg, dev = s.g, s.g.total_rows, s.g.B, v.size(1), s.L, s.Fh, s.nodes, s.sn, s.sg, s.dev
    pk = s.packed[s.off:s.off + B * N] if not nodes else None
    if l == L - 1:
        if head is None and not nodes and not s.last_ro_done:
            nat.call("readout_partial_f32", g.graph_ptr, B, sn, g.n_rows, sg, v, v.stride(0), N, pk)
        return None, None, None
    mean = torch.empty(R if per_graph else g.nmax, dtype=torch.float32, device=dev)      # per ROW / per slot
    rstd = torch.empty(R if per_graph else g.nmax, dtype=torch.float32, device=dev)
    y = torch.empty_like(v) if not nodes else s.cat[:, l * Fh:(l + 1) * Fh]      # (node form: straight into its column block)
    if per_graph:
        if l == 0 and not nodes:
            s.packed[:s.total].zero_()                    # (what the first slot_bn_fwd launch does on its way)
        nat.call("row_ln_fwd_f32", v, v.stride(0), g.n_rows + sg, N, 1, mean, rstd, y, y.stride(0))
    else:
        nat.call("slot_bn_fwd_f32", g.graph_ptr, g.slot_count, B, sn, g.n_rows, sg, v, v.stride(0), N, 1, mean, rstd, y, y.stride(0),
                 s.packed if (l == 0 and not nodes) else None, s.total)
    if not nodes:
        s.pending_ro = (y, pk)                    # rides along with the next layer's product (or is flushed before it)
    s.keep.append(y)
    return mean, rstd, y


def _forward_layers(s, head, per_graph):
    """the generic route: per layer one product launch (_layer_product) and its post step (_layer_post).  -> saved"""
    g, L, x, saved = s.g, s.L, s.x, []
    for l in range(L):
        N = s.Ws[l].size(1)
        # (node form: the last layer's output IS its block of the concatenation)
        v = s.cat[:, (L - 1) * s.Fh:] if (s.nodes and l == L - 1) else torch.empty(g.total_rows, N, dtype=torch.float32, device=s.dev)
        rinv = torch.empty(g.total_rows, dtype=torch.float32, device=s.dev)
        z, lean = _layer_product(s, l, x, v, rinv)
        mean, rstd, y = _layer_post(s, l, v, per_graph, head)
        saved.append(_Saved(z, v, rinv, mean, rstd, lean))
        s.off += g.B * N
        x = y
    return saved


def _forward_tail(s, head, bnf, saved):
    """the node's result: the node features, or readout_decode_layers, or the decode + both nn.Linear in one of three head launches.
    -> (result, arg, ctx.head)"""
    g, B, L, Fh, Fl, dev, packed, sn, sg = s.g, s.g.B, s.L, s.Fh, s.Fl, s.dev, s.packed, s.sn, s.sg
    if s.nodes:
        if s.nodes == 2 and g.n_ghost:
            nat.defer_zero(s.cat[g.n_rows:])               # embedding mask: ghost rows of the node output are zero
        return s.cat, None, None
    out = torch.empty(B, (L - 1) * Fh + Fl, dtype=torch.float32, device=dev)
    arg = torch.empty(s.total, dtype=torch.int32, device=dev)
    if head is None:
        nat.call("readout_decode_layers_f32", packed, B, L, Fh, Fl, out, out.stride(0), arg)
        return out, arg, None
    # last layer's readout (straight from its rows) + decode of the earlier layers + both Linear layers: one launch
    w1, b1, w2, b2 = head
    w1c, w2c = w1.contiguous(), w2.contiguous()
    E, C = w1c.size(0), w2c.size(0)
    vec = torch.empty(B, E, dtype=torch.float32, device=dev)
    y = torch.empty(B, C, dtype=torch.float32, device=dev)
    if bnf is not None:
        # decode + both Linear layers + the step's housekeeping (packed and the integer sums zeroed for the next step)
        nat.call("packed_head_fwd_z_f32", packed, B, L, Fh, Fl, out, out.stride(0), arg, w1c, b1, w2c, b2, E, C, vec, y, bnf["sums"],
                 (L - 1) * 2 * sn)
        bnf["dirty"] = False
    elif s.last_ro_done and E <= 128 and out.size(1) <= 2048:
        # every layer's maxima are in `packed`: decode + both Linear layers, one memory round trip per block
        nat.call("packed_head_fwd_f32", packed, B, L, Fh, Fl, out, out.stride(0), arg, w1c, b1, w2c, b2, E, C, vec, y)
    else:
        nat.call("readout_head_fwd_f32", packed, B, L, Fh, Fl, saved[-1].v, saved[-1].v.stride(0), g.graph_ptr, g.n_rows, sn, sg, out,
                 out.stride(0), arg, w1c, b1, w2c, b2, E, C, vec, y)
    return (vec, y), arg, (out, vec, w1c, w2c, head)


def _head_backward(ctx, gouts, keep):
    """the head's backward launch; the last layer's dU rides in it where it can (head2_bwd_du_map).
    -> (dout, du_last or None, head_grads), or None: no gradient arrived"""
    g, L, (Fh, Fl), (dvec, dy), (sn, sg) = ctx.g, ctx.L, ctx.dims, gouts, ctx.slots
    out, vec, w1c, w2c, (pw1, pb1, pw2, pb2) = ctx.head
    R, B, dev, last = g.total_rows, g.B, out.device, ctx.saved[L - 1]
    P, E, C = out.size(1), w1c.size(0), w2c.size(0)
    if dy is None and dvec is None:
        return None
    ce = mp.take_deferred_ce(dy) if dy is not None else None      # deferred cross-entropy: this backward rebuilds dy
    if ce is None:
        dy = dy.contiguous() if dy is not None else torch.zeros(B, C, device=dev)
    dvec = dvec.contiguous() if dvec is not None else None
    dout = torch.empty(B, P, dtype=torch.float32, device=dev)
    dw1, s1 = mp._sink_or_new(pw1, (E, P), dev)
    dw2, s2 = mp._sink_or_new(pw2, (C, E), dev)
    db1, s3 = mp._sink_or_new(pb1, (E,), dev) if pb1 is not None else (None, False)
    db2, s4 = mp._sink_or_new(pb2, (C,), dev) if pb2 is not None else (None, False)
    parts = mp.head_norm_slots((s1, s2, s3, s4), (pb1 is not None, pb2 is not None), (pw1, pb1, pw2, pb2), E)
    keep.append((ce, dy, dvec, dw1, dw2, db1, db2, parts))
    du_last = None
    if (HEAD_DU and LAST_LAYER_ROWS and not ctx.nodes and L > 1 and last.lean and Fl % 4 == 0 and Fl <= 128 and g.n_ghost == g.nmax
            and sn == sg and g.n_ghost >= B and ctx.needs_input_grad[5 + 2 * (L - 1)] and last.v.stride(0) % 4 == 0):
        # the last layer's dU (a row-wise function of the readout gradient: it has no batch-norm) rides in this launch
        du_l = torch.empty(R, Fl, dtype=torch.float32, device=dev)
        keep.append(du_l)
        argl = ctx.arg[(L - 1) * B * Fh:(L - 1) * B * Fh + B * Fl]
        # (the non-empty (graph, chunk) pairs listed by the host for an exact batch: no workgroup that only returns)
        dmap, ndmap, dchunk = g.du_map(B + (E + 3) // 4 + 1) if DU_MAP else (None, 0, 64)
        if nat.try_call("head2_bwd_du_map_f32", out, out.stride(0), vec, ce[0] if ce is not None else None,
                        ce[1] if ce is not None else None, ce[2] if ce is not None else None, None if ce is not None else dy, dvec,
                        w1c, w2c, B, P, E, C, dout, dout.stride(0), dw1, db1, dw2, db2, parts, g.graph_ptr, g.n_rows, sg, sn,
                        last.v, last.v.stride(0), last.rinv, argl, (L - 1) * Fh, Fl, du_l, du_l.stride(0), dmap, ndmap, dchunk):
            du_last = du_l
    if du_last is None and ce is not None:
        nat.call("head2_bwd_ce_f32", out, out.stride(0), vec, ce[0], ce[1], ce[2], dvec, w1c, w2c, B, P, E, C, dout, dout.stride(0),
                 dw1, db1, dw2, db2, parts)
    elif du_last is None:
        nat.call("head2_bwd_f32", out, out.stride(0), vec, dy, dvec, w1c, w2c, B, P, E, C, dout, dout.stride(0), dw1, db1, dw2, db2, parts)
    if mp.GRAD_SINK is not None and s1 and s2 and (s3 or pb1 is None) and (s4 or pb2 is None):
        mp.GRAD_SINK.ready((pw1, pb1, pw2, pb2))       # final already: their all-reduce may overlap the conv backward
    return dout, du_last, (None if s1 else dw1, None if s3 else db1, None if s2 else dw2, None if s4 else db2)


def _layer_du(ctx, l, dout, dxs, du_last, red, grads, keep):
    """layer l's dU = gradient of its product's output, from the readout (or node-block) gradient `dout` and the next layer's input
    gradient `dxs`, by one of five launch forms.  -> (du, bo: rows behind the real ones that feed the bias gradient only), or
    (None, 0) where the launch took the layer's weight gradient along (slot_post_wgrad: nothing is left to spend)"""
    g, L, nodes, Fh, (sn, sg), dev = ctx.g, ctx.L, ctx.nodes, ctx.dims[0], ctx.slots, dout.device
    z, v, rinv, mean, rstd, lean = ctx.saved[l]
    R, B, K, N = g.total_rows, g.B, ctx.Ws[l].size(0), ctx.Ws[l].size(1)
    last = l == L - 1
    if last and du_last is not None:
        return du_last, B                         # B ghost CONTRIBUTION rows stand for the sg ghost rows (tsgnn_head2_bwd_du_f32)
    du = torch.empty(R, N, dtype=torch.float32, device=dev)
    dsl = dout[:, l * Fh:l * Fh + N] if not nodes else None      # this layer's readout gradient and its winners' rows ...
    argl = ctx.arg[l * B * Fh:l * B * Fh + B * N] if not nodes else None
    dnode = dout[:, l * Fh:l * Fh + N] if nodes else None        # ... or the gradient of this layer's block of the node output
    lddxs, post = dxs.stride(0) if dxs is not None else 0, 0 if last else 1      # (post: ReLU and batch-norm follow the layer)
    if (LAST_LAYER_ROWS and last and not nodes and dxs is None and N % 4 == 0 and N <= 128 and g.n_ghost == g.nmax
            and sn == sg and dout.stride(0) % 4 == 0 and dsl.data_ptr() % 16 == 0 and g.row_graph is not None):
        # the last layer has no batch-norm: its dU is a row-wise function of the readout gradient (no slot structure)
        nat.call("readout_l2_bwd_f32", g.graph_ptr, g.row_graph, B, g.n_rows, sg, v, v.stride(0), dsl, dout.stride(0), argl, N, rinv, du,
                 du.stride(0))
    elif (SLOT_WGRAD and l == 0 and L > 1 and not nodes and not ctx.needs_input_grad[0] and lean and B <= 32 and N == 128
          and K <= 128 and sn == sg and g.n_ghost == g.nmax and ctx.needs_input_grad[5] and z.stride(0) % 4 == 0
          and z.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0 and (not ctx.has_bias or ctx.needs_input_grad[6])):
        # layer 0's dU has ONE consumer, its own weight / bias gradient: both in one launch, the rows of dU stay in LDS
        per = int(os.environ.get("TSGNN_SLOT_WGRAD_PER", "2"))      # slots per workgroup (each slot is a full latency chain)
        nblk = max(1, -(-sn // per))
        ws0 = torch.empty(nblk * (K + 1) * N, dtype=torch.float32, device=dev)
        nat.call("slot_post_wgrad_f32", g.graph_ptr, g.slot_count, B, sn, g.n_rows, sg, v, v.stride(0), dxs, lddxs, dsl,
                 dout.stride(0) if dsl is not None else 0, argl, N, 1, 1, mean, rstd, rinv, z, z.stride(0), K, ws0, nblk)
        dw = red.grad(ctx.params[0], (K, N))
        db = red.grad(ctx.params[1] if ctx.has_bias else None, (N,))
        red.add((ws0, nblk, K, N, dw, db))
        grads[0], grads[1] = red.autograd_grad(dw), red.autograd_grad(db)
        keep.append(du)
        return None, 0
    elif ctx.per_graph and nodes:
        # per-graph statistics, node output: the block's own gradient + row layer norm + ReLU + normalise backward, row by row
        nat.call("row_post_nodes_bwd_f32", g.n_rows, g.n_rows + sg, v, v.stride(0), dxs, lddxs, dnode, dnode.stride(0),
                 1 if nodes == 2 else 0, N, post, post, mean, rstd, rinv, du, du.stride(0))
    elif ctx.per_graph:
        # per-graph statistics: readout winners + row layer norm + ReLU + normalise backward, row by row
        nat.call("row_post_bwd_f32", g.row_graph, B, g.n_rows, g.n_rows + sg, v, v.stride(0), dxs, lddxs, dsl, dout.stride(0), argl, N,
                 post, post, mean, rstd, rinv, du, du.stride(0))
    else:
        nat.call("slot_post_bwd_f32", g.graph_ptr, g.slot_count, B, sn, g.n_rows, sg, v, v.stride(0), dxs, lddxs, dnode,
                 dnode.stride(0) if dnode is not None else 0, dsl, dout.stride(0) if dsl is not None else 0, argl, N, post, post,
                 mean, rstd, rinv, du, du.stride(0))
    return du, sg


def _spend_du(ctx, l, du, bo, red, grads, keep):
    """layer l's gradients from its dU: weight-gradient slabs beside dX in the merged launch, else slabs / linear_wgrad / the bias
    column sum, and then the input gradient by the fused gather product or the transposed aggregation.  -> dX, or None when nobody asks"""
    g, W, sg = ctx.g, ctx.Ws[l], ctx.slots[1]
    z, lean, K, N = ctx.saved[l].z, ctx.saved[l].lean, W.size(0), W.size(1)
    want_w = ctx.needs_input_grad[5 + 2 * l]
    want_b = ctx.has_bias and ctx.needs_input_grad[6 + 2 * l]
    keep.append(du)
    dxs = sl = None
    if (MERGED_BWD and want_w and lean and l > 0 and K == 128 and N == 128 and g.symmetric and z.size(1) == K
            and _gather_ok(g, du) and z.data_ptr() % 16 == 0 and du.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0
            and W.stride(0) % 4 == 0):
        nslab, rps, need = mp.wgrad_plan(g.n_rows, K, N, z.stride(0), du.stride(0))
        nslab, rps, need = _slabs_beside_panels(nslab, rps, need, g.n_rows, K, N, du.device, g.panel_units)
        if 0 < nslab < 512:
            # weight-gradient slabs and dX = (A dU) W^T side by side in one launch (both only need dU); the forward's weight
            # image in input-gradient orientation (rows 2 (l - 1) + 1) stands in for W when there is one
            nb = _neighbours(g, *_gather_sched(g))
            ws = torch.empty(need, dtype=torch.float32, device=du.device)
            dxs = torch.empty(g.total_rows, K, dtype=torch.float32, device=du.device)
            nat.call("sage_layer_bwd_f32", *nb, du, du.stride(0), W, W.stride(0), dxs, dxs.stride(0), z, z.stride(0), g.n_rows, nslab, rps,
                     bo, ws, int(g.panel_units), ctx.w_img[2 * (l - 1) + 1] if ctx.w_img is not None else None)
            sl = (ws, nslab)
    if want_w and sl is None:
        if not lean and sg < g.n_ghost:
            du[g.n_rows + sg:].zero_()          # rows no slot kernel wrote
        sl = mp.linear_wgrad_slabs(z, K, du[:g.n_rows + bo] if lean else du, bias_only_rows=bo if lean else 0)
        if sl is None:
            if lean:
                z[g.n_rows:].zero_()
                du[g.n_rows + sg:].zero_()
            grads[2 * l], grads[2 * l + 1] = mp.linear_wgrad(z, K, du, want_b)
    elif want_b and not want_w:
        if sg < g.n_ghost:
            du[g.n_rows + sg:].zero_()
        grads[2 * l + 1] = mp.colsum(du)
    if sl is not None:                          # slabs now, ONE reduction for all layers at the end
        dw = red.grad(ctx.params[2 * l], (K, N))       # straight into the flat bucket if one is installed
        db = red.grad(ctx.params[2 * l + 1] if want_b else None, (N,))
        red.add((sl[0], sl[1], K, N, dw, db))
        grads[2 * l], grads[2 * l + 1] = red.autograd_grad(dw), red.autograd_grad(db)
    if dxs is not None or not (l > 0 or ctx.needs_input_grad[0]):
        return dxs
    R, ldz, dev = g.total_rows, z.size(1), du.device
    if (l > 0 and g.n_ghost > 0 and g.symmetric and ldz == K and K <= 128 and _gather_ok(g, du)
            and mp.rowgemm_ok(du, du.stride(0), W, W.stride(0), N, K, True)):
        # dX = A^T (dU W^T) = (A dU) W^T for a symmetric A: the same fused gather + product; only real rows
        nb = _neighbours(g)
        dxs = torch.empty(R, ldz, dtype=torch.float32, device=dev)
        nat.call("gather_rowgemm_f32", *nb, du, du.stride(0), W, W.stride(0), 1, None, dxs, dxs.stride(0), None, None, 0, g.n_rows, N, K, 0, 0)
        return dxs
    dz = torch.zeros(R, ldz, dtype=torch.float32, device=dev) if ldz > K else torch.empty(R, ldz, dtype=torch.float32, device=dev)
    keep.append(dz)
    if mp.rowgemm_ok(du, du.stride(0), W, W.stride(0), N, K, True):
        # ghost rows have no edges: their dz is never gathered, so only the real rows go through the product
        nat.call("rowgemm_f32", du, du.stride(0), W, W.stride(0), 1, None, dz, dz.stride(0), None, g.n_rows, N, K, 0, 0)
    else:
        mp.gemm(du, du.stride(0), 1, W, 1, W.stride(0), dz, dz.stride(0), 1, R, K, N)
    # ... and nothing reads the ghost rows of the aggregated gradient (slot_post_bwd takes 0 for them)
    return _aggregate_raw(g, dz, transposed=True, rows=g.n_rows if (l > 0 and g.n_ghost) else None)


class _SageStack(torch.autograd.Function):
    """forward(x0, g, has_bias, n_head, nodes, *conv params[, w1, b1, w2, b2]).  n_head = 0: returns the concatenated readout
    [B, P].  n_head = 4: the two chained nn.Linear after the readout (encoders.py:207-217) are part of the node: the last
    layer's readout, the decode of the earlier layers and the head run as ONE launch and (vec, y) are returned.
    nodes = 1 / 2: no readouts; returns the per-layer NODE features concatenated on the feature axis [R, P] (gcn_forward,
    encoders.py:140-167), 2 = ghost rows zeroed (the embedding mask); layers write straight into the concatenated buffer."""

    @staticmethod
    def forward(ctx, x0, g, has_bias, n_head, nodes, *params):
        head = params[len(params) - n_head:] if n_head else None
        params = params[:len(params) - n_head] if n_head else params
        s = _Fwd(x0, g, has_bias, nodes, params)
        per_graph = ctx.per_graph = bool(_PER_GRAPH[0])
        if per_graph and head is not None:
            raise NotImplementedError("per-graph statistics: the readout and the node-feature form of the stack only")
        ctx.w_img = ctx.pack_desc = None
        bnf = _fused_bn_workspace(s, head, per_graph)
        if bnf is not None:
            s.packed = bnf["packed"]
            saved, ctx.w_img, ctx.pack_desc = _forward_fused_bn(s, bnf)
        else:
            saved = _forward_layers(s, head, per_graph)
        ctx.g, ctx.L, ctx.has_bias, ctx.dims = g, s.L, has_bias, (s.Fh, s.Fl)
        ctx.slots, ctx.nodes = (s.sn, s.sg), nodes
        ctx.Ws, ctx.saved, ctx.params = s.Ws, saved, params
        result, ctx.arg, ctx.head = _forward_tail(s, head, bnf, saved)
        if ctx.head is not None:
            ctx.set_materialize_grads(False)
        return result

    @staticmethod
    def backward(ctx, *gouts):
        L = ctx.L
        keep = []
        if ctx.head is None:
            dout, du_last, head_grads = gouts[0].contiguous(), None, ()
        else:
            h = _head_backward(ctx, gouts, keep)
            if h is None:
                return (None,) * (5 + 2 * L + 4)
            dout, du_last, head_grads = h       # du_last: the last layer's dU when the head's backward launch produced it
        grads = [None] * (2 * L)
        dxs = dx0 = None
        red = mp.WgradSets(mp.wgrad_reduce_multi, max_sets_with_shares=4)     # ONE reduction for all layers' slabs, at the end
        for l in range(L - 1, -1, -1):
            du, bo = _layer_du(ctx, l, dout, dxs, du_last, red, grads, keep)
            if du is None:
                continue
            dx = _spend_du(ctx, l, du, bo, red, grads, keep)
            if dx is not None:
                dxs = dx
                if l == 0:
                    dx0 = dx
        red.close()
        del keep
        return (dx0, None, None, None, None) + tuple(grads) + head_grads


def _conv_params(convs):
    """(has_bias, [w0, b0, w1, b1, ...]): the node's parameter list; a one-element dummy in each bias's place when there is none"""
    has_bias = convs[0].bias is not None
    return has_bias, [p for c in convs for p in (c.weight, c.bias if has_bias else c.weight.new_zeros(1))]


def sage_stack_readouts(x, g, convs):
    """concatenated max readouts [B, hidden*(L-1)+embedding] of the conv stack (encoders.py:177-203)."""
    has_bias, params = _conv_params(convs)
    return _SageStack.apply(x, g, has_bias, 0, 0, *params)


def sage_stack_nodes(x, g, convs, mask_ghost):
    """per-layer node features concatenated on the feature axis [R, sum F] (gcn_forward, encoders.py:140-167)."""
    has_bias, params = _conv_params(convs)
    return _SageStack.apply(x, g, has_bias, 0, 2 if (mask_ghost and g.n_ghost) else 1, *params)


# ----------------------------------------------------------------------------- two stacks on one graph, launches shared
PAIR_LAUNCHES = os.environ.get("TSGNN_STACK_PAIRS", "1") != "0"
ZERO_RIDER = os.environ.get("TSGNN_ZERO_RIDER", "1") != "0"        # the embedding mask's clearing inside the last paired product launch


def _multi(tn, gs, zero=None):
    """one launch for the recorded argument tuples of <= 2 tsgnn_linear_wgrad_f32 (slab form) and <= 2 tsgnn_gather_rowgemm_f32
    calls; False when the entry point does not take the combination (csrc/multi.hip).  zero: two contiguous tensors that the
    products' filler blocks clear after their own rows (the deferred `_zero` records that follow the products)."""
    words = [len(tn), len(gs)]
    for a in tn:
        words += [nat._arg(v) or 0 for v in a[:11]]
    for a in gs:
        words += [(nat._arg(v) or 0) if not isinstance(v, bool) else int(v) for v in a[:20]]
    d = np.asarray(words, dtype=np.int64)
    if zero is not None:
        za, zb = zero
        if not (za.is_contiguous() and zb.is_contiguous()):
            return False
        return nat.try_call("sage_multi_zero_f32", d.ctypes.data, za, za.numel(), zb, zb.numel())
    return nat.try_call("sage_multi_f32", d.ctypes.data)


def _zero_after(q, i):
    return q[i + 1][1][0] if i + 1 < len(q) and q[i + 1][0] == "_zero" else None


def _slab_form(rec):
    return rec[0] == "linear_wgrad_f32" and len(rec[1]) >= 13 and rec[1][11] is None and rec[1][12] is None


def run_paired(qa, qb):
    """issue two launch records of INDEPENDENT computations (nat.deferred) in lockstep; where both are at the same kind of
    step, the two problems share a launch: gather products pairwise, weight-gradient slabs pairwise and together with the
    gather products that follow them (all four only read dU).  Any interleaving that keeps each record's order is valid."""
    i = j = 0
    while i < len(qa) and j < len(qb):
        a, b = qa[i], qb[j]
        if a[0] == b[0] == "gather_rowgemm_f32":
            za, zb = _zero_after(qa, i), _zero_after(qb, j)
            if ZERO_RIDER and za is not None and zb is not None and _multi([], [a[1], b[1]], zero=(za, zb)):
                i += 2; j += 2                      # the ghost rows' clearing rode in the products' filler blocks
                continue
            if _multi([], [a[1], b[1]]):
                i += 1; j += 1
                continue
        if _slab_form(a) and _slab_form(b):
            na = qa[i + 1] if i + 1 < len(qa) else (None,)
            nb = qb[j + 1] if j + 1 < len(qb) else (None,)
            if na[0] == nb[0] == "gather_rowgemm_f32" and _multi([a[1], b[1]], [na[1], nb[1]]):
                i += 2; j += 2
                continue
            if _multi([a[1], b[1]], []):
                i += 1; j += 1
                continue
        if a[0] == b[0] == "_zero":
            torch._foreach_zero_([a[1][0], b[1][0]])
            i += 1; j += 1
            continue
        if a[0] == b[0] and a[0] in _PAIRED and _PAIRED[a[0]](a[1], b[1]):
            i += 1; j += 1
            continue
        nat.run([a]); nat.run([b])
        i += 1; j += 1
    nat.run(qa[i:]); nat.run(qb[j:])


def _same(x, y):
    if torch.is_tensor(x) or torch.is_tensor(y):
        return torch.is_tensor(x) and torch.is_tensor(y) and x.data_ptr() == y.data_ptr()
    return x == y


def _pair_slot_bn(a, b):
    # (graph_ptr, slot_count, B, sn, n_rows, sg, v, ldv, N, relu, mean, rstd, y, ldy, zero_ptr, total)
    if a[14] is not None or b[14] is not None or not all(_same(a[k], b[k]) for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 13)):
        return False
    return nat.try_call("slot_bn_fwd_pair_f32", a[0], a[1], a[2], a[3], a[4], a[5], a[6], b[6], a[7], a[8], a[9], a[10], b[10], a[11], b[11],
                        a[12], b[12], a[13])


def _pair_slot_post_bwd(a, b):
    # (graph_ptr, slot_count, B, sn, n_rows, sg, v, ldv, dxs, lddxs, dxs2, lddxs2, dout, ldo, arg, N, relu, bn, mean, rstd, rinv, du, lddu)
    if any(t[12] is not None or t[14] is not None for t in (a, b)):
        return False
    if (a[8] is None) != (b[8] is None) or (a[10] is None) != (b[10] is None):
        return False
    if not all(_same(a[k], b[k]) for k in (0, 1, 2, 3, 4, 5, 7, 9, 11, 15, 16, 17, 22)):
        return False
    return nat.try_call("slot_post_bwd_pair_f32", a[0], a[1], a[2], a[3], a[4], a[5], a[6], b[6], a[7], a[8], b[8], a[9], a[10], b[10], a[11],
                        a[15], a[16], a[17], a[18], b[18], a[19], b[19], a[20], b[20], a[21], b[21], a[22])


def _pair_reduce(a, b):
    # 4 x (ws, nslab, K, N, dw, db), normparts, step: the sets of both records in one descriptor
    if a[24] is not None or a[25] is not None or b[24] is not None or b[25] is not None:
        return False
    sets = [mp.wgrad_set(*t[6 * k:6 * k + 6], kn=1, lddw=t[6 * k + 3]) for t in (a, b) for k in range(4) if t[6 * k] is not None]
    if not sets:
        return False
    d = mp._desc(sets)
    return nat.try_call("wgrad_reduce_sets_f32", d.ctypes.data, None, None)


_PAIRED = {"slot_bn_fwd_f32": _pair_slot_bn, "slot_post_bwd_f32": _pair_slot_post_bwd, "wgrad_reduce_multi_f32": _pair_reduce}


class _StackCtx:
    """what _SageStack.forward / backward need of an autograd context, for the two halves of _SageStackPair"""
    needs_input_grad = ()

    def set_materialize_grads(self, v):
        pass


class _SageStackPair(torch.autograd.Function):
    """two _SageStack nodes (node outputs) on the SAME graph whose launches are recorded and issued in pairs (run_paired): the
    embedding and the assignment stack of DiffPool's first level.  forward(xa, xb, g, has_bias, nodes_a, nodes_b, n_a, *params)."""

    @staticmethod
    def forward(ctx, xa, xb, g, has_bias, nodes_a, nodes_b, n_a, *params):
        ca, cb = _StackCtx(), _StackCtx()
        with nat.deferred() as qa:
            oa = _SageStack.forward(ca, xa, g, has_bias, 0, nodes_a, *params[:n_a])
        with nat.deferred() as qb:
            ob = _SageStack.forward(cb, xb, g, has_bias, 0, nodes_b, *params[n_a:])
        run_paired(qa, qb)
        ctx.ca, ctx.cb, ctx.n_a = ca, cb, n_a
        return oa, ob

    @staticmethod
    def backward(ctx, da, db):
        n, n_a = ctx.needs_input_grad, ctx.n_a
        ctx.ca.needs_input_grad = (n[0], False, False, False, False) + tuple(n[7:7 + n_a])
        ctx.cb.needs_input_grad = (n[1], False, False, False, False) + tuple(n[7 + n_a:])
        with nat.deferred() as qa:
            ga = _SageStack.backward(ctx.ca, da)
        with nat.deferred() as qb:
            gb = _SageStack.backward(ctx.cb, db)
        run_paired(qa, qb)
        return (ga[0], gb[0], None, None, None, None, None) + tuple(ga[5:]) + tuple(gb[5:])


def sage_stack_nodes_pair(xa, xb, g, convs_a, convs_b, mask_ghost):
    """sage_stack_nodes of two stacks on one graph, launches shared where both are at the same step"""
    has_bias = convs_a[0].bias is not None
    if (convs_b[0].bias is not None) != has_bias:
        return sage_stack_nodes(xa, g, convs_a, mask_ghost), sage_stack_nodes(xb, g, convs_b, mask_ghost)
    params = _conv_params(list(convs_a) + list(convs_b))[1]
    nodes = 2 if (mask_ghost and g.n_ghost) else 1
    # lazily built structures of the batch are built NOW: a build launch recorded inside one stack's launch record shifts it
    # against the other's, and the first step on a batch would run every launch singly (a different — split-K — product
    # kernel, so also slightly different numbers than every later step)
    if mp.ell_ok(xa) and g.val is None:
        g.ell()
        if not g.symmetric:
            g.transposed()
    return _SageStackPair.apply(xa, xb, g, has_bias, nodes, nodes, 2 * len(convs_a), *params)


def head_ok(g, convs, lin1, lin2):
    """the fused readout + head tail covers these shapes (else: sage_stack_readouts + message_passing.head2)"""
    P = sum(c.output_dim for c in convs)
    Fl = convs[-1].output_dim
    return (FUSED_TAIL and isinstance(lin1, torch.nn.Linear) and isinstance(lin2, torch.nn.Linear) and P % 4 == 0 and P <= 2048
            and Fl % 4 == 0 and Fl <= 128 and lin1.out_features <= 4096 and g.B <= 1024 and lin1.in_features == P
            and lin1.weight.data_ptr() % 16 == 0)


def sage_stack_head(x, g, convs, lin1, lin2):
    """(lin1(readout), lin2(lin1(readout))) with the readout tail and the head fused into the stack node."""
    has_bias, params = _conv_params(convs)
    vec, y = _SageStack.apply(x, g, has_bias, 4, 0, *params, lin1.weight, lin1.bias, lin2.weight, lin2.bias)
    y._tsgnn_defer_ce = True          # a cross-entropy on these logits may be folded into this node's backward (mp._SoftmaxCE)
    return vec, y
