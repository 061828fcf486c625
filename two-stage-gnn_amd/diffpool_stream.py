"""DiffPool triplet stream: a NEW triplet at every replay of ONE hipGraph for ``triplet.tripletnet`` over a ``SoftPoolingGcnEncoder``
(train_triplet.py --method=soft-assign: ``sampler()`` -> ``TNet(a, p, n)`` -> margin loss -> clip -> Adam, thousands of times per epoch).

``triplet_stream.TripletStream`` does this for the GraphSage family; the DiffPool encoder was refused there because of one node, the
level-0 contraction X' = S^T Z, A' = S^T A S (``diffpool._ContractRows``), which read CSR arrays, host-side sizes and host-built slab
lists.  On the capacity-padded batch the gather launch writes, ``diffpool._ContractCap`` (csrc/contract_cap.hip) takes its place; the
rest of the step already has a fixed shape: both level-0 stacks run as the fused per-graph node on the batch with all of its
ghost-slot rows, the pooled levels are [3, K, .] (``dense_stack_pg``), the tail is ``triplet._TripletTail``.

``PostTrainStream`` is the same batch at ONE graph per schedule entry: the anchor steps of the 2stg+ post-training phase
(train_triplet_pre_train.py:233-262 with --method=soft-assign), the concatenated readout rows of every level into the fused head of
csrc/posttrain_head.hip.  ``DiffPoolChecks`` holds the eligibility checks the two share.

The arena carries ONE feature table: a dataset whose ``assign_feats`` differ from ``feats`` is refused (``ValueError``)."""
import numpy as np
import torch

from . import _native as nat
from . import post_train as PT
from .triplet_stream import SageArenaStream, TripletSteps, _graph_dict, check_schedule, pack_arena, schedule_of  # noqa: F401  (the stream's vocabulary)

EAGER = "; use the eager drop-in, tripletnet.forward(a, p, n)"
# SoftPoolingGcnEncoder.forward derives `masked` from ``batch_num_nodes is not None`` and make_batch ignores the argument for a
# GraphBatch: the node counts themselves live on the device (graph_ptr), this stands in for them
SIZES_ON_DEVICE = ("the node counts are in graph_ptr, on the device",)


def check_assign_feats(graphs):
    """ValueError naming the first graph whose ``assign_feats`` differ from ``feats`` on its real rows [:n]"""
    for i, obj in enumerate(graphs):
        d = _graph_dict(obj)
        if "assign_feats" not in d or d["assign_feats"] is d["feats"]:
            continue
        n = int(d["num_nodes"])
        fa, ff = np.asarray(d["assign_feats"]), np.asarray(d["feats"])
        if fa.ndim != 2 or fa.shape[1:] != ff.shape[1:] or fa.shape[0] < n or not np.array_equal(fa[:n], ff[:n]):
            raise ValueError("graph %d: assign_feats differ from feats on [:num_nodes] (the arena carries one feature table)%s" % (i, EAGER))


class DiffPoolChecks:
    """the eligibility checks of the DiffPool streams, whatever the number ``self.B`` of graphs a schedule entry names"""

    def _family_ok(self, model):
        from .dense_encoders import SoftPoolingGcnEncoder
        return type(model) is SoftPoolingGcnEncoder and bool(model.concat) and bool(model.bn) and int(model.num_pooling) >= 1

    def _stacks_ok(self, model):
        """both level-0 stacks as the fused per-graph node on the gathered batch, every pooled stack on dense_stack_pg, the first
        contraction inside tsgnn_contract_cap_supported; a TypeError of its own names what failed"""
        from . import dense_encoders as E
        from . import dense_stack_pg, sage_stack

        def refuse(what):
            raise TypeError("%s: %s%s" % (self.NAME, what, self.EAGER))
        if not (E.FUSED_STACK and E.PER_GRAPH_STACK and E.PER_GRAPH_DENSE and E.READOUT_IN_CONTRACT and E.READOUT_COLUMNS):
            refuse("a fused route of dense_encoders is switched off")
        g, x, fin = self.g, self.x, self.arena.fin
        for what, convs in (("embedding", model.conv_stack()), ("assignment", model.assign_stack(0))):
            if convs[0].input_dim != fin or not sage_stack.eligible(g, convs, model.bn, x) or not E.per_graph_node_ok(g, convs):
                refuse("the level-0 %s stack does not run as the fused per-graph node on this dataset" % what)
        F = int(model.pred_input_dim)
        lib = nat.lib()
        for i in range(model.num_pooling):
            K = int(model.assign_linear(i).out_features)
            if K < 1:
                refuse("pooling level %d has no clusters" % i)
            if i == 0 and not (lib.tsgnn_contract_cap_supported(K, F) and lib.tsgnn_ragged_tn_direct_supported(K, int(g.nmax))):
                refuse("the first contraction (K = %d clusters, F = %d features) lies outside tsgnn_contract_cap_supported" % (K, F))
            xk = torch.empty(self.B, K, F, dtype=torch.float32, device=self.device)
            ak = torch.empty(self.B, K, K, dtype=torch.float32, device=self.device)
            stacks = [model.conv_stack(i + 1)] + ([model.assign_stack(i + 1)] if i + 1 < model.num_pooling else [])
            if not all(dense_stack_pg.eligible(xk, ak, convs) for convs in stacks):
                refuse("a stack of pooled level %d (K = %d) lies outside dense_stack_pg" % (i, K))
        return True


class TripletStream(TripletSteps, DiffPoolChecks, SageArenaStream):
    """``net``: a ``triplet.tripletnet`` over a ``SoftPoolingGcnEncoder`` with concat and bn, num_pooling >= 1 and
    final_dim == "output_dim"; ``graphs``: the dataset's graph objects.  The interface of ``triplet_stream.TripletStream``: ``load``,
    ``gather``, ``embed``, ``loss(criterion, target)``, ``position``, ``len``.  TypeError (ending in the eager drop-in) for a model
    whose stacks do not run as the fused per-graph nodes on the gathered batch or whose first contraction lies outside
    ``tsgnn_contract_cap_supported``."""

    NAME = "diffpool_stream.TripletStream"
    EAGER = EAGER
    TAKES = "takes a tripletnet over a SoftPoolingGcnEncoder with concat and bn, num_pooling >= 1 and final_dim == \"output_dim\""

    def __init__(self, net, graphs, nmax=None, max_steps=None):
        graphs = list(graphs)
        model = getattr(net, "model", None)
        if not self._model_ok(model):                   # (before the graphs are read; the base's constructor asks again)
            self._refuse(self.TAKES)
        check_assign_feats(graphs)
        super().__init__(model, graphs, 3, nmax, max_steps)
        self.net = net
        self._warm_up_schedule()

    def _model_ok(self, model):
        return self._family_ok(model) and model.final_dim == "output_dim"

    def embed(self):
        """gather + the model on the gathered batch -> (dist_p, dist_n, embed_a, embed_p, embed_n), as ``tripletnet.forward`` returns"""
        self.gather()
        return self.net._embed(self.x, self.g, SIZES_ON_DEVICE, self.x)


class PostTrainStream(PT.PostTrainSteps, DiffPoolChecks, SageArenaStream):
    """An epoch of the 2stg+ post-training steps with --method=soft-assign from ONE hipGraph: ``post_train.PostTrainStream`` for a
    ``SoftPoolingGcnEncoder(final_dim='pretrain')`` with concat and bn and num_pooling >= 1 under the installed head
    (``post_train.install_head``).  Per replay: the gather launch at one graph, ``TripletStream``'s fused levels on it, every level's
    readout concatenated (P = pred_input_dim * (num_pooling + 1) columns) and the fused head of csrc/posttrain_head.hip, whose label is
    ``labels[ids_out[0]]`` read on the device.  ``load(anchors)``, ``step()`` -> (loss, pred, out), ``step_loss()``, ``position``,
    ``len`` as ``post_train.PostTrainStream``; TypeErrors end in ``post_train.post_train_step``; ``mine()`` refuses (no negative)."""

    NAME = "diffpool_stream.PostTrainStream"
    EAGER = PT.EAGER
    SIZES = SIZES_ON_DEVICE
    TAKES = "takes a SoftPoolingGcnEncoder with concat and bn, num_pooling >= 1 and final_dim == \"pretrain\""

    def __init__(self, model, graphs, nmax=None, max_steps=None):
        graphs = list(graphs)
        if not self._model_ok(model):                   # (before the graphs are read; the base's constructor asks again)
            self._refuse(self.TAKES)
        check_assign_feats(graphs)
        layers = PT.head_layers(model)
        if layers is not None:                     # (a label the head has no class for: named before anything is packed or uploaded)
            PT.label_table(graphs, layers[3].out_features)
        super().__init__(model, graphs, 1, nmax, max_steps)
        self._init_post_train(model, graphs)

    def _model_ok(self, model):
        return self._family_ok(model) and model.final_dim == "pretrain"

    def _readout_width(self, model):
        return int(model.pred_input_dim) * (int(model.num_pooling) + 1)
