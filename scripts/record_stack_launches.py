#!/usr/bin/env python3
"""The launch records of the fused GraphSage stack node (two_stage_gnn_amd/sage_stack.py) -> tests/golden/sage_stack_launches.json and of
the DiffPool / base encoders' host code around it (two_stage_gnn_amd/dense_encoders.py) -> tests/golden/diffpool_launches.json.

For every configuration below (tiny shapes, one per branch of the node: each switch flipped from its default, the head / readout /
node / pair routes, the shapes that steer the fallbacks) the model and the batch are built from fixed seeds and forward + backward
run twice: the first run builds the batch's lazy structures (neighbour table, gather schedule, du_map, readout map), the second is
recorded through ``_native.trace``.  A record is the list of (entry point, dispatched kernel, canonical arguments):

  tensor -> ["t", k], k = order of first appearance of its data_ptr() in the record (the trace keeps every argument alive, so no
  address is reused inside a record); None, bool, int, float as they are (floats exact); an int >= 2**32 is a host address -> "addr".

Beside the record: a sha256 over the bytes of the outputs and of every gradient, kept only where it is reproducible.

The second family pins SoftPoolingGcnEncoder.forward + loss + backward (masked / unmasked, assign_x, every final_dim, linkpred,
0 / 1 / 2 pooling levels, each switch of the two-level model flipped once, the triplet step's per-graph routes) and the
GcnEncoderGraph heads the first family does not reach.

tests/test_gpu_sage_stack_launches.py compares the tree's launches with the committed files.  A change that alters a launch sequence
ON PURPOSE re-records the files from its own tree and shows their diff; a refactor leaves them untouched.

Usage:  python scripts/record_stack_launches.py [--out DIR] [--previous DIR]
        --out: the directory that takes one file per family (default: tests/golden)
        --previous: the result of an earlier process; the launch records must equal its records (else something in them is not
        canonical), and a digest that differs between the two is dropped from the output (and named).
"""
import argparse
import hashlib
import importlib
import json
import numbers
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from util_graphs import dd_like_sizes, dense_batch  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
GOLDENS = {"sage_stack": "sage_stack_launches.json", "diffpool": "diffpool_launches.json"}       # family -> its file in GOLDEN_DIR
GOLDEN = os.path.join(GOLDEN_DIR, GOLDENS["sage_stack"])        # the first family's file, under the name it has always had here
_DD6 = dict(B=6, nmax=150, sizes=dd_like_sizes(3, 6, nbar=70, nmax=150).tolist(), p_edge=0.06, seed=5)
_DD3 = dict(B=3, nmax=150, sizes=_DD6["sizes"][:3], p_edge=0.06, seed=5)
# DiffPool: Nmax 64 at assign_ratio 0.25 -> K = 16 clusters at level 0 and K = 4 at level 1 (a graph that fills every slot among them)
_DP4 = dict(B=4, nmax=64, sizes=[64, 23, 37, 50], p_edge=0.1, seed=11)
_DP3 = dict(B=3, nmax=64, sizes=[64, 23, 37], p_edge=0.1, seed=11)


def _cfg(name, route="head", shape=_DD6, hid=128, layers=3, fin=89, flags=None, expect=(), absent=(), **kw):
    """flags: {switch: value}, a switch being "module.NAME" in the package, or a bare NAME of sage_stack"""
    return dict(name=name, route=route, shape=shape, hid=hid, layers=layers, fin=fin, flags=dict(flags or {}), expect=tuple(expect),
                absent=tuple(absent), **kw)


def _dp(name, pooling=1, shape=_DP4, **kw):
    """a SoftPoolingGcnEncoder configuration: hidden = embedding = assign-hidden = 64, 3 layers, 8 input features"""
    return _cfg("dp_" + name, shape=shape, hid=64, fin=8, family="diffpool", encoder="diffpool", pooling=pooling, **kw)


def configurations(family="sage_stack"):
    """the configurations of one family (None: of all), in the order of the golden files; `expect` / `absent`: entry points the record
    must (not) contain, so a configuration that drifts off the branch it exists for fails instead of pinning another one.  Called
    without an argument it answers as it did when the fused stack node was the only family: a caller written then still works."""
    c = _sage_stack_configurations() + _diffpool_configurations()
    return [x for x in c if family is None or x.get("family", "sage_stack") == family]


def _diffpool_configurations():
    """SoftPoolingGcnEncoder.forward / GcnEncoderGraph.forward and what they consult: one configuration per branch of the host code"""
    E, S, D, M = "dense_encoders.", "sage_stack.", "dense_stack.", "message_passing."
    # level 0: the embedding stack (64 | 64 | 64 columns) and the assignment stack (64 | 64 | 16) share launches pairwise; 16
    # assignment columns lie below the paired launches' 33..64, so the LAST layers run one by one (recorded as they run)
    pair, contract = ("sage_multi_f32", "slot_bn_fwd_f32"), ("ragged_tn_direct_ro_f32", "contract_rows_bwd_ro_f32")
    dense, tail = ("contract_dense_fwd_ro_f32", "contract_dense_bwd_ro_f32", "dense_stack_fwd_f32"), ("head2_fwd_ro_f32", "head2_bwd_ro_f32")
    c = [_dp("default", expect=pair + contract + tail + ("dense_stack_fwd_f32",), absent=("readout_max_fwd_f32",)),
         _dp("pool2", pooling=2, expect=pair + contract + dense + tail, absent=("readout_max_fwd_f32",)),
         _dp("unmasked", padded=True, expect=("sage_multi_f32", "ell_spmm_f32") + contract + tail),
         _dp("assign_x", assign_x=True, expect=("pack_rows_f32",) + pair + contract),
         _dp("pretrain", final_dim="pretrain", expect=contract + tail),
         _dp("output_dim", final_dim="output_dim", expect=contract + ("readout_max_fwd_f32",), absent=("head2_fwd_ro_f32", "head2_fwd_f32")),
         _dp("linkpred", linkpred=True, expect=contract + ("linkpred_loss_f32",)),
         _dp("pool0", pooling=0, expect=("readout_max_fwd_f32", "head2_fwd_f32"), absent=("sage_multi_f32", "ragged_tn_direct_ro_f32"))]
    # (SOFTMAX_IN_CONTRACT off shows in no entry point's name: one row_softmax_masked launch more each way, pinned by the record)
    off = {E + "FUSED_STACK": (("bn_slots_fwd_f32",) + dense, ("sage_multi_f32", "slot_bn_fwd_f32")),
           E + "FUSED_HEAD": (("readout_max_fwd_f32",) + dense, ("head2_fwd_ro_f32", "head2_fwd_f32")),
           E + "FUSED_DENSE_STACK": (("gemm_f32", "contract_dense_fwd_ro_f32"), ("dense_stack_fwd_f32",)),
           E + "READOUT_IN_CONTRACT": (("readout_max_bwd_rows_f32", "contract_rows_bwd_f32") + tail, ("contract_rows_bwd_ro_f32",)),
           E + "SOFTMAX_IN_CONTRACT": (dense + tail, ()),
           E + "READOUT_COLUMNS": (("readout_max_fwd_f32", "head2_fwd_f32") + dense, ("head2_fwd_ro_f32",)),
           S + "PAIR_LAUNCHES": (("gather_rowgemm_f32", "slot_bn_fwd_f32") + dense, ("sage_multi_f32",)),
           D + "ONE_LAUNCH": (("gemm_f32", "contract_dense_fwd_ro_f32"), ("dense_stack_fwd_f32",)),
           M + "HEAD_TAIL": (("readout_max_fwd_f32", "head2_fwd_f32") + dense, ("head2_fwd_ro_f32",))}
    for k, (exp, ab) in off.items():
        c.append(_dp("pool2_%s_off" % k.split(".")[1], pooling=2, flags={k: False}, expect=exp, absent=ab))
    # per-graph statistics: three graphs through triplet.tripletnet._embed
    trip = dict(pooling=2, shape=_DP3, route="triplet", final_dim="output_dim")
    c.append(_dp("triplet", expect=("row_ln_fwd_f32", "row_post_nodes_bwd_f32", "dense_pg_layer_fwd_f32", "triplet_embed_fwd_f32") + contract,
                 absent=("slot_bn_fwd_f32", "sage_multi_f32"), **trip))
    c.append(_dp("triplet_PER_GRAPH_STACK_off", flags={E + "PER_GRAPH_STACK": False}, expect=("row_ln_bwd_f32", "dense_pg_layer_fwd_f32"),
                 absent=("row_post_nodes_bwd_f32",), **trip))
    c.append(_dp("triplet_PER_GRAPH_DENSE_off", flags={E + "PER_GRAPH_DENSE": False}, expect=("row_post_nodes_bwd_f32", "gemm_f32"),
                 absent=("dense_pg_layer_fwd_f32",), **trip))
    # GcnEncoderGraph beside the "number_classes" head the sage_stack family records
    enc, readouts = dict(family="diffpool"), ("readout_decode_layers_f32", "readout_l2_bwd_f32")
    c.append(_cfg("enc_pretrain", final_dim="pretrain", expect=("packed_head_fwd_z_f32", "head2_bwd_du_map_f32"), **enc))
    c.append(_cfg("enc_output_dim", final_dim="output_dim", expect=readouts, absent=("packed_head_fwd_z_f32",), **enc))
    c.append(_cfg("enc_pretrain_FUSED_HEAD_off", final_dim="pretrain", flags={E + "FUSED_HEAD": False}, expect=readouts,
                  absent=("packed_head_fwd_z_f32", "head2_fwd_f32"), **enc))
    # concat=False: add_self layers, the stack falls to the composed path and the last layer's readout alone feeds the head.  (The
    # DiffPool encoder has no such configuration: like the reference's, its gcn_forward concatenates whatever `concat` says, and the
    # pooled levels' and the head's input widths then do not match.)
    # (no digest: the launches repeat, the bits of this per-op route were seen to differ between a recorder process and a long test session)
    c.append(_cfg("enc_no_concat", concat=False, digest=False, expect=("bn_slots_fwd_f32", "readout_max_fwd_f32", "head2_fwd_f32"),
                  absent=("slot_bn_fwd_f32", "readout_decode_layers_f32"), **enc))
    for fd in ("output_dim", "pretrain"):           # tripletnet applies map_model itself (_defer_map)
        c.append(_cfg("enc_triplet_" + fd, route="triplet", shape=_DD3, final_dim=fd,
                      expect=("row_ln_fwd_f32", "row_post_bwd_f32", "triplet_embed_fwd_f32") + readouts, absent=("slot_bn_fwd_f32",), **enc))
    return c


def _sage_stack_configurations():
    c = [_cfg("head_default", expect=("gather_rowgemm_st_f32", "sage_layer_fwd_bn_f32", "packed_head_fwd_z_f32", "head2_bwd_du_map_f32",
                                      "sage_layer_bwd_f32"))]
    off = {"FUSED_BN": (("slot_bn_fwd_f32", "sage_layer_fwd_ro_f32", "packed_head_fwd_f32"), ("sage_layer_fwd_bn_f32",)),
           "MERGED_FWD": (("gather_rowgemm_f32", "readout_partial_f32", "readout_head_fwd_f32"), ("sage_layer_fwd_f32",)),
           "MERGED_BWD": (("gather_rowgemm_f32",), ("sage_layer_bwd_f32",)),
           "GATHER_FUSED": (("rowgemm_f32",), ("gather_rowgemm_f32", "gather_rowgemm_st_f32")),
           "FUSED_TAIL": (("readout_decode_layers_f32",), ("packed_head_fwd_z_f32",)),
           "EPILOGUE_READOUT": (("sage_layer_fwd_f32", "readout_head_fwd_f32"), ("sage_layer_fwd_ro_f32", "sage_layer_fwd_bn_f32")),
           "LAST_LAYER_ROWS": (("slot_post_bwd_f32",), ("readout_l2_bwd_f32", "head2_bwd_du_map_f32")),
           "RO_MAP": (("sage_layer_fwd_bn_f32",), ()),
           "HEAD_DU": (("readout_l2_bwd_f32",), ("head2_bwd_du_map_f32",)),
           "DU_MAP": (("head2_bwd_du_map_f32",), ()),
           "GATHER_SCHED": (("sage_layer_fwd_bn_f32",), ()),
           "GATHER_SCHED_L0": (("gather_rowgemm_st_f32",), ()),
           "L0_DIRECT_B": (("gather_rowgemm_st_mode_f32",), ("gather_rowgemm_st_f32",)),
           "SLABS_BESIDE": (("sage_layer_bwd_f32",), ())}
    for k, (exp, ab) in off.items():
        c.append(_cfg("head_%s_off" % k, flags={k: False}, expect=exp, absent=ab))
    c.append(_cfg("head_SLOT_WGRAD_on", flags={"SLOT_WGRAD": True}, expect=("slot_post_wgrad_f32", "sage_layer_fwd_bn_f32")))
    c.append(_cfg("head_SLOT_WGRAD_on_FUSED_BN_off", flags={"SLOT_WGRAD": True, "FUSED_BN": False},
                  expect=("slot_post_wgrad_f32", "slot_bn_fwd_f32")))
    c.append(_cfg("head_h64", hid=64, expect=("gather_rowgemm_f32", "slot_bn_fwd_f32"), absent=("sage_layer_fwd_bn_f32",)))
    c.append(_cfg("head_L2", layers=2, expect=("sage_layer_fwd_bn_f32", "packed_head_fwd_z_f32")))
    c.append(_cfg("head_L2_h64", layers=2, hid=64, expect=("gather_rowgemm_f32", "slot_bn_fwd_f32"), absent=("sage_layer_fwd_bn_f32",)))
    c.append(_cfg("head_full_graph", shape=dict(B=5, nmax=96, sizes=[96, 40, 61, 17, 80], p_edge=0.08, seed=9), expect=("head2_bwd",)))
    c.append(_cfg("head_single_graph", shape=dict(B=1, nmax=200, sizes=[137], p_edge=0.05, seed=9), expect=("head2_bwd",)))
    c.append(_cfg("head_high_degree", shape=dict(B=3, nmax=100, sizes=[90, 75, 60], p_edge=0.35, seed=9), expect=("head2_bwd",),
                  need_tail=True))
    # an adjacency with a value per edge (what GraphBatch.from_dense keeps): CSR aggregation beside the products
    c.append(_cfg("head_weighted", weighted=True, expect=("csr_spmm_f32", "rowgemm_f32"), absent=("gather_rowgemm_f32", "gather_rowgemm_st_f32")))
    c.append(_cfg("readouts", route="readouts", expect=("slot_bn_fwd_f32", "readout_decode_layers_f32", "slot_post_bwd_f32")))
    c.append(_cfg("readouts_per_graph", route="readouts", per_graph=True,
                  shape=dict(B=3, nmax=150, sizes=_DD6["sizes"][:3], p_edge=0.06, seed=5),
                  expect=("row_ln_fwd_f32", "row_post_bwd_f32", "readout_decode_layers_f32"), absent=("slot_bn_fwd_f32",)))
    # (padded rows keep the width of the input: a multiple of 4 for the node to take them)
    c.append(_cfg("nodes1_no_ghost", route="nodes", padded=True, mask=False, fin=88, expect=("slot_bn_fwd_f32", "slot_post_bwd_f32"),
                  absent=("readout_decode_layers_f32",)))
    c.append(_cfg("nodes2_masked", route="nodes", mask=True, expect=("slot_bn_fwd_f32", "slot_post_bwd_f32"),
                  absent=("readout_decode_layers_f32",)))
    c.append(_cfg("nodes2_per_graph", route="nodes", mask=True, per_graph=True, expect=("row_ln_fwd_f32", "row_post_nodes_bwd_f32"),
                  absent=("slot_bn_fwd_f32",)))
    # (the shared launches of csrc/multi.hip take products 33..64 columns wide)
    c.append(_cfg("pair_zero_rider", route="pair", mask=True, hid=64, expect=("sage_multi_zero_f32", "slot_bn_fwd_pair_f32",
                                                                    "slot_post_bwd_pair_f32")))
    c.append(_cfg("pair_ZERO_RIDER_off", route="pair", mask=True, hid=64, flags={"ZERO_RIDER": False}, expect=("sage_multi_f32",),
                  absent=("sage_multi_zero_f32",)))
    c.append(_cfg("pair_bias_differs", route="pair", mask=True, hid=64, bias_b=False, expect=("gather_rowgemm_f32", "slot_bn_fwd_f32"),
                  absent=("sage_multi_f32", "sage_multi_zero_f32")))
    # no gradient for the input (l = 0 needs no dX), for layer 0's bias and for layer 1's weight (its bias alone: a column sum)
    c.append(_cfg("readouts_partial_grads", route="readouts", x_grad=False, frozen=("conv_first.bias", "conv_block.0.weight"),
                  expect=("readout_decode_layers_f32", "colsum")))
    return c


def _canonical(trace):
    ids, out = {}, []

    def one(a):
        if a is None or isinstance(a, (bool, str)):
            return a
        if isinstance(a, torch.Tensor):
            return ["t", ids.setdefault(a.data_ptr(), len(ids))]
        if isinstance(a, (numbers.Integral, np.integer)):
            return "addr" if int(a) >= 2 ** 32 else int(a)
        if isinstance(a, (float, np.floating)):
            return float(a)
        raise TypeError("launch argument of type %s has no canonical form" % type(a).__name__)
    for name, args, kernel in trace:
        out.append([name, kernel, [one(a) for a in args]])
    return out


def _model(fin, cfg, seed, bias=True):
    from two_stage_gnn_amd import dense_encoders as E

    class A:
        pass
    A.bias = bias
    torch.manual_seed(seed)
    hid, final_dim = cfg["hid"], cfg.get("final_dim", "number_classes")
    if cfg.get("encoder") == "diffpool":
        m = E.SoftPoolingGcnEncoder(cfg["shape"]["nmax"], fin, hid, hid, 2, cfg["layers"], hid, assign_ratio=0.25, num_pooling=cfg["pooling"],
                                    bn=True, linkpred=cfg.get("linkpred", False), assign_input_dim=fin, args=A(), final_dim=final_dim)
    else:
        m = E.GcnEncoderGraph(fin, hid, hid, 2, cfg["layers"], concat=cfg.get("concat", True), bn=True, args=A(), final_dim=final_dim)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("bias") and "conv" in k:
                p.copy_(torch.randn_like(p) * 0.2)           # ghost rows (the normalised bias) take part in every readout
    for k, p in m.named_parameters():
        if k in cfg.get("frozen", ()):
            p.requires_grad_(False)
    return m.cuda()


def _switch(key):
    """"module.NAME" -> (that module of the package, NAME); a bare NAME is a switch of sage_stack"""
    mod, _, name = key.rpartition(".")
    return importlib.import_module("two_stage_gnn_amd." + (mod or "sage_stack")), name


def record(cfg):
    """-> {"launches": [[entry point, kernel, canonical arguments], ...], "digest": sha256 of outputs and gradients} of the SECOND of
    two forward + backward runs of the configuration"""
    from two_stage_gnn_amd import _native as nat, sage_stack as S
    from two_stage_gnn_amd.graph import GraphBatch
    sh = cfg["shape"]
    fin = cfg["fin"]
    x, adj, sizes = dense_batch(sh["seed"], sh["B"], sh["nmax"], fin, sizes=sh["sizes"], p_edge=sh["p_edge"])
    models = [_model(fin, cfg, 1)] + ([_model(fin, cfg, 2, bias=cfg.get("bias_b", True))] if cfg["route"] == "pair" else [])
    g = GraphBatch.from_dense(adj.cuda(), None if cfg.get("padded") else sizes, layout="padded" if cfg.get("padded") else "packed",
                              assume_symmetric=True)
    if not cfg.get("weighted"):
        g.val = None                                         # 0 / 1 entries: unit weights (what the data pipeline's batches carry)
    xr, g = models[0].make_batch(x.cuda(), g, None)
    if cfg.get("need_tail"):
        assert g.ell()[2] is not None, "%s: the neighbour table has no CSR tail" % cfg["name"]
    if cfg["route"] not in ("head", "triplet"):
        assert all(S.eligible(g, m.conv_stack(), True, xr) for m in models), cfg["name"]
        xr = xr.detach().requires_grad_(cfg.get("x_grad", True))
    label = (torch.arange(sh["B"]) % 2).cuda()
    # SoftPoolingGcnEncoder masks where it is given node counts; a padded [B, Nmax, F] assignment input is packed by its forward
    counts = sizes if cfg.get("encoder") == "diffpool" and not cfg.get("padded") else None
    assign = {"assign_x": dense_batch(sh["seed"] + 1, sh["B"], sh["nmax"], fin, sizes=sh["sizes"])[0].cuda()} if cfg.get("assign_x") else {}
    if cfg["route"] == "triplet":
        from two_stage_gnn_amd.triplet import tripletnet
        net, target = tripletnet(models[0]), torch.tensor([-1.0]).cuda()
    gen = torch.Generator().manual_seed(7)

    def step():
        m = models[0]
        if cfg["route"] == "head":
            outs = m(xr, g, counts, **assign)
            m.loss(outs[0] if cfg.get("final_dim") == "pretrain" else outs[1], label).backward()
            return list(outs)
        if cfg["route"] == "triplet":           # -> (dist_p, dist_n, embed_a, embed_p, embed_n)
            outs = net._embed(xr, g, sizes, xr)
            torch.nn.MarginRankingLoss(margin=1.0)(outs[0], outs[1], target).backward()
            return list(outs)
        with S.per_graph_stats(bool(cfg.get("per_graph"))):
            if cfg["route"] == "readouts":
                outs = [S.sage_stack_readouts(xr, g, m.conv_stack())]
            elif cfg["route"] == "nodes":
                outs = [S.sage_stack_nodes(xr, g, m.conv_stack(), cfg["mask"])]
            else:
                outs = list(S.sage_stack_nodes_pair(xr, xr, g, m.conv_stack(), models[1].conv_stack(), cfg["mask"]))
        gen.manual_seed(7)
        sum((o * torch.randn(o.shape, generator=gen).cuda()).sum() for o in outs).backward()
        return outs
    flags = [(_switch(k), v) for k, v in cfg["flags"].items()]
    old = [(mk, getattr(*mk)) for mk, _ in flags]
    prev = nat.trace
    try:
        for mk, v in flags:
            setattr(*mk, v)
        step()
        for m in models:
            m.zero_grad(set_to_none=True)
        xr.grad = None
        nat.trace = []
        outs = step()
        torch.cuda.synchronize()
        trace = nat.trace
    finally:
        nat.trace = prev
        for mk, v in old:
            setattr(*mk, v)
    launches = _canonical(trace)
    names = [r[0] for r in launches]
    for e in cfg["expect"]:
        assert any(n.startswith(e) for n in names), "%s: no %s launch in %s" % (cfg["name"], e, names)
    for e in cfg["absent"]:
        assert e not in names, "%s: unexpected %s launch in %s" % (cfg["name"], e, names)
    if not cfg.get("digest", True):
        return {"launches": launches}
    h = hashlib.sha256()
    grads = [p.grad for m in models for p in m.parameters()] + [xr.grad]
    for t in [t for t in outs + grads if t is not None]:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return {"launches": launches, "digest": h.hexdigest()}


def write_golden(path, res):
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in res.items()) + "\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN_DIR)
    ap.add_argument("--previous", default=None)
    a = ap.parse_args()
    failed = []
    for family, fname in GOLDENS.items():
        prev = json.load(open(os.path.join(a.previous, fname))) if a.previous else None
        res = {}
        for cfg in configurations(family):
            try:
                r = json.loads(json.dumps(record(cfg)))
            except AssertionError as e:
                failed.append(str(e))
                print("FAILED", e)
                continue
            if prev is not None:
                assert r["launches"] == prev[cfg["name"]]["launches"], "%s: the launch record differs between two processes" % cfg["name"]
                if "digest" in r and r["digest"] != prev[cfg["name"]].get("digest"):
                    print("digest not reproducible, dropped:", cfg["name"])
                    del r["digest"]
            res[cfg["name"]] = r
            print("%-34s %3d launches  %s" % (cfg["name"], len(r["launches"]), " ".join(sorted(set(x[0] for x in r["launches"])))))
        write_golden(os.path.join(a.out, fname), res)
    if failed:
        sys.exit("%d configuration(s) off their branch" % len(failed))


if __name__ == "__main__":
    main()
