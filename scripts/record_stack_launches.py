#!/usr/bin/env python3
"""The launch record of the fused GraphSage stack node (two_stage_gnn_amd/sage_stack.py) -> tests/golden/sage_stack_launches.json.

For every configuration below (tiny shapes, one per branch of the node: each switch flipped from its default, the head / readout /
node / pair routes, the shapes that steer the fallbacks) the model and the batch are built from fixed seeds and forward + backward
run twice: the first run builds the batch's lazy structures (neighbour table, gather schedule, du_map, readout map), the second is
recorded through ``_native.trace``.  A record is the list of (entry point, dispatched kernel, canonical arguments):

  tensor -> ["t", k], k = order of first appearance of its data_ptr() in the record (the trace keeps every argument alive, so no
  address is reused inside a record); None, bool, int, float as they are (floats exact); an int >= 2**32 is a host address -> "addr".

Beside the record: a sha256 over the bytes of the outputs and of every gradient, kept only where it is reproducible.

tests/test_gpu_sage_stack_launches.py compares the tree's launches with the committed file.  A change that alters the launch sequence
ON PURPOSE re-records the file from its own tree and shows the file's diff; a refactor leaves it untouched.

Usage:  python scripts/record_stack_launches.py [--out FILE] [--previous FILE]
        --previous: the result of an earlier process; the launch records must equal its records (else something in them is not
        canonical), and a digest that differs between the two is dropped from the output (and named).
"""
import argparse
import hashlib
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "sage_stack_launches.json")
_DD6 = dict(B=6, nmax=150, sizes=dd_like_sizes(3, 6, nbar=70, nmax=150).tolist(), p_edge=0.06, seed=5)


def _cfg(name, route="head", shape=_DD6, hid=128, layers=3, fin=89, flags=None, expect=(), absent=(), **kw):
    return dict(name=name, route=route, shape=shape, hid=hid, layers=layers, fin=fin, flags=dict(flags or {}), expect=tuple(expect),
                absent=tuple(absent), **kw)


def configurations():
    """the configurations, in the order of the golden file; `expect` / `absent`: entry points the record must (not) contain, so a
    configuration that drifts off the branch it exists for fails instead of pinning another one"""
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
    m = E.GcnEncoderGraph(fin, cfg["hid"], cfg["hid"], 2, cfg["layers"], bn=True, args=A(), final_dim="number_classes")
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("bias") and "conv" in k:
                p.copy_(torch.randn_like(p) * 0.2)           # ghost rows (the normalised bias) take part in every readout
    for k, p in m.named_parameters():
        if k in cfg.get("frozen", ()):
            p.requires_grad_(False)
    return m.cuda()


def _convs(m):
    return [m.conv_first] + list(m.conv_block) + [m.conv_last]


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
    if cfg["route"] != "head":
        assert all(S.eligible(g, _convs(m), True, xr) for m in models), cfg["name"]
        xr = xr.detach().requires_grad_(cfg.get("x_grad", True))
    label = (torch.arange(sh["B"]) % 2).cuda()
    gen = torch.Generator().manual_seed(7)

    def step():
        m = models[0]
        if cfg["route"] == "head":
            outs = m(xr, g)
            m.loss(outs[1], label).backward()
            return list(outs)
        with S.per_graph_stats(bool(cfg.get("per_graph"))):
            if cfg["route"] == "readouts":
                outs = [S.sage_stack_readouts(xr, g, _convs(m))]
            elif cfg["route"] == "nodes":
                outs = [S.sage_stack_nodes(xr, g, _convs(m), cfg["mask"])]
            else:
                outs = list(S.sage_stack_nodes_pair(xr, xr, g, _convs(m), _convs(models[1]), cfg["mask"]))
        gen.manual_seed(7)
        sum((o * torch.randn(o.shape, generator=gen).cuda()).sum() for o in outs).backward()
        return outs
    old = {k: getattr(S, k) for k in cfg["flags"]}
    prev = nat.trace
    try:
        for k, v in cfg["flags"].items():
            setattr(S, k, v)
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
        for k, v in old.items():
            setattr(S, k, v)
    launches = _canonical(trace)
    names = [r[0] for r in launches]
    for e in cfg["expect"]:
        assert any(n.startswith(e) for n in names), "%s: no %s launch in %s" % (cfg["name"], e, names)
    for e in cfg["absent"]:
        assert e not in names, "%s: unexpected %s launch in %s" % (cfg["name"], e, names)
    h = hashlib.sha256()
    grads = [p.grad for m in models for p in m.parameters()] + [xr.grad]
    for t in outs + [t for t in grads if t is not None]:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return {"launches": launches, "digest": h.hexdigest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--previous", default=None)
    a = ap.parse_args()
    prev = json.load(open(a.previous)) if a.previous else None
    res, failed = {}, []
    for cfg in configurations():
        try:
            r = json.loads(json.dumps(record(cfg)))
        except AssertionError as e:
            failed.append(str(e))
            print("FAILED", e)
            continue
        if prev is not None:
            assert r["launches"] == prev[cfg["name"]]["launches"], "%s: the launch record differs between two processes" % cfg["name"]
            if r["digest"] != prev[cfg["name"]].get("digest"):
                print("digest not reproducible, dropped:", cfg["name"])
                del r["digest"]
        res[cfg["name"]] = r
        print("%-34s %3d launches  %s" % (cfg["name"], len(r["launches"]), " ".join(sorted(set(x[0] for x in r["launches"])))))
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in res.items()) + "\n}\n")
    if failed:
        sys.exit("%d configuration(s) off their branch" % len(failed))


if __name__ == "__main__":
    main()
