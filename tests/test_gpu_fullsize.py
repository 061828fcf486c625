"""Parity of the TIMED steps at their TIMED sizes ("next round" item 1).

Every test builds exactly what `bench.py` / `scripts/config_bench.py` time — the same synthetic batch, the same model ctor
arguments, `FlatTrainer` + `GraphedStep` (one hipGraph: forward, loss, backward, gradient bucket, clip, Adam) — replays k = 3
optimiser steps and compares, AFTER EACH STEP, the loss, the logits, the gradient norm and every parameter with the CPU oracle
(`oracle/dense_ref.py`, `oracle/pyg_ref.py`) driven by `clip_grad_norm_(2.0)` + `torch.optim.Adam`, i.e. the body of the reference's
loop (train.py:110-131).  The oracle runs twice, in fp32 and in fp64; fp64 arbitrates wherever fp32 itself is ill-conditioned
(ReLU / arg-max winners that flip on a last-bit difference, Adam's first steps being `lr * sign(g)` for tiny |g|):

  loss, logits   |hip - fp64| <= max(10 * |cpu32 - fp64|, 1e-4 * scale)        (north_star: 1e-4 fp32)
  parameters     on the movement since step 0, per tensor, with u = lr * steps (what Adam can move an entry):
                 max|hip - fp64| <= max(10 * max|cpu32 - fp64|, 0.02 * u), and at most a handful of entries (or 4x as many as
                 the fp32 CPU run has) further than 0.01 * u from fp64.

Reference: encoders.py:169-224 (SAGE), :327-406 (DiffPool), encoders_GAT.py:175-198, Code/sag/network.py:30-53, train.py:121-129.
"""
import numpy as np
import pytest
import torch

from oracle import dense_ref as R
from oracle import pyg_ref as P

pytestmark = pytest.mark.gpu


class _A:
    bias = True


def _clone_params(model, dtype):
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in model.state_dict().items()}


class _OracleLoop:
    """the reference's training loop on the CPU oracle: loss -> backward -> clip_grad_norm_(clip) -> Adam.step() (train.py:121-129)"""

    def __init__(self, params, forward, lr, clip):
        self.p, self.forward, self.clip = params, forward, clip
        self.opt = torch.optim.Adam(list(params.values()), lr=lr)

    def step(self):
        self.opt.zero_grad()
        loss, logits = self.forward(self.p)
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_([v for v in self.p.values() if v.grad is not None], self.clip)
        self.opt.step()
        return float(loss.detach()), logits.detach().double(), float(norm)


def _run(model, loss_fn, forward32, forward64, lr, clip=2.0, steps=3, defer_loss=False, logit_scale=1.0, handful=8, tag="", pre_step=None,
         max_frac=0.02):
    """loss_fn(stash) builds the step the bench times (stash['logits'] = the head's output); forwardNN(p) -> (loss, logits) on
    the oracle with parameter dict p."""
    from two_stage_gnn_amd import message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    p32, p64 = _clone_params(model, torch.float32), _clone_params(model, torch.float64)
    init = {k: v.detach().clone().double() for k, v in p64.items()}
    trainer = FlatTrainer(model, lr=lr, clip=clip, defer_loss=defer_loss)
    stash = {}
    gs = GraphedStep(trainer, lambda: loss_fn(stash), warmup=3)
    assert gs.describe().startswith("one graph"), gs.describe()
    o32, o64 = _OracleLoop(p32, forward32, lr, clip), _OracleLoop(p64, forward64, lr, clip)
    names = [k for k, _ in model.named_parameters()]
    report = []
    for i in range(1, steps + 1):
        if pre_step is not None:
            pre_step(i, p64)                                        # (per-step inputs that depend on the oracle's parameters)
        gs.step()
        loss_hip = gs.loss_value()                                  # synchronises and checks the device's error word
        logits_hip = stash["logits"].detach().cpu().double()
        norm_hip = float(trainer.state[1])
        assert float(trainer.state[0]) == float(i) and float(trainer.state[3]) == 0.0
        l32, z32, n32 = o32.step()
        l64, z64, n64 = o64.step()
        # loss / gradient norm / logits
        assert abs(loss_hip - l64) <= max(10 * abs(l32 - l64), 1e-4 * max(1.0, abs(l64))), (tag, i, loss_hip, l32, l64)
        assert abs(norm_hip - n64) <= max(10 * abs(n32 - n64), 1e-3 * n64), (tag, i, norm_hip, n32, n64)
        zs = max(logit_scale, float(z64.abs().max()))
        e_hip, e_cpu = float((logits_hip - z64).abs().max()), float((z32.double() - z64).abs().max())
        assert e_hip <= max(10 * e_cpu, 1e-4 * zs), (tag, i, "logits", e_hip, e_cpu, zs)
        # parameters: movement since step 0
        u = lr * i
        worst = 0.0
        for k, p in model.named_parameters():
            hip = p.detach().cpu().double() - init[k]
            d32, d64 = p32[k].detach().double() - init[k], p64[k].detach() - init[k]
            a_hip, a_cpu = (hip - d64).abs(), (d32 - d64).abs()
            g_err, c_err = float(a_hip.max()), float(a_cpu.max())
            assert g_err <= max(10 * c_err, max_frac * u), (tag, i, k, g_err, c_err, u)
            n_hip, n_cpu = int((a_hip > 0.01 * u).sum()), int((a_cpu > 0.01 * u).sum())
            assert n_hip <= max(handful, 4 * n_cpu), (tag, i, k, n_hip, n_cpu, hip.numel())
            worst = max(worst, g_err / u)
        report.append((i, loss_hip, l32, l64, e_hip, e_cpu, worst))
    mp.check_device_errors()
    for r in report:
        print("%s step %d: loss hip %.7f cpu32 %.7f fp64 %.7f | logits err hip %.2e cpu32 %.2e | worst parameter error %.3f of lr*steps"
              % ((tag,) + r))
    assert names
    return report


def test_panel_units_batch_equals_plain_panel_batch():
    """rows beyond one 32-row panel per compute unit as 16- / 8-row units (csrc/rowgemm_body.h panel_split; the first layer's product, the
    fused forward launches, the merged backward launches) against plain panels on the SAME batches (two fresh batch objects of one seed,
    one of them with panel_units = False): a row's arithmetic does not depend on the block that owns it, so logits, loss and the
    input-side results are BITWISE equal; the weight gradients are sums over differently cut slabs (the slab count follows the panel
    blocks) and agree to rounding.  The two batches run interleaved in one process (forward, forward, backward, backward): the split
    travels with the batch, not with the order of the calls.  Batches of 271 (8-row units) and 288 panels (16-row units)."""
    from two_stage_gnn_amd import dense_encoders as E, synthetic, _native as nat
    dev = torch.device("cuda")

    class A:
        bias = True
    for seed, want_unit in ((3, 8), (6, 16)):
        hb = synthetic.host_batch(seed=seed, B=32, shape="DD", nmax=1000)
        g, x, label = synthetic.to_device(hb, dev)
        npan = -(-g.n_rows // 32)
        ncu = torch.cuda.get_device_properties(dev).multi_processor_count
        if not (ncu < npan <= ncu + ncu // 2):
            pytest.skip("this device hosts every panel of the batch at once")
        blocks = int(nat.lib().tsgnn_panel_blocks(int(g.n_rows), 1))
        assert blocks == (ncu & ~7) + -(-(g.n_rows - 32 * (ncu & ~7)) // want_unit), (blocks, npan)
        assert int(nat.lib().tsgnn_panel_blocks(int(g.n_rows), 0)) == npan
        runs = []
        for units in (True, False):
            torch.manual_seed(11)
            m = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").to(dev)
            g2, x2, _ = synthetic.to_device(hb, dev)              # (a fresh batch object: no cached launch plans)
            g2.panel_units = units
            runs.append({"m": m, "g": g2, "x": x2})
        prev = nat.trace
        try:
            for r in runs:                                        # forward of one batch, then of the other ...
                nat.trace = r["fwd"] = []
                r["logits"] = r["m"](r["x"], r["g"])[1]
                r["loss"] = r["m"].loss(r["logits"], label)
            for r in runs:                                        # ... then both backwards
                nat.trace = r["bwd"] = []
                r["loss"].backward()
                torch.cuda.synchronize()
        finally:
            nat.trace = prev
        for r, flag in zip(runs, ("true", "false")):
            fwd = [k for _, _, k in r["fwd"]]
            bwd = [k for _, _, k in r["bwd"]]
            assert "rowgemm_gather_st_kernel<%s>" % flag in fwd, fwd
            assert "sage_layer_bwd_kernel<true,%s>" % flag in bwd, bwd
        out = [(r["logits"].detach(), float(r["loss"].detach()), [p.grad.detach() for p in r["m"].parameters() if p.grad is not None])
               for r in runs]
        assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
        for a, b in zip(out[0][2], out[1][2]):
            torch.testing.assert_close(a, b, rtol=2e-5, atol=1e-7 * float(b.abs().max() + 1e-30) + 1e-9)


# ------------------------------------------------------------------------------------------------ GraphSage stack (bench.py)
@pytest.mark.parametrize("shape,B,nmax,layers,hid,seed", [
    ("DD", 32, 1000, 3, 128, 0),          # the headline batch: 8,151 rows = 255 row panels (bench.py, rank 0)
    ("DD", 32, 1000, 3, 128, 6),          # bench.py's rank 6: 9,191 rows = 288 row panels (more panels than compute units: 16-row units)
    ("DD", 32, 1000, 3, 128, 3),          # rank 3: 8,662 rows = 271 panels (a small overflow: 8-row units behind one panel per unit)
    ("PROTEINS", 64, 620, 3, 128, 1),     # BASELINE config 2 (scripts/config_bench.py)
    ("MUTAG", 32, 40, 2, 64, 0),          # BASELINE config 1
])
def test_sage_timed_step_vs_oracle(shape, B, nmax, layers, hid, seed):
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=seed, B=B, shape=shape, nmax=nmax)
    g, x, label = synthetic.to_device(hb, dev)
    fin = synthetic.SHAPES[shape][2]
    torch.manual_seed(1234)                                    # bench.py's seed
    model = E.GcnEncoderGraph(fin, hid, hid, 2, layers, bn=True, args=_A(), final_dim="number_classes").to(dev)
    xd, adj = synthetic.to_dense(hb)
    lab = torch.from_numpy(hb["label"])

    def fwd(dtype):
        xx, aa = xd.to(dtype), adj.to(dtype)

        def f(p):
            _, y = R.gcn_encoder(p, xx, aa, bn=True, final_dim="number_classes")
            return torch.nn.functional.cross_entropy(y, lab), y
        return f

    def loss_fn(stash):
        stash["logits"] = model(x, g)[1]
        return model.loss(stash["logits"], label)

    _run(model, loss_fn, fwd(torch.float32), fwd(torch.float64), lr=1e-3, defer_loss=True,
         tag="%s b%d seed %d (%d rows)" % (shape, B, seed, int(g.n_rows)))


# ------------------------------------------------------------------------------------------------ DiffPool (config 5)
def test_diffpool_timed_step_vs_oracle():
    """DD DiffPool 512 -> 64 -> 8, h = 64, batch 16 (scripts/config_bench.py cfg5; encoders.py:327-406)"""
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(4, 16, "DD", 512)
    g, x, label = synthetic.to_device(hb, dev)
    torch.manual_seed(0)
    model = E.SoftPoolingGcnEncoder(512, 89, 64, 64, 2, 3, 64, assign_ratio=0.125, num_pooling=2, bn=True, linkpred=False,
                                    args=_A(), assign_input_dim=89, final_dim="number_classes").to(dev)
    xd, adj = synthetic.to_dense(hb)
    lab = torch.from_numpy(hb["label"])
    sizes = hb["sizes"]

    def fwd(dtype):
        xx, aa = xd.to(dtype), adj.to(dtype)

        def f(p):
            _, y = R.diffpool_encoder(p, xx, aa, sizes, 2, assign_x=xx, final_dim="number_classes")
            return torch.nn.functional.cross_entropy(y, lab), y
        return f

    def loss_fn(stash):
        stash["logits"] = model(x, g, sizes, assign_x=x)[1]
        return model.loss(stash["logits"], label)

    _run(model, loss_fn, fwd(torch.float32), fwd(torch.float64), lr=5e-4, defer_loss=True, tag="DiffPool DD b16 Nmax 512")


# ------------------------------------------------------------------------------------------------ GAT (config 3)
def test_gat_timed_step_vs_oracle():
    """DD GAT 2 layers x 4 heads x 64, 32 graphs in ONE block-diagonal step with per-graph features at the reference's Nmax = 1000
    (scripts/config_bench.py cfg3 b32) = 32 reference forwards at B = 1 (encoders_GAT.py:175-198; train.py:480), mean loss."""
    from two_stage_gnn_amd import gat_encoders as G, synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(2, 32, "DD", 1000)
    xd, adj = synthetic.to_dense(hb)
    torch.manual_seed(0)
    model = G.DGATEncoderGraph(89, 64, 64, 2, None, num_layers=2, num_heads=[4, 4], final_dim="number_classes",
                               per_graph_features=True).to(dev)
    x, g = model.packed_batch(xd.to(dev), adj.to(dev), hb["sizes"])
    label = torch.from_numpy(hb["label"]).to(dev)
    lab = torch.from_numpy(hb["label"])
    B = len(hb["sizes"])

    def fwd(dtype):
        xx, aa = xd.to(dtype), adj.to(dtype)

        def f(p):
            ys = [R.gat_encoder(p, xx[b:b + 1], aa[b:b + 1], final_dim="number_classes")[1] for b in range(B)]
            y = torch.cat(ys)
            return torch.nn.functional.cross_entropy(y, lab), y                 # mean over the 32 B = 1 losses
        return f

    def loss_fn(stash):
        stash["logits"] = model(x, g)[1]
        return model.loss(stash["logits"], label)

    _run(model, loss_fn, fwd(torch.float32), fwd(torch.float64), lr=5e-4, defer_loss=True, tag="GAT DD b32 Nmax 1000")


# ------------------------------------------------------------------------------------------------ SAGPool (config 4)
def _imdb_batch(x_seed=None):
    """the batch scripts/config_bench.py times for config 4; x_seed None: its constant features, else 1 + 0.25 N(0,1)"""
    from two_stage_gnn_amd import synthetic
    hb = synthetic.host_batch(3, 128, "IMDB-BINARY", 136)
    sizes = hb["sizes"]
    n = int(sizes.sum())
    rp, col = hb["rowptr"][: n + 1], hb["col"]
    dst = np.repeat(np.arange(n), np.diff(rp))
    ei = torch.from_numpy(np.stack([col.astype(np.int64), dst.astype(np.int64)]))
    batch = torch.repeat_interleave(torch.arange(128), torch.from_numpy(sizes))
    if x_seed is None:
        x = torch.ones(n, 1)                                   # IMDB-B has no node features: what the bench feeds
    else:
        x = 1.0 + 0.25 * torch.randn(n, 1, generator=torch.Generator().manual_seed(x_seed))
    return hb, x, ei, batch, torch.from_numpy(hb["label"])


def _ambiguous_graphs(p, x, ei, batch, ratio, tol=1e-4):
    """fp64 oracle, level by level: the graphs whose top-k has no defined answer.  A graph is ambiguous at a level when
    scores within `tol` of the last kept score (relative to the graph's largest score; 1e-4 ~ ten times what fp32 rounding moves a
    pooled level's score, a 128-term dot product with cancellation) lie on BOTH sides of the cut — unless the tied nodes are true twins (equal
    feature rows and equal closed neighbourhoods, e.g. the nodes of a complete graph after a GCN layer): keeping one twin or the
    other is an automorphism of the graph, every readout and every parameter gradient is the same."""
    B = int(batch.max()) + 1
    bad = torch.zeros(B, dtype=torch.bool)
    for i in (1, 2, 3):
        x = torch.relu(P.gcn_conv(x, ei, p["conv%d.weight" % i], p["conv%d.bias" % i]))
        score = P.gcn_conv(x, ei, p["pool%d.score_layer.weight" % i], p["pool%d.score_layer.bias" % i]).squeeze(-1)
        n = x.size(0)
        A = torch.eye(n, dtype=torch.bool)                            # closed neighbourhoods
        A[ei[1], ei[0]] = True
        for b in range(B):
            idx = (batch == b).nonzero().view(-1)
            s = score[idx]
            k = int(np.ceil(np.float32(ratio) * np.float32(s.numel())))
            if k >= s.numel():
                continue
            order = torch.argsort(s, descending=True)
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.numel())
            near = (s - s[order[k - 1]]).abs() <= tol * (float(s.abs().max()) + 1e-30)
            if not (int(rank[near].min()) < k <= int(rank[near].max())):
                continue                                               # the tie group does not reach across the cut
            tied = idx[near]
            xs = x[tied]
            twins = (float((xs - xs[0]).abs().max()) <= 1e-9 * (float(xs.abs().max()) + 1e-30)) and bool((A[tied] == A[tied[0]]).all())
            if not twins:
                bad[b] = True
        x, ei, batch, _ = P.sag_pool(x, ei, batch, ratio, p["pool%d.score_layer.weight" % i], p["pool%d.score_layer.bias" % i])
    return bad


@pytest.mark.parametrize("x_mode", ["tie_free", "ones"])
def test_sagpool_timed_step_vs_oracle(x_mode):
    """IMDB-B SAGPool(0.5) h = 128, batch 128 (scripts/config_bench.py cfg4; Code/sag/network.py:30-53 with PyG's per-graph
    `batch`).  The oracle behind it (oracle/pyg_ref.py) is PARITY UNPINNED — torch_geometric is absent from the reference tree
    and from this image.  Dropout (network.py:50) is off: another implementation cannot reproduce torch's random stream.
    The workload is small DENSE graphs (20 nodes, 97 edges: many are complete): nodes tie in score, and a top-k cut between two
    tied nodes that are not twins has no defined answer (_ambiguous_graphs) — with 128 graphs x 3 levels about one graph
    per step is in that state by chance.  Graphs do not interact in this model (no batch statistics), so such a graph is taken out
    of the comparison individually:
      tie_free  node features 1 + 0.25 N(0,1).  Three optimiser steps of the WHOLE batch; before each step the graphs that are
                ambiguous for the fp64 oracle's current parameters get weight 0 in the loss (a device vector updated in place
                between replays; the same weights in the oracle), so they contribute nothing to the loss or to any gradient on
                either side; at least 96 of the 128 graphs must count in every step.  Everything compared.
      ones      the bench's own input (constant features): the forward is compared on the graphs whose top-k is defined in the
                fp64 oracle (they must be the large majority), per graph."""
    from two_stage_gnn_amd import sag_layers as S
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = S.Net(1, 128, 2, 0.5, 0.0, use_batch=True).to(dev).train()
    assert net._fused_ok()
    lr = 5e-4

    def fwd(x, ei, batch, lab, dtype):
        xx = x.to(dtype)

        def f(p):
            y = P.sag_net(p, xx, ei, 0.5, batch)
            return torch.nn.functional.nll_loss(y, lab), y
        return f

    class D:
        pass
    d = D()
    if x_mode == "ones":
        hb, x, ei, batch, lab = _imdb_batch(None)
        d.x, d.edge_index, d.batch = x.to(dev), ei.to(dev), batch.to(dev)
        p64 = _clone_params(net, torch.float64)
        with torch.no_grad():
            safe = ~_ambiguous_graphs(p64, x.double(), ei, batch, 0.5)
            ref = P.sag_net(p64, x.double(), ei, 0.5, batch)
            out = net(d).detach().cpu().double()
        print("IMDB-B b128, constant features: %d of 128 graphs have a defined top-k at every level" % int(safe.sum()))
        assert int(safe.sum()) >= 96
        torch.testing.assert_close(out[safe], ref[safe], rtol=1e-4, atol=1e-4)
        return

    hb, x, ei, batch, lab = _imdb_batch(5)
    d.x, d.edge_index, d.batch = x.to(dev), ei.to(dev), batch.to(dev)
    label = lab.to(dev)
    w_cpu = torch.ones(128, dtype=torch.float64)
    w_dev = torch.ones(128, dtype=torch.float32, device=dev)
    counted = []

    def weighted(dtype):
        xx = x.to(dtype)

        def f(p):
            y = P.sag_net(p, xx, ei, 0.5, batch)
            w = w_cpu.to(dtype)
            return -(y.gather(1, lab.view(-1, 1)).squeeze(1) * w).sum() / w.sum(), y * w.view(-1, 1)
        return f

    def loss_fn(stash):
        y = net(d)
        stash["logits"] = y * w_dev.view(-1, 1)                    # (masked graphs are not compared)
        return -(y.gather(1, label.view(-1, 1)).squeeze(1) * w_dev).sum() / w_dev.sum()

    def mask(i, p64):
        with torch.no_grad():
            bad = _ambiguous_graphs({k: v.detach() for k, v in p64.items()}, x.double(), ei, batch, 0.5)
        w_cpu.copy_((~bad).double())
        w_dev.copy_((~bad).float().to(dev))
        torch.cuda.synchronize()
        counted.append(int((~bad).sum()))
        assert counted[-1] >= 96, counted

    _run(net, loss_fn, weighted(torch.float32), weighted(torch.float64), lr=lr, tag="SAGPool IMDB-B b128 (tie-free features)", pre_step=mask)
    print("graphs counted per step:", counted)


# ------------------------------------------------------------------------------------------------ surface (B): PyG-named layers
class _Data:
    pass


@pytest.mark.parametrize("shape,B,layers,hid,seed", [
    ("DD", 32, 3, 128, 0),                # the headline shape on the PyG-named layers (8,151 rows = 255 row panels)
    ("DD", 32, 3, 128, 6),                # 9,191 rows = 288 row panels: more panels than compute units
    ("PROTEINS", 64, 3, 128, 1),          # BASELINE config 2 as worded: "PROTEINS SAGEConv 3-layer h=128 batch=64"
    ("MUTAG", 32, 2, 64, 0),              # BASELINE config 1 as worded: "MUTAG SAGEConv 2-layer h=64, batch=32"
])
def test_pyg_sage_timed_step_vs_oracle(shape, B, layers, hid, seed):
    """pyg.SageNet (SAGEConv layers as fused launches, pyg_sage.py / csrc/sageconv.hip) at the sizes scripts/config_bench.py times:
    three replayed optimiser steps against oracle/pyg_ref.sage_net + clip_grad_norm_ + Adam in fp32 and fp64.  PARITY UNPINNED: the
    oracle restates torch_geometric's documented SAGEConv (absent from the reference tree and from this image)."""
    from two_stage_gnn_amd import message_passing as mp, pyg, synthetic
    dev = torch.device("cuda")
    nmax = {"DD": 1000, "PROTEINS": 620, "MUTAG": 40}[shape]
    hb = synthetic.host_batch(seed=seed, B=B, shape=shape, nmax=nmax)
    d = _Data()
    d.x, d.edge_index, d.batch, label = synthetic.to_pyg(hb, dev)
    fin = synthetic.SHAPES[shape][2]
    torch.manual_seed(1234)
    net = pyg.SageNet(fin, hid, 2, num_layers=layers, dropout_ratio=0.0).to(dev).train()
    x_cpu = torch.from_numpy(hb["x"])
    ei, batch, lab = d.edge_index.cpu(), d.batch.cpu(), torch.from_numpy(hb["label"])

    def fwd(dtype):
        xx = x_cpu.to(dtype)

        def f(p):
            y = P.sage_net(p, xx, ei, batch, layers)
            return torch.nn.functional.nll_loss(y, lab), y
        return f

    def loss_fn(stash):
        stash["logits"] = net(d)
        return mp.nll_loss(stash["logits"], label)

    # max_frac: an entry whose gradient is below ~1e-8 (1e-6 of its tensor's largest) moves by lr * g / (|g| + eps) per Adam step, so a
    # gradient error at fp32 rounding level (1.5e-9 here, 3e-7 of the largest entry — scripts/dev/pyg_grad_check.py, on par with the
    # fp32 CPU run) is amplified by up to 1 / eps = 1e8: 0.0245 lr*steps was observed for ONE entry of one tensor (DD seed 6, step 2).
    # The count of entries further than 0.01 lr*steps stays bounded by `handful` as everywhere else.
    _run(net, loss_fn, fwd(torch.float32), fwd(torch.float64), lr=1e-3, defer_loss=True, max_frac=0.05,
         tag="PyG SAGEConv %s b%d %dL h%d seed %d (%d rows)" % (shape, B, layers, hid, seed, int(d.x.size(0))))


def test_pyg_gat_timed_step_vs_oracle():
    """BASELINE config 3 as worded — "DD GATConv 2-layer 4-head h=64 batch=32" — pyg.GatNet at the size scripts/pyg_bench.py times:
    three replayed optimiser steps against oracle/pyg_ref.gat_net + clip_grad_norm_ + Adam (fp32, fp64).  PARITY UNPINNED."""
    from two_stage_gnn_amd import message_passing as mp, pyg, synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=2, B=32, shape="DD", nmax=1000)
    d = _Data()
    d.x, d.edge_index, d.batch, label = synthetic.to_pyg(hb, dev)
    torch.manual_seed(0)
    net = pyg.GatNet(89, 64, 2, heads=4, num_layers=2).to(dev).train()
    x_cpu = torch.from_numpy(hb["x"])
    ei, batch, lab = d.edge_index.cpu(), d.batch.cpu(), torch.from_numpy(hb["label"])

    def fwd(dtype):
        xx = x_cpu.to(dtype)

        def f(p):
            y = P.gat_net(p, xx, ei, batch, 2, 4)
            return torch.nn.functional.nll_loss(y, lab), y
        return f

    def loss_fn(stash):
        logits = net.logits(d)
        stash["logits"] = torch.log_softmax(logits.detach(), dim=-1)           # (what net(d) returns; compared with the oracle's)
        return mp.cross_entropy(logits, label)

    _run(net, loss_fn, fwd(torch.float32), fwd(torch.float64), lr=5e-4, max_frac=0.05, defer_loss=True,
         tag="PyG GATConv DD b32 2L 4 heads h64")


def _ambiguous_graphs_sage(p, x, ei, batch, ratio, tol=1e-4):
    """_ambiguous_graphs for the SAGPool + SAGEConv network (conv = "sage"): the graphs whose top-k has no defined answer at some level"""
    B = int(batch.max()) + 1
    bad = torch.zeros(B, dtype=torch.bool)
    for i in (1, 2, 3):
        x = torch.relu(P.sage_conv(x, ei, p["conv%d.lin_l.weight" % i], p["conv%d.lin_l.bias" % i], p["conv%d.lin_r.weight" % i]))
        score = P.gcn_conv(x, ei, p["pool%d.score_layer.weight" % i], p["pool%d.score_layer.bias" % i]).squeeze(-1)
        n = x.size(0)
        A = torch.eye(n, dtype=torch.bool)
        A[ei[1], ei[0]] = True
        for b in range(B):
            idx = (batch == b).nonzero().view(-1)
            s = score[idx]
            k = int(np.ceil(np.float32(ratio) * np.float32(s.numel())))
            if k >= s.numel():
                continue
            order = torch.argsort(s, descending=True)
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.numel())
            near = (s - s[order[k - 1]]).abs() <= tol * (float(s.abs().max()) + 1e-30)
            if not (int(rank[near].min()) < k <= int(rank[near].max())):
                continue
            tied = idx[near]
            xs = x[tied]
            twins = (float((xs - xs[0]).abs().max()) <= 1e-9 * (float(xs.abs().max()) + 1e-30)) and bool((A[tied] == A[tied[0]]).all())
            if not twins:
                bad[b] = True
        x, ei, batch, _ = P.sag_pool(x, ei, batch, ratio, p["pool%d.score_layer.weight" % i], p["pool%d.score_layer.bias" % i])
    return bad


def test_sagpool_sage_timed_step_vs_oracle():
    """BASELINE config 4 as worded, literally — "IMDB-BINARY SAGPool (ratio 0.5) + SAGEConv h=128 batch=128": the reference's network
    (Code/sag/network.py) with its conv layers replaced by SAGEConv and its OWN SAGPool layers, as ONE sync-free node replayed from a hipGraph
    (sag_layers.Net(conv="sage"), sag_stack_sage.py).  Three optimiser steps against oracle/pyg_ref.sag_net(conv="sage") + Adam (fp32, fp64);
    graphs whose top-k is ambiguous for the fp64 oracle's current parameters get weight 0 on both sides (as in
    test_sagpool_timed_step_vs_oracle); at least 80 of 128 must count (93-103 do: IMDB-B's one input feature and the
    mean aggregation leave more near-ties at the k-th score than the GCN network's 96+).  SAGEConv half: PARITY UNPINNED."""
    from two_stage_gnn_amd import sag_layers as S
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = S.Net(1, 128, 2, 0.5, 0.0, use_batch=True, conv="sage").to(dev).train()
    assert net._fused_ok()
    hb, x, ei, batch, lab = _imdb_batch(5)
    d = _Data()
    d.x, d.edge_index, d.batch = x.to(dev), ei.to(dev), batch.to(dev)
    label = lab.to(dev)
    w_cpu = torch.ones(128, dtype=torch.float64)
    w_dev = torch.ones(128, dtype=torch.float32, device=dev)
    counted = []

    def weighted(dtype):
        xx = x.to(dtype)

        def f(p):
            y = P.sag_net(p, xx, ei, 0.5, batch, conv="sage")
            w = w_cpu.to(dtype)
            return -(y.gather(1, lab.view(-1, 1)).squeeze(1) * w).sum() / w.sum(), y * w.view(-1, 1)
        return f

    def loss_fn(stash):
        y = net(d)
        stash["logits"] = y * w_dev.view(-1, 1)
        return -(y.gather(1, label.view(-1, 1)).squeeze(1) * w_dev).sum() / w_dev.sum()

    def mask(i, p64):
        with torch.no_grad():
            bad = _ambiguous_graphs_sage({k: v.detach() for k, v in p64.items()}, x.double(), ei, batch, 0.5)
        w_cpu.copy_((~bad).double())
        w_dev.copy_((~bad).float().to(dev))
        torch.cuda.synchronize()
        counted.append(int((~bad).sum()))
        assert counted[-1] >= 80, counted

    _run(net, loss_fn, weighted(torch.float32), weighted(torch.float64), lr=5e-4, max_frac=0.05,
         tag="SAGPool + SAGEConv IMDB-B b128 (tie-free features)", pre_step=mask)
    print("graphs counted per step:", counted)


def test_pyg_dense_diff_pool_config5_size_vs_oracle():
    """pyg.dense_diff_pool at BASELINE config 5's first pooling level (16 graphs, Nmax 512 -> 64 clusters, h = 64; DD-shaped adjacency,
    ragged sizes through the mask) against oracle/pyg_ref.dense_diff_pool in fp32 and fp64: the four outputs, and the gradients of EACH
    of them alone with respect to x and the assignment logits (the link loss here is the closed form ||A||^2 - 2 tr(S^T A S) + ||S^T S||^2
    — no [B, N, N] product — and the entropy term comes out of the softmax launch: their gradients are the new code).  PARITY UNPINNED."""
    from two_stage_gnn_amd import pyg, synthetic
    B, N, K, Fd = 16, 512, 64, 64
    hb = synthetic.host_batch(seed=2, B=B, shape="DD", nmax=N)
    _, adj = synthetic.to_dense(hb)
    sizes = torch.from_numpy(np.asarray(hb["sizes"]))
    mask = torch.arange(N)[None, :] < sizes[:, None]
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, N, Fd, generator=g)
    s = torch.randn(B, N, K, generator=g)
    wo = [torch.randn(B, K, Fd, generator=g), torch.randn(B, K, K, generator=g)]

    def oracle(dtype):
        xr, sr = x.to(dtype).requires_grad_(True), s.to(dtype).requires_grad_(True)
        o = P.dense_diff_pool(xr, adj.to(dtype), sr, mask)
        losses = [(o[0] * wo[0].to(dtype)).sum(), (o[1] * wo[1].to(dtype)).sum(), o[2], o[3]]
        return o, [torch.autograd.grad(l, [xr, sr], retain_graph=True, allow_unused=True) for l in losses]

    o32, g32 = oracle(torch.float32)
    o64, g64 = oracle(torch.float64)
    xg, sg = x.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
    o = pyg.dense_diff_pool(xg, adj.cuda(), sg, mask.cuda())
    from test_gpu_pyg_fused import assert_arbitrated
    for name, a, b, c in zip(("out", "out_adj", "link", "ent"), o, o32, o64):
        assert_arbitrated(a, b, c, name)
    print("link loss hip %.9g cpu32 %.9g fp64 %.9g | entropy hip %.9g cpu32 %.9g fp64 %.9g"
          % (float(o[2]), float(o32[2]), float(o64[2]), float(o[3]), float(o32[3]), float(o64[3])))
    losses = [(o[0] * wo[0].cuda()).sum(), (o[1] * wo[1].cuda()).sum(), o[2], o[3]]
    for li, (name, l) in enumerate(zip(("out", "out_adj", "link", "ent"), losses)):
        got = torch.autograd.grad(l, [xg, sg], retain_graph=True, allow_unused=True)
        for vn, a, b, c in zip(("dx", "dlogits"), got, g32[li], g64[li]):
            if c is None:
                assert a is None or float(a.abs().max()) == 0.0, (name, vn)
                continue
            assert_arbitrated(a, b, c, "%s of %s" % (vn, name), handful=16)


def test_pyg_sagpool_sage_config4_vs_oracle():
    """BASELINE config 4 as worded — "IMDB-BINARY SAGPool (ratio 0.5) + SAGEConv h=128 batch=128" — pyg.SagePoolNet (fused SAGEConv
    launches + PyG SAGPooling with its GraphConv scorer) at full size against oracle/pyg_ref.sage_pool_net in fp64: log-probabilities
    and every parameter gradient of a weighted nll.  Small dense graphs tie in score: a graph whose kept node sets differ
    between the two sides at any level (a tie at the cut resolved differently) gets weight 0 on BOTH sides — graphs do not interact in
    this model — and at least 96 of the 128 graphs must count.  PARITY UNPINNED (no torch_geometric in the reference tree / image)."""
    from two_stage_gnn_amd import pyg
    dev = torch.device("cuda")
    hb, x, ei, batch, lab = _imdb_batch(5)
    torch.manual_seed(0)
    net = pyg.SagePoolNet(1, 128, 2, pooling_ratio=0.5).to(dev).eval()
    d = _Data()
    d.x, d.edge_index, d.batch = x.to(dev), ei.to(dev), batch.to(dev)
    y = net(d)
    p64 = _clone_params(net, torch.float64)
    y64, perms64 = P.sage_pool_net(p64, x.double(), ei, batch, 0.5, return_perms=True)
    # per graph: the same kept nodes at every level?  (perm indexes the level's own rows; compare as sets of positions per graph)
    ok = torch.ones(128, dtype=torch.bool)
    b_hip = b_ref = batch
    for ph, pr in zip(net.last_perms, perms64):
        ph = ph.cpu()
        for b in range(128):
            sh = set(ph[b_hip[ph] == b].tolist()); sr = set(pr[b_ref[pr] == b].tolist())
            if sh != sr:
                ok[b] = False
        b_hip, b_ref = b_hip[ph], b_ref[pr]
    print("config 4 as worded: %d of 128 graphs keep the same nodes at every level on both sides" % int(ok.sum()))
    assert int(ok.sum()) >= 96
    torch.testing.assert_close(y.detach().cpu().double()[ok], y64.detach()[ok], rtol=1e-4, atol=1e-4)
    w = ok.double()
    loss64 = -(y64.gather(1, lab.view(-1, 1)).squeeze(1) * w).sum() / w.sum()
    names = [k for k, _ in net.named_parameters()]
    g64 = torch.autograd.grad(loss64, [p64[k] for k in names], allow_unused=True)
    wd = w.float().to(dev)
    loss = -(y.gather(1, lab.to(dev).view(-1, 1)).squeeze(1) * wd).sum() / wd.sum()
    gh = torch.autograd.grad(loss, [p for _, p in net.named_parameters()], allow_unused=True)
    for k, a, c in zip(names, gh, g64):
        if c is None:
            continue
        scale = float(c.abs().max()) + 1e-30
        err = float((a.cpu().double() - c).abs().max())
        assert err <= 2e-4 * scale + 1e-7, (k, err, scale)


# ------------------------------------------------------------------------------------------------ long trajectories
TRAJ_STEPS = int(__import__("os").environ.get("TSGNN_TRAJ_STEPS", "100"))


def _trajectory(model, loss_fn, forward32, forward64, lr, steps=None, every=20, clip=2.0, tag=""):
    """`steps` replayed optimiser steps against the oracle loop in fp32 and fp64; the loss is compared every `every` steps within
    max(10 |cpu32 - fp64|, 1e-3): a defect that shows once per N steps (a step counter that runs ahead, an accumulator that is not
    re-armed, a workspace left dirty) moves a trajectory long before it moves three steps.  100 steps by default (the
    two CPU oracle loops cost ~1.4 s per step); TSGNN_TRAJ_STEPS=200 is the run recorded in profiles/r04/trajectories.txt."""
    steps = TRAJ_STEPS if steps is None else steps
    from two_stage_gnn_amd import message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    p32, p64 = _clone_params(model, torch.float32), _clone_params(model, torch.float64)
    trainer = FlatTrainer(model, lr=lr, clip=clip, defer_loss=True)
    gs = GraphedStep(trainer, loss_fn, warmup=3)
    o32, o64 = _OracleLoop(p32, forward32, lr, clip), _OracleLoop(p64, forward64, lr, clip)
    rows = []
    for i in range(1, steps + 1):
        gs.step()
        l32 = o32.step()[0]
        l64 = o64.step()[0]
        if i % every == 0 or i == 1:
            lh = gs.loss_value()                                     # (synchronises, checks the device's error word)
            assert float(trainer.state[0]) == float(i) and float(trainer.state[3]) == 0.0
            rows.append((i, lh, l32, l64))
            print("%s step %3d: loss hip %.6f cpu32 %.6f fp64 %.6f" % (tag, i, lh, l32, l64), flush=True)
            assert abs(lh - l64) <= max(10 * abs(l32 - l64), 1e-3), (tag, i, lh, l32, l64)
    mp.check_device_errors()
    assert rows[-1][3] < rows[0][3]                                   # (and the model did learn something on its one batch)


def test_sage_long_trajectory_vs_oracle():
    """200 optimiser steps of the headline step (DD b32, 3 layers h = 128, Nmax 1000) replayed from its hipGraph"""
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=0, B=32, shape="DD", nmax=1000)
    g, x, label = synthetic.to_device(hb, dev)
    torch.manual_seed(1234)
    model = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=_A(), final_dim="number_classes").to(dev)
    xd, adj = synthetic.to_dense(hb)
    lab = torch.from_numpy(hb["label"])
    # the oracle's aggregation as a sparse product over the block-diagonal adjacency (the same arithmetic as adj @ x on the padded
    # rows: absent entries are exact zeros), so that 2 x 200 CPU steps fit the test budget
    B, N = adj.size(0), adj.size(1)
    bi, ri, ci = adj.nonzero(as_tuple=True)

    def fwd(dtype):
        xx = xd.to(dtype)
        asp = torch.sparse_coo_tensor(torch.stack([bi * N + ri, bi * N + ci]), adj[bi, ri, ci].to(dtype), (B * N, B * N)).coalesce()

        def f(p):
            _, y = R.gcn_encoder(p, xx, asp, bn=True, final_dim="number_classes")
            return torch.nn.functional.cross_entropy(y, lab), y
        return f

    _trajectory(model, lambda: model.loss(model(x, g)[1], label), fwd(torch.float32), fwd(torch.float64), lr=1e-3, tag="SAGE DD b32")


def test_diffpool_long_trajectory_vs_oracle():
    """200 optimiser steps of the DiffPool step (DD b16, Nmax 512 -> 64 -> 8, h = 64): the step whose Adam counter once ran ahead"""
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(4, 16, "DD", 512)
    g, x, label = synthetic.to_device(hb, dev)
    torch.manual_seed(0)
    model = E.SoftPoolingGcnEncoder(512, 89, 64, 64, 2, 3, 64, assign_ratio=0.125, num_pooling=2, bn=True, linkpred=False,
                                    args=_A(), assign_input_dim=89, final_dim="number_classes").to(dev)
    xd, adj = synthetic.to_dense(hb)
    lab = torch.from_numpy(hb["label"])
    sizes = hb["sizes"]

    def fwd(dtype):
        xx, aa = xd.to(dtype), adj.to(dtype)

        def f(p):
            _, y = R.diffpool_encoder(p, xx, aa, sizes, 2, assign_x=xx, final_dim="number_classes")
            return torch.nn.functional.cross_entropy(y, lab), y
        return f

    _trajectory(model, lambda: model.loss(model(x, g, sizes, assign_x=x)[1], label), fwd(torch.float32), fwd(torch.float64), lr=5e-4,
                tag="DiffPool DD b16")


# ------------------------------------------------------------------------------------------------ failure path of the barriers
def test_barrier_timeout_poisons_the_optimiser_and_raises():
    """A bounded device-wide barrier that cannot complete (dense_stack.hip; forced with the library's self-test hook: one workgroup
    waits for two arrivals) must (a) raise the device's error word, (b) make the optimiser skip its update while the word is set,
    (c) raise on the host at the next synchronisation point, and (d) leave everything usable afterwards (ADVICE r2 / VERDICT r2 #13)."""
    from two_stage_gnn_amd import _native as nat, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    dev = torch.device("cuda")
    assert nat.lib().tsgnn_dense_stack_max_resident() >= torch.cuda.get_device_properties(0).multi_processor_count
    lin = torch.nn.Linear(64, 8).to(dev)
    tr = FlatTrainer(lin, lr=1e-2, clip=2.0)
    xin = torch.randn(16, 64, device=dev)

    def one():
        return tr.step(lambda: lin(xin).square().mean())

    one(); tr.check()
    before = tr.flat_param.clone()
    words = torch.zeros(32 + 256, dtype=torch.int32, device=dev)
    mp.register_barrier_words(dev, words)
    err = mp.device_error_word(dev)
    nat.call("dense_stack_barrier_selftest", words, err, 1)              # completes
    torch.cuda.synchronize()
    assert float(err) == 0.0 and int(words.abs().sum()) == 0
    nat.call("dense_stack_barrier_selftest", words, err, 2)              # can never complete: gives up at its bound
    one(); one()                                                         # enqueued behind it: must NOT touch the parameters
    torch.cuda.synchronize()
    assert float(err) == 1.0
    assert torch.equal(tr.flat_param, before) and float(tr.state[3]) == 1.0 and float(tr.state[0]) == 1.0
    with pytest.raises(RuntimeError, match="barrier timed out"):
        tr.check()
    assert float(err) == 0.0 and int(words.abs().sum()) == 0 and float(tr.state[3]) == 0.0      # cleared, barrier words re-armed
    one(); tr.check()                                                    # and the next step is applied again
    assert not torch.equal(tr.flat_param, before) and float(tr.state[0]) == 2.0
    # self-clearing workspaces (a completed launch leaves them zero, an aborted one may not) are re-zeroed by the same path
    ws = mp.register_clear_on_error(torch.ones(16, dtype=torch.int64, device=dev))
    nat.call("dense_stack_barrier_selftest", words, err, 2)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="barrier timed out"):
        tr.check()
    assert int(ws.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ bitwise repeatability
@pytest.mark.parametrize("seed", [0, 6])
def test_timed_step_is_bitwise_repeatable(seed):
    """The benched step run five times from the same state gives the same bits (loss, every gradient, every parameter): the slot
    batch-norm statistics are accumulated with 64-bit INTEGER atomics (order-independent), the max readout with packed atomicMax,
    the weight gradients as slabs summed in fixed order — no float atomics anywhere on the path."""
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=seed, B=32, shape="DD", nmax=1000)
    g, x, label = synthetic.to_device(hb, dev)
    torch.manual_seed(1234)
    model = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=_A(), final_dim="number_classes").to(dev)
    tr = FlatTrainer(model, lr=1e-3, clip=2.0, defer_loss=True)
    gs = GraphedStep(tr, lambda: model.loss(model(x, g)[1], label), warmup=3)
    snap = [t.clone() for t in (tr.flat_param, tr.exp_avg, tr.exp_avg_sq, tr.state)]
    runs = []
    for _ in range(5):
        for t, s_ in zip((tr.flat_param, tr.exp_avg, tr.exp_avg_sq, tr.state), snap):
            t.copy_(s_)
        gs.step(); gs.step()                                        # two steps: the second starts from accumulators the first one cleared
        loss = gs.loss_value()
        runs.append((loss, tr.flat_grad.clone(), tr.flat_param.clone()))
    for loss, grad, param in runs[1:]:
        assert loss == runs[0][0]
        assert torch.equal(grad, runs[0][1]) and torch.equal(param, runs[0][2])
