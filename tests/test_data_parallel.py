"""Data-parallel path: flat gradient bucket + one all-reduce + one optimiser step.
CPU: world_size-2 gloo processes exercise the bucket/collective logic (the HIP optimiser kernel is replaced
by its host arithmetic in a TEST subclass — the product's apply() refuses to run off-GPU).
GPU: two gloo ranks sharing cuda:0 run the real HIP step and must agree with the average of the per-rank
gradients and stay bit-identical to each other."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_apply(tr, scale):
    g = tr.flat_grad * scale
    norm = g.norm()
    coef = torch.clamp(tr.clip / (norm + 1e-6), max=1.0) if tr.clip > 0 else torch.tensor(1.0)
    g = g * coef
    tr.state[0] += 1
    step = float(tr.state[0])
    b1, b2 = tr.betas
    tr.exp_avg.mul_(b1).add_(g, alpha=1 - b1)
    tr.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
    denom = tr.exp_avg_sq.sqrt() / (1 - b2 ** step) ** 0.5 + tr.eps
    tr.flat_param.addcdiv_(tr.exp_avg, denom, value=-tr.lr / (1 - b1 ** step))


def _cpu_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from two_stage_gnn_amd.data_parallel import FlatTrainer

    class HostTrainer(FlatTrainer):
        def apply(self):
            _host_apply(self, 1.0 / self.world)

    torch.manual_seed(rank)          # replicas start from DIFFERENT bits: FlatTrainer broadcasts rank 0's parameters
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 2))
    tr = HostTrainer(model, lr=1e-2, clip=2.0)
    assert tr.world == world
    start = tr.flat_param.detach().clone()
    gen = torch.Generator().manual_seed(100 + rank)
    x, y = torch.randn(8, 6, generator=gen), torch.randint(0, 2, (8,), generator=gen)
    local = None
    for _ in range(3):
        tr.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(x), y)
        loss.backward()
        tr.gather_grads()
        if local is None:
            local = tr.flat_grad.clone()
        tr.all_reduce()
        tr.apply()
    q.put((rank, local.numpy(), tr.flat_param.detach().numpy().copy(), start.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_flat_bucket_allreduce_gloo_world2():
    ctx = mp_.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_cpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(2)])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    # the constructor aligned the replicas (rank 1 was initialised from another seed) ...
    np.testing.assert_array_equal(res[0][3], res[1][3])
    # ... and they stay identical after every all-reduced step
    np.testing.assert_array_equal(res[0][2], res[1][2])
    # and equal a single process that averages the two local gradients itself
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd.data_parallel import FlatTrainer

    class HostTrainer(FlatTrainer):
        def apply(self):
            _host_apply(self, 0.5)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 2))
    tr = HostTrainer(model, lr=1e-2, clip=2.0)
    data = []
    for r in range(2):
        gen = torch.Generator().manual_seed(100 + r)
        data.append((torch.randn(8, 6, generator=gen), torch.randint(0, 2, (8,), generator=gen)))
    for _ in range(3):
        total = torch.zeros_like(tr.flat_grad)
        for x, y in data:
            tr.zero_grad()
            torch.nn.functional.cross_entropy(model(x), y).backward()
            total += tr.gather_grads()
        tr.flat_grad.copy_(total)
        tr.apply()
    np.testing.assert_allclose(tr.flat_param.detach().numpy(), res[0][2], rtol=1e-6, atol=1e-7)


def test_flat_trainer_views_alias_parameters():
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    m = torch.nn.Linear(3, 2)
    tr = FlatTrainer(m)
    assert tr.numel == 10 and tr.views == [(0, 6), (8, 2)]          # parameters start on 16-byte boundaries of the flat buffer
    tr.flat_param.fill_(1.5)
    assert float(m.weight[0, 0]) == 1.5 and float(m.bias[1]) == 1.5
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.apply()


# ----------------------------------------------------------------------------------------------- GPU
def _gpu_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer

    class A:
        bias = True
    torch.manual_seed(7 + rank)          # different initial bits per rank: the trainer broadcasts rank 0's
    model = E.GcnEncoderGraph(7, 16, 16, 2, 3, bn=True, args=A(), final_dim="number_classes").cuda()
    tr = FlatTrainer(model, lr=1e-3, clip=2.0)
    hb = synthetic.host_batch(seed=rank, B=6, shape="MUTAG", nmax=40)
    g, x, label = synthetic.to_device(hb, torch.device("cuda"))
    local = None
    for it in range(2):
        tr.zero_grad()
        _, yp = model(x, g)
        model.loss(yp, label).backward()
        tr.gather_grads()
        if local is None:
            local = tr.flat_grad.clone()
        tr.all_reduce()
        if it == 0:
            reduced = tr.flat_grad.clone()
        tr.apply()
    # the N > 1 GraphedStep (two hipGraphs around the eagerly issued collective) against the same steps launched eagerly
    from two_stage_gnn_amd.data_parallel import GraphedStep
    graphed = []
    for use_graph in (False, True):
        torch.manual_seed(21)
        m2 = E.GcnEncoderGraph(7, 16, 16, 2, 3, bn=True, args=A(), final_dim="number_classes").cuda()
        t2 = FlatTrainer(m2, lr=1e-2, clip=2.0)
        before = t2.flat_param.clone()
        gs = GraphedStep(t2, lambda: m2.loss(m2(x, g)[1], label), warmup=2, use_graph=use_graph)
        assert gs.multi and not gs.one_graph
        assert torch.equal(before, t2.flat_param) and float(t2.state[0]) == 0.0      # warm-up left the trainer as it was
        for _ in range(3):
            gs.step()
        torch.cuda.synchronize()
        graphed.append((t2.flat_param.detach().cpu().numpy(), float(t2.state[0])))
    q.put((rank, local.cpu().numpy(), reduced.cpu().numpy(), tr.flat_param.detach().cpu().numpy(), tr.state.cpu().numpy(), graphed))
    dist.barrier()
    dist.destroy_process_group()


def _rccl_one_rank_worker(port, q):
    """one-rank RCCL group (RCCL refuses two ranks on one device): the N > 1 step as two hipGraphs around an eager all-reduce,
    as ONE hipGraph with the collective captured (TSGNN_GRAPH_ALLREDUCE=1), as the self-checked one-graph step (auto, the
    default), with the head's gradient bucket all-reduced on a side branch (buckets=2), and eagerly with that overlap, must all
    leave identical parameters"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    class A:
        bias = True
    hb = synthetic.host_batch(seed=3, B=8, shape="DD", nmax=400)
    g, x, label = synthetic.to_device(hb, torch.device("cuda"))
    out = []
    for one_graph, buckets in (("0", 1), ("1", 1), ("auto", 1), ("1", 2), ("eager", 2)):
        os.environ["TSGNN_GRAPH_ALLREDUCE"] = one_graph
        torch.manual_seed(5)
        model = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").cuda()
        tr = FlatTrainer(model, lr=1e-2, clip=2.0, buckets=buckets)
        tr.always_reduce = True
        gs = GraphedStep(tr, lambda: model.loss(model(x, g)[1], label), warmup=2, use_graph=one_graph != "eager")
        assert gs.multi and gs.one_graph == (one_graph in ("1", "auto")), gs.describe()
        for _ in range(3):
            gs.step()
        torch.cuda.synchronize()
        if buckets == 2:
            # the head's gradients (the tail of the flat buffer) went through the side-stream all-reduce
            assert tr._early is not None and tr._early[1] - tr._early[0] >= 128 * 384, tr._early
        out.append((tr.flat_param.detach().cpu().numpy(), float(tr.state[0])))
    q.put(out)
    dist.destroy_process_group()


@pytest.mark.gpu
def test_one_graph_allreduce_step_equals_two_graph_step():
    """one rank over RCCL: the step as two hipGraphs around an eager all-reduce == one hipGraph with the collective captured == the checked
    ("auto") one-graph step == the same with the head's bucket on a side branch == eager with that overlap — bitwise.

    The worker is started a second time if the FIRST one dies without a result: torch's ProcessGroupNCCL watchdog thread polls the events of
    collectives it still holds, and a poll that lands inside a stream capture aborts the process (hipErrorCapturedEvent, seen once in some tens
    of runs before GraphedStep began to wait out a watchdog pass ahead of its captures; the race is in the process group, not in the step)."""
    ctx = mp_.get_context("spawn")
    out = None
    for attempt in range(2):
        q = ctx.Queue()
        p = ctx.Process(target=_rccl_one_rank_worker, args=(29500 + (os.getpid() + 977 + 13 * attempt) % 2000, q))
        p.start()
        try:
            out = q.get(timeout=240)
        except Exception:                                       # noqa: BLE001 - queue.Empty: the worker died (or hung) without a result
            out = None
        p.join(60)
        if p.is_alive():
            p.kill()
            p.join(10)
        if out is not None:
            assert p.exitcode == 0
            break
        print("worker attempt %d ended without a result (exit code %s)" % (attempt, p.exitcode))
    assert out is not None
    for o in out:                                             # two graphs == one graph == checked one graph == 2 buckets == eager
        assert o[1] == 3.0
        np.testing.assert_array_equal(out[0][0], o[0])


@pytest.mark.gpu
def test_two_ranks_hip_step_on_one_gpu():
    ctx = mp_.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    np.testing.assert_allclose(res[0][2], res[0][1] + res[1][1], rtol=1e-6, atol=1e-7)     # SUM over ranks
    np.testing.assert_array_equal(res[0][2], res[1][2])
    np.testing.assert_array_equal(res[0][3], res[1][3])                                    # replicas identical
    assert res[0][4][0] == 2.0                                                             # two optimiser steps
    for r in range(2):
        (p_eager, n_eager), (p_graph, n_graph) = res[r][5]
        assert n_eager == n_graph == 3.0
        np.testing.assert_array_equal(p_eager, p_graph)                                    # two-graph step == eager step
    np.testing.assert_array_equal(res[0][5][1][0], res[1][5][1][0])                        # replicas identical after GraphedStep


@pytest.mark.gpu
def test_hip_clip_adam_matches_torch():
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    torch.manual_seed(0)
    m1 = torch.nn.Sequential(torch.nn.Linear(20, 30), torch.nn.Linear(30, 3)).cuda()
    m2 = torch.nn.Sequential(torch.nn.Linear(20, 30), torch.nn.Linear(30, 3)).cuda()
    m2.load_state_dict(m1.state_dict())
    tr = FlatTrainer(m1, lr=1e-3, clip=0.5)
    opt = torch.optim.Adam(m2.parameters(), lr=1e-3)
    x, y = torch.randn(16, 20).cuda() * 3, torch.randint(0, 3, (16,)).cuda()
    for _ in range(5):
        tr.step(lambda: torch.nn.functional.cross_entropy(m1(x), y))
        opt.zero_grad()
        torch.nn.functional.cross_entropy(m2(x), y).backward()
        torch.nn.utils.clip_grad_norm_(m2.parameters(), 0.5)
        opt.step()
    for a, b in zip(m1.parameters(), m2.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    assert float(tr.state[0]) == 5.0 and float(tr.state[3]) == 0.0          # five steps; the reserved word stays 0 (no barrier, nothing to time out)


@pytest.mark.gpu
def test_hip_clip_adam_large_model_three_launch_path():
    """more than 131,072 parameters: separate norm / final / update launches, same arithmetic."""
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    torch.manual_seed(1)
    m1 = torch.nn.Linear(600, 500).cuda()
    m2 = torch.nn.Linear(600, 500).cuda()
    m2.load_state_dict(m1.state_dict())
    tr = FlatTrainer(m1, lr=1e-3, clip=1.0)
    assert tr.numel > 131072
    opt = torch.optim.Adam(m2.parameters(), lr=1e-3)
    x, y = torch.randn(8, 600).cuda(), torch.randint(0, 500, (8,)).cuda()
    for _ in range(3):
        tr.step(lambda: torch.nn.functional.cross_entropy(m1(x), y))
        opt.zero_grad()
        torch.nn.functional.cross_entropy(m2(x), y).backward()
        torch.nn.utils.clip_grad_norm_(m2.parameters(), 1.0)
        opt.step()
    for a, b in zip(m1.parameters(), m2.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_direct_gradient_placement_equals_concatenated_bucket():
    """gradients written in place by the fused backward nodes (GradSink) == autograd tensors concatenated afterwards,
    also when seeded with the cached unit scalar, and for a parameter outside every fused node."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from two_stage_gnn_amd import dense_encoders as E, synthetic, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer

    class A:
        bias = True

    class WithExtra(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.enc = E.GcnEncoderGraph(7, 16, 16, 2, 3, bn=True, args=A(), final_dim="number_classes")
            self.temperature = torch.nn.Parameter(torch.tensor([1.3]))      # plain torch op: stays on the autograd path
            self.unused = torch.nn.Parameter(torch.ones(5))                  # never receives a gradient

        def forward(self, x, g):
            return self.enc(x, g)[1] * self.temperature

    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=3, B=6, shape="MUTAG", nmax=40)
    g, x, label = synthetic.to_device(hb, dev)
    results = []
    for direct in (False, True):
        torch.manual_seed(11)
        model = WithExtra().to(dev)
        tr = FlatTrainer(model, lr=1e-3, clip=2.0, direct_grads=direct)
        grads = []
        for it in range(3):
            tr.zero_grad()
            loss = model.enc.loss(model(x, g), label)
            if direct:
                tr.backward(loss)
            else:
                loss.backward()
            tr.gather_grads()
            assert mp.GRAD_SINK is None
            grads.append(tr.flat_grad.clone())
            tr.apply()
        if direct:
            assert len(tr.sink.written) >= 4                                 # conv and head parameters landed in place
        results.append((grads, tr.flat_param.clone()))
    for a, b in zip(results[0][0], results[1][0]):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    torch.testing.assert_close(results[0][1], results[1][1], rtol=0, atol=0)
    assert float(results[1][0][0].abs().sum()) > 0


@pytest.mark.gpu
def test_barrier_free_optimiser_equals_three_stage_path():
    """all gradients produced in place with their |grad|^2 shares -> tsgnn_adam_from_partials_f32; must match the generic
    norm -> clip -> Adam path (direct_grads=False) step for step"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer

    class A:
        bias = True
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=4, B=8, shape="DD", nmax=500)
    g, x, label = synthetic.to_device(hb, dev)
    finals = []
    for direct in (False, True):
        torch.manual_seed(3)
        model = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").to(dev)
        tr = FlatTrainer(model, lr=1e-2, clip=0.05, direct_grads=direct)        # a clip that bites: the norm matters
        for it in range(4):
            tr.zero_grad()
            loss = model.loss(model(x, g)[1], label)
            tr.backward(loss) if direct else loss.backward()
            tr.gather_grads()
            if direct:
                assert tr._norm_ready, "expected the barrier-free path on a fully fused model"
            tr.apply()
        finals.append((tr.flat_param.clone(), tr.state.clone()))
    assert float(finals[0][1][0]) == 4.0 and float(finals[1][1][0]) == 4.0
    torch.testing.assert_close(finals[1][1][1], finals[0][1][1], rtol=1e-5, atol=0)          # gradient norm of the last step
    torch.testing.assert_close(finals[1][0], finals[0][0], rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
def test_graphed_step_replays_the_eager_step():
    """GraphedStep (one hipGraph per optimiser step) == the same steps launched eagerly"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    class A:
        bias = True
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=6, B=8, shape="DD", nmax=400)
    g, x, label = synthetic.to_device(hb, dev)
    out = []
    for graphed in (False, True):
        torch.manual_seed(5)
        model = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").to(dev)
        tr = FlatTrainer(model, lr=1e-2, clip=2.0)
        gs = GraphedStep(tr, lambda: model.loss(model(x, g)[1], label), warmup=2, use_graph=graphed)
        for _ in range(3):
            gs.step()
        torch.cuda.synchronize()
        out.append((tr.flat_param.clone(), float(tr.state[0]), float(gs.loss.detach())))
    assert out[0][1] == out[1][1] == 3.0                       # the 2 warm-up steps are undone: 3 steps
    torch.testing.assert_close(out[1][0], out[0][0], rtol=0, atol=0)
    assert out[0][2] == out[1][2]


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["gat", "diffpool"])
def test_graphed_step_other_model_families(family):
    """the flat-bucket trainer and the hipGraph step are model-agnostic: the fused GAT layers (packed heads, blocked dW) and the
    DiffPool encoder (paired level-0 launches, one-launch pooled levels, fused contractions) replay from one hipGraph exactly
    as they run eagerly, and the loss goes down"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from two_stage_gnn_amd import dense_encoders as E, gat_encoders as G, synthetic, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    class A:
        bias = True
    dev = torch.device("cuda")
    out = []
    for graphed in (False, True):
        torch.manual_seed(7)
        if family == "gat":
            hb = synthetic.host_batch(seed=3, B=6, shape="DD", nmax=400)
            x, adj = synthetic.to_dense(hb)
            model = G.DGATEncoderGraph(89, 64, 64, 2, None, num_layers=2, num_heads=[4, 4], final_dim="number_classes",
                                       per_graph_features=True).to(dev)
            xr, g = model.packed_batch(x.to(dev), adj.to(dev), hb["sizes"])
            label = torch.from_numpy(hb["label"]).to(dev)
            loss_fn = lambda: model.loss(model(xr, g)[1], label)
        else:
            hb = synthetic.host_batch(seed=4, B=8, shape="DD", nmax=256)
            g, x, label = synthetic.to_device(hb, dev)
            model = E.SoftPoolingGcnEncoder(256, 89, 64, 64, 2, 3, 64, assign_ratio=0.125, num_pooling=2, bn=True, linkpred=False,
                                            args=A(), assign_input_dim=89, final_dim="number_classes").to(dev)
            loss_fn = lambda: model.loss(model(x, g, hb["sizes"], assign_x=x)[1], label)
        tr = FlatTrainer(model, lr=5e-3, clip=2.0)
        gs = GraphedStep(tr, loss_fn, warmup=2, use_graph=graphed)
        losses = []
        for _ in range(6):
            gs.step()
            torch.cuda.synchronize()                               # (the step runs on the GraphedStep's own stream)
            losses.append(float(gs.loss.detach()))
        mp.check_device_errors()
        out.append((tr.flat_param.clone(), losses))
    assert out[1][1][-1] < out[1][1][0]
    torch.testing.assert_close(out[1][0], out[0][0], rtol=0, atol=0)
    assert out[0][1] == out[1][1]


@pytest.mark.gpu
def test_deferred_loss_equals_ordinary_step():
    """FlatTrainer(defer_loss=True): the cross-entropy launches nothing, the head's backward kernel rebuilds its gradient and
    writes the loss value — same loss and same parameters after the step as the ordinary sequence (bitwise)"""
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer

    class A:
        bias = True
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=5, B=12, shape="DD", nmax=400)
    g, x, label = synthetic.to_device(hb, dev)
    outs = []
    for defer in (False, True):
        torch.manual_seed(3)
        m = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").to(dev)
        tr = FlatTrainer(m, lr=1e-2, clip=2.0, defer_loss=defer)
        losses = []
        for _ in range(3):
            loss = tr.step(lambda: m.loss(m(x, g)[1], label))
            losses.append(float(loss.detach()))
        outs.append((losses, tr.flat_param.clone()))
    assert outs[0][0] == outs[1][0]
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=0, atol=0)
    assert all(np.isfinite(v) and v > 0.0 for v in outs[1][0]) and len(set(outs[1][0])) == 3    # written, and changing step to step


@pytest.mark.gpu
def test_run_of_multi_step_graphs_equals_single_steps_bitwise():
    """GraphedStep(steps_per_replay=k).run(n): graph launches of k consecutive optimiser steps + single steps for the rest are the
    same n steps as n calls of step() — parameters, Adam moments, step counter and the last loss, bit for bit; and constructing
    the multi-step graph leaves the trainer's state as it found it"""
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    class A:
        bias = True
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=2, B=12, shape="DD", nmax=400)
    g, x, label = synthetic.to_device(hb, dev)
    outs = []
    for k in (1, 3):
        torch.manual_seed(3)
        m = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").to(dev)
        tr = FlatTrainer(m, lr=1e-2, clip=2.0, defer_loss=True)
        before = tr.flat_param.clone()
        gs = GraphedStep(tr, lambda: m.loss(m(x, g)[1], label), warmup=2, steps_per_replay=k)
        assert torch.equal(tr.flat_param, before) and float(tr.state[0]) == 0.0
        assert ("3 consecutive steps" in gs.describe()) == (k == 3)
        gs.run(7)                                            # k = 3: two graph launches of three steps + one single step
        l7 = gs.loss_value()
        gs.run(6)                                            # ... and a run that ends on a multi-step graph
        l13 = gs.loss_value()
        outs.append((l7, l13, tr.flat_param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), float(tr.state[0])))
    assert outs[0][5] == outs[1][5] == 13.0
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and outs[0][0] != outs[0][1]
    for a_, b_ in zip(outs[0][2:5], outs[1][2:5]):
        assert torch.equal(a_, b_)


@pytest.mark.gpu
def test_deferred_nll_equals_ordinary_sagpool_step():
    """SAGPool Net under FlatTrainer(defer_loss=True) with mp.nll_loss: the head's backward forms the nll gradient and writes
    the loss — same losses and parameters as torch's nll_loss through autograd (dropout off: identical random state)"""
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd import sag_layers as S, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    dev = torch.device("cuda")
    sizes = [20, 12, 31, 20, 9, 25, 14, 40]
    n = sum(sizes)
    gen = torch.Generator().manual_seed(9)
    src, dst, off = [], [], 0
    for nb in sizes:
        e = torch.randint(0, nb, (2, 3 * nb), generator=gen)
        e = e[:, e[0] != e[1]] + off
        src += [e[0], e[1]]; dst += [e[1], e[0]]
        off += nb
    code = torch.unique(torch.cat(src) * n + torch.cat(dst))
    ei = torch.stack([code // n, code % n]).to(dev)

    class D:
        pass
    d = D()
    d.x, d.edge_index = torch.randn(n, 4, generator=gen).to(dev), ei
    d.batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
    label = (torch.arange(len(sizes)) % 2).to(dev)
    outs = []
    for defer in (False, True):
        torch.manual_seed(11)
        net = S.Net(4, 64, 2, 0.5, 0.0, use_batch=True).to(dev).train()
        tr = FlatTrainer(net, lr=1e-2, clip=2.0, defer_loss=defer)
        losses = []
        for _ in range(3):
            loss = tr.step(lambda: mp.nll_loss(net(d), label))
            losses.append(float(loss.detach()))
        outs.append((losses, tr.flat_param.clone()))
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-6)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-5, atol=1e-7)
    assert all(np.isfinite(v) and v > 0.0 for v in outs[1][0]) and len(set(outs[1][0])) == 3


@pytest.mark.gpu
def test_parameter_feeding_two_fused_nodes_accumulates():
    """the fused backward nodes STORE into their slice of the flat bucket, so a parameter used by two fused nodes in
    one backward (the reference's tripletnet calls one encoder three times, tripletnet.py:36-38) must get the second
    contribution through autograd: direct placement == plain autograd == the sum of the single-forward gradients."""
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer

    class A:
        bias = True
    dev = torch.device("cuda")
    batches = [synthetic.to_device(synthetic.host_batch(seed=s_, B=5, shape="DD", nmax=300), dev) for s_ in (1, 2, 3)]
    flat = {}
    for direct in (False, True):
        torch.manual_seed(3)
        model = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").to(dev)
        tr = FlatTrainer(model, lr=1e-2, clip=2.0, direct_grads=direct)
        tr.zero_grad()
        loss = sum(model.loss(model(x, g)[1], label) for g, x, label in batches)          # three forwards, shared weights
        loss.backward()
        tr.gather_grads()
        if direct:
            assert tr.sink.reused and not tr._norm_ready          # the |grad|^2 shares of the first producer must not be used
        flat[direct] = tr.flat_grad.clone()
        singles = torch.zeros_like(tr.flat_grad)
        for g, x, label in batches:
            tr.zero_grad()
            model.loss(model(x, g)[1], label).backward()
            singles += tr.gather_grads()
        flat[("sum", direct)] = singles
        tr.zero_grad(); tr.gather_grads()
    scale = float(flat[False].abs().max())
    assert scale > 0
    torch.testing.assert_close(flat[True], flat[False], rtol=0, atol=2e-6 * scale)
    torch.testing.assert_close(flat[True], flat[("sum", True)], rtol=0, atol=2e-6 * scale)
    torch.testing.assert_close(flat[False], flat[("sum", False)], rtol=0, atol=2e-6 * scale)


@pytest.mark.gpu
def test_selfnorm_optimiser_sizes_and_replay():
    """the one-launch, barrier-free clip + Adam (every block sums the whole norm) at sizes around its block / vector
    boundaries, replayed from a hipGraph (the sign-off counter re-arms itself), against torch"""
    sys.path.insert(0, ROOT)
    from two_stage_gnn_amd import _native as nat
    dev = torch.device("cuda")
    for n in (1, 3, 1023, 1024, 1025, 4099, 61002, 131072):
        gen = torch.Generator().manual_seed(n)
        p0 = torch.randn(n, generator=gen).to(dev)
        grads = [torch.randn(n, generator=gen).to(dev) * (0.01 if n > 5000 else 1.0) for _ in range(3)]
        ref = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([ref], lr=1e-2)
        p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        state, ws = torch.zeros(4, device=dev), torch.zeros(264, device=dev)
        gbuf = torch.empty(n, device=dev)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            graph = torch.cuda.CUDAGraph()
            gbuf.copy_(grads[0])
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=s):
                nat.call("clip_adam_step_f32", p, gbuf, m, v, n, 1e-2, 0.9, 0.999, 1e-8, 0.0, 0.7, 0.5, state, ws, None)
            for gi in grads:
                gbuf.copy_(gi)
                graph.replay()
                ref.grad = gi * 0.5
                torch.nn.utils.clip_grad_norm_([ref], 0.7)
                opt.step()
            torch.cuda.synchronize()
        assert float(state[0]) == 3.0 and float(state[3]) == 0.0
        torch.testing.assert_close(float(state[1]), float((grads[-1] * 0.5).norm()), rtol=1e-5, atol=0)
        torch.testing.assert_close(p, ref.detach(), rtol=2e-5, atol=2e-6)


def _fallback_worker(rank, port, q):
    """a one-graph capture that raises on every rank (TSGNN_ONE_GRAPH_ANY_BACKEND=1 makes the auto mode try on a gloo group,
    TSGNN_TEST_BREAK_CAPTURE=all puts an operation no capture admits into it): the capture is invalidated, and GraphedStep must
    carry on (fresh stream, two graphs) with the trainer's state intact"""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TSGNN_ONE_GRAPH_ANY_BACKEND="1", TSGNN_GRAPH_ALLREDUCE="auto",
                      TSGNN_TEST_BREAK_CAPTURE="all")
    dist.init_process_group("gloo", rank=rank, world_size=2)
    torch.cuda.set_device(0)
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    class A:
        bias = True
    hb = synthetic.host_batch(seed=rank, B=6, shape="DD", nmax=400)
    g, x, label = synthetic.to_device(hb, torch.device("cuda"))
    finals = []
    for use_graph in (True, False):
        torch.manual_seed(1)
        m = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").cuda()
        tr = FlatTrainer(m, lr=1e-3, clip=2.0)
        gs = GraphedStep(tr, lambda: m.loss(m(x, g)[1], label), warmup=2, use_graph=use_graph)
        for _ in range(3):
            gs.step()
        torch.cuda.synchronize()
        finals.append((tr.flat_param.detach().cpu().numpy(), float(tr.state[0]), gs.describe()))
    q.put((rank, finals))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_failed_collective_capture_falls_back_to_two_graphs():
    ctx = mp_.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 311) % 2000
    procs = [ctx.Process(target=_fallback_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=90) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, ((p_graph, n_graph, note), (p_eager, n_eager, _)) in res:
        assert "fell back" in note and "two graphs" in note, note
        assert n_graph == n_eager == 3.0
        np.testing.assert_array_equal(p_graph, p_eager)            # the fall-back step == the eager step, state untouched by the attempt
    np.testing.assert_array_equal(res[0][1][0][0], res[1][1][0][0])    # replicas identical


def _disagree_worker(rank, port, q):
    """rank 0's capture raises (TSGNN_TEST_BREAK_CAPTURE=0: an operation no capture admits); rank 1's capture SUCCEEDS (its gloo
    all_reduce is left out of the capture, so nothing un-capturable is recorded).  The ranks then disagree about the one-graph step: both must fall
    back to two graphs, with matched collectives all the way (the failing rank used to skip the verification replay
    its peer ran — a bucket-sized SUM against a 1-element MIN)."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TSGNN_ONE_GRAPH_ANY_BACKEND="1", TSGNN_GRAPH_ALLREDUCE="auto",
                      TSGNN_TEST_BREAK_CAPTURE="0")
    dist.init_process_group("gloo", rank=rank, world_size=2)
    torch.cuda.set_device(0)
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep

    class A:
        bias = True
    hb = synthetic.host_batch(seed=rank, B=6, shape="DD", nmax=400)
    g, x, label = synthetic.to_device(hb, torch.device("cuda"))
    finals = []
    for use_graph in (True, False):
        torch.manual_seed(1)
        m = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").cuda()
        tr = FlatTrainer(m, lr=1e-3, clip=2.0)
        if rank == 1 and use_graph:
            real = tr.all_reduce
            tr.all_reduce = lambda: None if torch.cuda.is_current_stream_capturing() else real()
        gs = GraphedStep(tr, lambda: m.loss(m(x, g)[1], label), warmup=2, use_graph=use_graph)
        for _ in range(3):
            gs.step()
        gs.synchronize()
        finals.append((tr.flat_param.detach().cpu().numpy(), float(tr.state[0]), gs.describe()))
    q.put((rank, finals))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_ranks_that_disagree_about_the_capture_fall_back_together():
    ctx = mp_.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 977) % 2000
    procs = [ctx.Process(target=_disagree_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=90) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    notes = [r[1][0][2] for r in res]
    assert "this rank" in notes[0] and "another rank" in notes[1], notes
    for rank, ((p_graph, n_graph, note), (p_eager, n_eager, _)) in res:
        assert "fell back" in note and "two graphs" in note, note
        assert n_graph == n_eager == 3.0
        np.testing.assert_array_equal(p_graph, p_eager)
    np.testing.assert_array_equal(res[0][1][0][0], res[1][1][0][0])    # replicas identical


@pytest.mark.gpu
def test_bench_two_ranks_end_to_end_gloo():
    """`python bench.py --gpus 2` exactly as the driver's launcher runs it (self-spawned ranks through torch.distributed.run, per-rank
    seeds, the barrier + max-over-ranks clock, `per_rank` in the JSON line, check_device_errors) — on ONE GPU with the gloo backend
    (TSGNN_DIST_BACKEND=gloo: both ranks share the card), so that the first real multi-GPU run cannot fail on plumbing."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TSGNN_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2", "--full", "--no-cpu-baseline",
                        "--no-sweep", "--no-kernels", "--no-seeds", "--no-pyg", "--settle-steps", "4"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines                         # exactly ONE JSON line on stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["scaling"] == "weak" and d["config"]["global_batch"] == 64
    assert d["value"] > 0 and abs(d["value"] - 2 * 32 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    pr = d["per_rank"]
    assert [p["rank"] for p in pr] == [0, 1] and pr[0]["rows"] != pr[1]["rows"]          # rank r drew the batch of seed r
    assert all(p["ms_per_step"] > 0 for p in pr)
    assert d["steps_per_graph_launch"] == 1 and d["settle_untimed_steps"] == 4
    ar = d["allreduce"]                                         # the collective by itself, for the scaling analysis of a real N > 1 run
    assert ar["us_alone"] > 0 and ar["bytes"] > 4 * 50000 and ar["backend"] == "gloo" and ar["buckets"] == 1


def test_bench_full_is_an_option_and_off_by_default(monkeypatch):
    """`--full` exists, is off in a plain run, and the options that prune it still parse beside it"""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.steps == 5 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--no-sweep", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.full is True and a.no_sweep and a.no_cpu_baseline and not a.no_kernels


BENCH_EXTRAS = ("roofline", "value_over_seeds", "value_mean_over_seeds", "value_worst_seed", "pyg_surface",
                "ms_per_step_four_steps_per_graph", "allreduce", "ingest", "triplet")


@pytest.mark.gpu
def test_bench_plain_run_is_lean():
    """`bench.py --gpus 1 --steps N --warmup W` without `--full`: one JSON line with the headline fields and none of the other
    measurements, and at most 30 s of the whole process (start to exit, a fresh interpreter) outside its N + W steps."""
    import json, subprocess, time
    n, w = 50, 10
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(n), "--warmup", str(w)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == "graphs/sec fwd+bwd, DD batch=32 SAGE-3L h=128" and d["unit"] == "graphs/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["steps"] == n and d["warmup"] == w and d["full"] is False
    assert d["value"] > 0 and abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["steps_per_graph_launch"] == 1 and d["settle_untimed_steps"] == 128 and d["ms_per_step_unsettled"] > 0
    assert d["cpu_baseline"] is None and not [k for k in BENCH_EXTRAS if k in d]
    outside = wall - (n + w) * d["ms_per_step"] * 1e-3
    print("plain bench.py: %.2f s start to exit, %.2f s outside its %d steps" % (wall, outside, n + w))
    assert outside <= 30.0, outside


@pytest.mark.gpu
def test_bench_full_run_carries_every_other_figure():
    """`--full` goes on to what a plain run leaves out (a short CPU sample and the two smallest sweep sizes keep it brief): same
    headline fields, plus the per-kernel roofline, the aggregation sweep, four steps per launch, seeds, the pyg surface, the CPU line."""
    import json, subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "10", "--full",
                        "--cpu-steps", "3", "--sweep-sizes", "32,256", "--seeds", "0,6"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["full"] is True and d["value"] > 0 and abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    rf = d["roofline"]
    assert rf["step_launches"] == sum(k["launches_per_step"] for k in rf["step_kernels"]) > 0 and 0 < rf["frac"] <= 1
    assert [s_["graphs"] for s_ in rf["sweep"]] == [32, 256] and rf["aggregation_standalone"]["us_per_launch"] > 0
    assert d["ms_per_step_four_steps_per_graph"] > 0
    assert [s_["seed"] for s_ in d["value_over_seeds"]["per_seed"]] == [0, 6] and rf["straggler"]["ms_per_step"] > 0
    assert d["pyg_surface"]["ms_per_step"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["sparse_variant"]["value"] > 0


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """`bench.py --dump-outputs DIR` writes what its LAST timed step computed.  W = 1 and K = 3 steps without settling at two steps per
    graph launch: the timed steps are one 2-step replay and one single step, so the last step is not the 2-step graph's.  Judged against
    the same four optimiser steps taken eagerly on the same model and batch."""
    import json, subprocess
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--steps-per-graph", "2", "--settle-steps", "0", "--no-cpu-baseline", "--no-sweep", "--no-kernels", "--no-seeds",
                        "--no-pyg", "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = json.loads(r.stdout.decode())
    assert d["steps"] == 3 and d["steps_per_graph_launch"] == 2
    got = {f[:-len(".npy")]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path))}
    assert all(v.dtype == np.float32 for v in got.values())

    class Args:
        bias = True
    dev = torch.device("cuda")
    g, x, label = synthetic.to_device(synthetic.host_batch(seed=0, B=32, shape="DD", nmax=1000), dev)
    torch.manual_seed(1234)                                          # bench.py's seed and model
    model = E.GcnEncoderGraph(synthetic.SHAPES["DD"][2], 128, 128, 2, 3, bn=True, args=Args(), final_dim="number_classes").to(dev)
    trainer = FlatTrainer(model, lr=1e-3, clip=2.0, defer_loss=True)
    want = {}

    def loss_fn():
        want["head_hidden"], want["logits"] = model(x, g)
        return model.loss(want["logits"], label)
    for _ in range(4):
        want["loss"] = trainer.step(loss_fn)
    trainer.check()
    want.update(("param." + k, v) for k, v in model.state_dict().items())
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    want.update(("grad." + k, trainer.flat_grad[o:o + n].view_as(p)) for k, p, (o, n) in zip(names, trainer.params, trainer.views))
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        np.testing.assert_allclose(got[k], v.detach().float().cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=k)


def _poison_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from two_stage_gnn_amd import message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    dev = torch.device("cuda")
    torch.manual_seed(0)
    lin = torch.nn.Linear(32, 4).to(dev)
    tr = FlatTrainer(lin, lr=1e-2, clip=2.0)
    x = torch.randn(8, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(rank))

    def one():
        return tr.step(lambda: lin(x).square().mean())
    one(); tr.check()
    before = tr.flat_param.clone()
    if rank == 1:
        mp.device_error_word(dev).fill_(1.0)                 # what a kernel whose bounded barrier timed out leaves behind
    one()
    torch.cuda.synchronize()
    unchanged = bool(torch.equal(tr.flat_param, before))
    skipped = float(tr.state[3])
    msg = ""
    try:
        tr.check()
    except RuntimeError as e:
        msg = str(e)
    one(); tr.check()                                        # cleared: the next step is applied again, on every rank
    q.put((rank, unchanged, skipped, msg, tr.flat_param.detach().cpu().numpy(), float(tr.state[0])))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_error_word_of_one_rank_stops_every_rank():
    """the device error word used to be rank-local — the rank whose kernel failed skipped its optimiser update while the other
    ranks applied theirs with the already all-reduced gradients.  It now rides in the gradient all-reduce: a failure on rank 1 makes BOTH
    ranks skip, both raise at their next check, and the replicas stay bit-identical."""
    ctx = mp_.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 311) % 2000
    procs = [ctx.Process(target=_poison_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in res:
        assert r[1] and r[2] == 1.0, r[:4]                   # neither rank applied the poisoned step
    assert "another rank" in res[0][3] and "timed out" in res[1][3], (res[0][3], res[1][3])
    np.testing.assert_array_equal(res[0][4], res[1][4])      # replicas identical after the recovery step
    assert res[0][5] == res[1][5] == 2.0
