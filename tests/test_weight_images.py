"""Fragment-major weight images for the hidden layers' row panels (csrc/rowgemm_body.h BIMG, csrc/pack_body.h): the trailing
arguments of tsgnn_gather_rowgemm_st_f32 (pack descriptor), tsgnn_sage_layer_fwd_bn_f32 and tsgnn_sage_layer_bwd_f32 (image).

A launch with the image produces, bit for bit, what the same launch produces when it stages W through LDS; the images the first
layer's launch writes are those of tsgnn_sage_conv_pack_f32; and a replayed step packs from the parameters it is about to use, however
they were rewritten.  (The host-side validation of the arguments: test_weight_images_host.py.)"""
import numpy as np
import pytest
import torch


class _A:
    bias = True


def _poison(*ts):
    for t in ts:
        if t is not None:
            t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-7)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _record_step(model, x, g, label):
    """one eager forward + backward; -> the recorded launches [(entry, args, kernel)]"""
    from two_stage_gnn_amd import _native as nat
    prev, nat.trace = nat.trace, []
    try:
        model.loss(model(x, g)[1], label).backward()
        torch.cuda.synchronize()
        return nat.trace
    finally:
        nat.trace = prev


def _check_batch(model, x, g, label, tag):
    from two_stage_gnn_amd import _native as nat
    rec = _record_step(model, x, g, label)
    st = [r for r in rec if r[0] == "gather_rowgemm_st_f32"]
    fwd = [r for r in rec if r[0] == "sage_layer_fwd_bn_f32"]
    bwd = [r for r in rec if r[0] == "sage_layer_bwd_f32"]
    assert len(st) == 1 and len(fwd) == 2 and len(bwd) == 2, (tag, [r[0] for r in rec])
    assert st[0][1][-1] is not None and all(r[1][-1] is not None for r in fwd + bwd), "the step does not use the images"
    # ---- the images of layer 0's launch = tsgnn_sage_conv_pack_f32 of the same matrices, byte for byte
    # (the step's head launch left the integer sums and the packed maxima zero: the forward launches replay from that state)
    for r in fwd + bwd:
        r[1][-1].fill_(float("nan"))
    nat.call(st[0][0], *st[0][1])
    ref = torch.full((len(fwd) + len(bwd), 16384), float("nan"), device=x.device)
    sets = [(r[1][6], r[1][7], 1) for r in fwd] + [(r[1][6], r[1][7], 0) for r in bwd]
    d = np.asarray([len(sets)] + [v for t, (w, ldw, kn) in enumerate(sets) for v in (w.data_ptr(), ldw, 128, 128, kn, ref[t].data_ptr())],
                   np.int64)
    nat.call("sage_conv_pack_f32", d.ctypes.data)
    torch.cuda.synchronize()
    for t, r in enumerate(fwd + bwd):
        assert torch.equal(_bits(r[1][-1]), _bits(ref[t])), (tag, "image", t)
    # ---- forward launches, in the step's order: with the image / staged through LDS
    for r in fwd:
        a = list(r[1])
        v, rinv, z, packed, packed_out, mean, rstd, sums_out, ghost_out = a[9], a[11], a[12], a[22], a[23], a[27], a[28], a[30], a[31]
        outs = []
        for img in (a[-1], None):
            _poison(v[:int(a[14]) + int(a[16])], rinv, z[:int(a[14])], mean, rstd, ghost_out)
            for t in (packed, packed_out, sums_out):
                if t is not None:
                    t.zero_()
            nat.call(r[0], *(a[:-1] + [img]))
            torch.cuda.synchronize()
            outs.append([_bits(t).clone() for t in (v, rinv, z, packed, packed_out, mean, rstd, sums_out, ghost_out) if t is not None])
        assert ("units" in tag) == r[2].endswith(",true>"), (tag, r[2])
        for i, (p, q) in enumerate(zip(*outs)):
            assert torch.equal(p, q), (tag, r[2], "forward output", i)
    # ---- backward launches (their operands are what the step's backward left): dX and the slabs
    for r in bwd:
        a = list(r[1])
        dxs, ws = a[8], a[16]
        outs = []
        for img in (a[-1], None):
            _poison(dxs[:int(a[12])], ws)
            nat.call(r[0], *(a[:-1] + [img]))
            torch.cuda.synchronize()
            outs.append([_bits(dxs[:int(a[12])]).clone(), _bits(ws).clone()])
        assert torch.equal(outs[0][0], outs[1][0]), (tag, r[2], "dX")
        assert torch.equal(outs[0][1], outs[1][1]), (tag, r[2], "slabs")
    # leave the batch's accumulators as a step leaves them
    for r in fwd:
        for t in (r[1][22], r[1][23], r[1][30], r[1][25]):
            if t is not None:
                t.zero_()
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B,nmax,seed,tag", [
    ("DD", 32, 1000, 0, "DD b32 seed 0: 255 panels"),
    ("DD", 32, 1000, 3, "DD b32 seed 3: 271 panels, 8-row units"),
    ("DD", 32, 1000, 6, "DD b32 seed 6: 288 panels, 16-row units"),
    ("PROTEINS", 64, 620, 1, "PROTEINS b64: 77 panels, a partial last panel"),
])
def test_image_launches_equal_staged_launches(shape, B, nmax, seed, tag):
    """tsgnn_sage_layer_fwd_bn_f32 / tsgnn_sage_layer_bwd_f32 on the same operands with and without the image: every output bitwise
    equal (v, rinv, z, the packed maxima, mean / rstd, the integer sums, the ghost row's numbers; dX and the slabs)"""
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=seed, B=B, shape=shape, nmax=nmax)
    g, x, label = synthetic.to_device(hb, dev)
    npan = -(-int(g.n_rows) // 32)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    if "units" in tag and not (ncu < npan <= ncu + ncu // 2):
        tag = tag.replace("units", "rows")                         # (this device hosts every panel at once: plain panels)
    torch.manual_seed(1234)
    model = E.GcnEncoderGraph(synthetic.SHAPES[shape][2], 128, 128, 2, 3, bn=True, args=_A(), final_dim="number_classes").to(dev)
    _check_batch(model, x, g, label, tag)


@pytest.mark.gpu
def test_image_launches_equal_staged_launches_on_a_capacity_padded_batch():
    """the same on an ingest slot's batch: plain panels, padding rows behind the real ones"""
    from two_stage_gnn_amd import dense_encoders as E, ingest
    dev = torch.device("cuda")
    ds = ingest.synthetic_dataset(seed=9, n_graphs=24, shape="DD", nmax=600)
    ids = np.array([3, 17, 5, 11, 20, 8])
    n = int(ds.sizes[ids].sum())
    nnz = int(sum(ds.rowptr[ds.graph_ptr[i + 1]] - ds.rowptr[ds.graph_ptr[i]] for i in ids))
    slot = ingest.CapacityBatch(len(ids), 600, (n + 200 + 31) // 32 * 32, nnz + 500, ds.num_node_labels, dev)
    slot.collate(ds, ids)
    slot.pull()
    torch.cuda.synchronize()
    assert slot.row_cap > n
    torch.manual_seed(2)
    model = E.GcnEncoderGraph(ds.num_node_labels, 128, 128, 2, 3, bn=True, args=_A(), final_dim="number_classes").to(dev)
    _check_batch(model, slot.x, slot.g, slot.label, "capacity-padded batch")


@pytest.mark.gpu
def test_replayed_step_packs_from_the_parameters_it_uses():
    """no stale image: a captured step replayed after the parameters were overwritten in place (as a benchmark restores a snapshot)
    leaves the parameters and the loss of an eager step from the same state, bitwise"""
    from two_stage_gnn_amd import dense_encoders as E, synthetic
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=0, B=32, shape="DD", nmax=1000)
    g, x, label = synthetic.to_device(hb, dev)
    torch.manual_seed(1234)
    model = E.GcnEncoderGraph(89, 128, 128, 2, 3, bn=True, args=_A(), final_dim="number_classes").to(dev)
    tr = FlatTrainer(model, lr=1e-3, clip=2.0, defer_loss=True)
    gs = GraphedStep(tr, lambda: model.loss(model(x, g)[1], label), warmup=3)
    state = (tr.flat_param, tr.exp_avg, tr.exp_avg_sq, tr.state)
    snap = [t.clone() for t in state]
    gs.step()
    first = (gs.loss_value(), tr.flat_param.clone())
    gen = torch.Generator(device="cpu").manual_seed(7)
    other = (snap[0].cpu() * (1.0 + 0.25 * torch.randn(snap[0].numel(), generator=gen)) + 0.01 * torch.randn(snap[0].numel(), generator=gen)).to(dev)
    results = []
    for graphed in (True, False):
        for t, s_ in zip(state, [other] + snap[1:]):
            t.copy_(s_)
        torch.cuda.synchronize()
        if graphed:
            gs.step()
        else:
            with torch.cuda.stream(gs.stream):
                gs._fwd_bwd()
                tr.apply()
        results.append((gs.loss_value(), tr.flat_param.clone()))
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1])
    assert results[0][0] != first[0] and not torch.equal(results[0][1], first[1])     # (the other parameters really were another problem)
