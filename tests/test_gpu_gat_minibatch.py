"""The GAT mini-batch stream on the GPU (two_stage_gnn_amd/gat_stream.py ``MiniBatchStream``, csrc/gat_batch_stream.hip):

  1. the gather launch alone, through the C ABI, into guarded buffers prefilled with NaN / -1: every word against the numpy
     restatement (tests/gat_minibatch_util.launch_np), the real prefixes bit for bit against ``gat_triplet.assemble`` of the same
     resident pieces, for B = 1 .. 128 and four capacities (the default; exactly the first entry's own sums; those sums + 1; a
     ``row_cap`` that is no multiple of 4), every launch twice, the cursor and all ticket words after each; B = 3 and B = 1 bit for bit
     against the two existing GAT gather launches; the "big" set (several chunks per array); an entry that does not fit; a schedule
     word past ``n_graphs``;
  2. one streamed step per entry, in eval and train mode: ``ypred`` and the loss bit for bit ``eager_step`` on the exact batch;
     against B separate B = 1 dense calls of the module with loss = their mean at the band tests/test_gpu_gat_stream.py applies
     between its step and the module (outputs rtol 1e-4 / atol 1e-5, gradients 5e-3 max|g| + 1e-6), and against the float64
     restatement of those calls (oracle/dense_ref.gat_encoder) at 8 x the restatement's own fp32 rounding (tests/fp32_yardstick.py);
  3. the reference's fixture tests/golden/minibatch_gat.npz: at B = 1 six replays of one hipGraph over the reference's schedule give
     its losses and final parameters (the bands of tests/test_gpu_posttrain_gat.py's loop: 8 x the fp32 yardstick per loss, 2 T lr on
     the parameters); at B = 4 the rows of ``ypred`` are the per-graph ``ypred``, the loss their mean and the gradients the mean of
     the per-graph gradients (the bands of tests/test_gpu_gat_triplet.py's fixture test);
  4. poisoned capacity buffers and allocator memory; the launch trace; no host in the loop; an epoch from one hipGraph with its
     remainder through ``eager_loss``; B = 128; every refusal of the constructor, ``load`` and ``mine``.
Datasets, schedules and the restatement: tests/gat_minibatch_util.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_yardstick as FY
import gat_minibatch_util as M
import posttrain_families_ref as FR
import test_gpu_gat_stream as GS
from conftest import load_golden, params_of
from guard_buf import GUARD, PAT

pytestmark = pytest.mark.gpu

IPAT = GS.IPAT
NAME = "minibatch_gat"


def _stream(name, B, mode="eval", **kw):
    from two_stage_gnn_amd import gat_stream as S
    m = M.model(name, mode)
    objs = M.dataset(name)
    return m, objs, S.MiniBatchStream(m, objs, B, **kw)


# ------------------------------------------------------------------------------------------------ 1. the gather launch alone
class _Guarded:
    """n words on the device prefilled with -1, GUARD words of it behind"""

    def __init__(self, n, dtype):
        self.n, self.w = n, 2 if dtype == torch.int64 else 1
        self.bits = torch.full((self.w * n + GUARD,), IPAT, dtype=torch.int32, device="cuda")
        self.t = self.bits[:self.w * n].view(dtype)

    def get(self, what):
        b = self.bits.cpu()
        assert bool((b[self.w * self.n:] == IPAT).all()), "%s: guard words overwritten" % what
        return b[:self.w * self.n].view(torch.int64 if self.w == 2 else torch.int32).numpy()


def _launch(st, caps, entry="gat_batch_gather_f32", n_graphs=None):
    """one gather launch on the stream's arena, schedule buffer and ticket words into guarded buffers of capacities ``caps`` of their
    own -> {array: int32 bit view on the CPU, 'ids', 'label'}"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.triplet_stream import HEAD
    ar, B, heads = st.arena, st.B, st.heads
    Rc, Ec, Ic = caps
    isz, fsz, fnames = M.sizes_of(Rc, Ec, Ic, B, ar.ldf, heads)
    a4 = lambda v: (v + 3) // 4 * 4
    ioff = np.concatenate([[0], np.cumsum([a4(s + GUARD) for s in isz])])
    foff = np.concatenate([[0], np.cumsum([a4(s + GUARD) for s in fsz])])
    ibuf = torch.full((int(ioff[-1]),), IPAT, dtype=torch.int32, device="cuda")
    fbuf = torch.full((int(foff[-1]),), PAT, dtype=torch.int32, device="cuda").view(torch.float32)
    iv = {nm: ibuf[int(o):int(o) + s] for nm, o, s in zip(M.INT_NAMES, ioff, isz)}
    fv = {nm: fbuf[int(o):int(o) + s] for nm, o, s in zip(fnames, foff, fsz)}
    d = np.zeros(int(nat.lib().tsgnn_gat_assemble_header_words()), dtype=np.int64)
    d[1:7] = (Rc, Ec, Ic, B, ar.ldf, len(heads))
    d[7:7 + len(heads)] = heads
    d[11:25] = [t.data_ptr() for t in (iv["rowptr"], iv["col"], iv["rowptr_t"], iv["col_t"], iv["src_e_t"], iv["inv"], fv["row_mult"],
                                       iv["graph_ptr"], iv["row_graph"], iv["row_slot"], iv["iso_idx"], fv["iso_w"], iv["iso_ptr"], fv["x"])]
    for j, h in enumerate(heads):
        d[25 + j] = fv["iso_cols%d" % h].data_ptr()
    ids, lab = _Guarded(B, torch.int32), _Guarded(B, torch.int64)
    G = ar.n_graphs if n_graphs is None else n_graphs
    if entry == "gat_batch_gather_f32":
        nat.call(entry, st.records, G, st.buf, ar.words, ar.top[0], ar.top[1], ar.top[2], st.labels, st._sched[HEAD:], st.max_steps,
                 st._sched, st._tickets, B, d.ctypes.data, ids.t, lab.t)
        assert nat.last_kernel() == "gat_batch_gather_kernel"
    else:                                                     # the triplet / anchor launch on the same arena and schedule
        nat.call(entry, st.records, G, st.buf, ar.words, ar.top[0], ar.top[1], ar.top[2], st._sched[HEAD:], st.max_steps, st._sched,
                 st._sched[4:HEAD], d.ctypes.data, ids.t)
    got = {k: v.numpy() for k, v in GS._read((ibuf, fbuf, ioff, isz, foff, fsz), heads).items()}
    got["ids"], got["label"] = ids.get("ids"), lab.get("label")
    return got


def _after(st, k):
    from two_stage_gnn_amd.triplet_stream import HEAD
    assert st.position() == k and not bool(st._tickets.any()) and not bool(st._sched[4:HEAD].any()), (k, "cursor / ticket words")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().reshape(-1)


def _equals_assemble(got, st, objs, ids, cache, what):
    """the [:R] / [:E] / [:I] prefixes bit for bit ``gat_triplet.assemble`` of the same resident pieces"""
    from two_stage_gnn_amd import gat_triplet as GT
    x, g = GT.assemble([GT.resident_piece(objs[int(i)], st.device, cache) for i in ids], st.device, st.heads)
    n, E, I = int(g.n_rows), int(g.nnz), int(g._iso_list[3])
    for key, t in (("rowptr", g.rowptr), ("rowptr_t", g._t[0]), ("graph_ptr", g.graph_ptr), ("iso_ptr", g._iso_list[2])):
        assert np.array_equal(got[key][:t.numel()], _bits(t)), (what, key)
    for key, t in (("col", g.col), ("col_t", g._t[1]), ("src_e_t", g.src_e_t), ("inv", g._inv_e_t)):
        assert np.array_equal(got[key][:E], _bits(t)[:E]), (what, key)
    for key, t in (("row_graph", g.row_graph), ("row_slot", g.row_slot), ("row_mult", g.row_mult)):
        assert np.array_equal(got[key][:n], _bits(t)[:n]), (what, key)
    assert np.array_equal(got["iso_idx"][:I], _bits(g._iso_list[0])[:I]) and np.array_equal(got["iso_w"][:I], _bits(g._iso_list[1])[:I]), what
    assert np.array_equal(got["x"][:n * st.arena.ldf], _bits(x)), (what, "x")
    for h in st.heads:
        assert np.array_equal(got["iso_cols%d" % h][:n * h], _bits(g._iso_cols[h])[:n * h]), (what, h)


def _capacities(S, rec, sched, B, mode):
    """"default": the sums of the B largest; "exact": the first entry's own sums (no padding row at all); "plus1": those + 1; "odd": the
    schedule's own with a ``row_cap`` that is no multiple of 4"""
    if mode == "default":
        return S.default_caps(rec, B)
    if mode == "odd":
        sc = S.schedule_capacity(rec, sched)
        r = sc["row_cap"] + (1 if (sc["row_cap"] + 1) % 4 else 2)
        return r, sc["nnz_cap"] + 5, sc["iso_cap"] + 3
    return tuple(int(v) + (mode == "plus1") for v in S.entry_sums(rec, sched[:1])[0])


def _run_mode(st, objs, rec, per, lab, sched, caps, mode, cache, with_assemble):
    """every entry of ``sched`` twice at capacities ``caps``: each launch against the restatement, the second against the first"""
    twice = np.repeat(sched, 2, axis=0)
    st.load(twice)
    prev = None
    for k, ids in enumerate(twice):
        got = _launch(st, caps)
        _after(st, k + 1)
        want = M.launch_np(rec, per, lab, ids, caps[0], caps[1], caps[2], st.arena.ldf, st.heads)
        assert set(got) == set(want)
        for key in want:
            assert np.array_equal(got[key], want[key]), (mode, k, key, int((got[key] != want[key]).sum()))
        if k % 2:
            assert all(np.array_equal(got[key], prev[key]) for key in got), (mode, k, "second launch differs")
        elif with_assemble:
            _equals_assemble(got, st, objs, ids, cache, (mode, k))
        prev = got
    return len(twice)


def _check_launches(name, B, modes=("default", "exact", "plus1", "odd"), with_assemble=("default", "exact")):
    """"default" and "odd" on the dataset's stream.  "exact" and "plus1" on a stream over the first entry's B graphs ALONE: the entry
    point takes no capacity below the arena's largest piece, and on that arena the entry's own sums are never below it, so the case
    without any padding row is launched at every B, B = 1 included"""
    from two_stage_gnn_amd import gat_stream as S, resident as R
    full = M.schedule(name, B)
    rec, per = M.pieces(M.dataset(name))
    own = S.schedule_capacity(rec, full)                          # (the stream's own capacities only have to let ``load`` pass:
    hold = dict(zip(("row_cap", "nnz_cap", "iso_cap"), (max(a, own[k]) for a, k in zip(S.default_caps(rec, B), ("row_cap", "nnz_cap", "iso_cap")))))
    m, objs, st = _stream(name, B, **hold)                        # every launch below writes buffers of its own capacities)
    lab = M.labels(name)
    st.load(np.repeat(full, 2, axis=0))                           # (the longest schedule first: it sizes the schedule buffer)
    sub = [objs[int(i)] for i in full[0]]                         # the first entry's graphs as a dataset of their own
    rec1, per1 = M.pieces(sub)
    lab1 = lab[full[0]]
    st1 = S.MiniBatchStream(M.model(name), sub, B)
    sched1 = np.stack([np.arange(B), np.arange(B)[::-1]]).astype(np.int64)
    cache, cache1 = R.ResidentCache(), R.ResidentCache()
    launches = 0
    for mode in modes:
        if mode in ("exact", "plus1"):
            caps = _capacities(S, rec1, sched1, B, mode)
            need0 = S.entry_sums(rec1, sched1[:1])[0]
            assert (need0 >= rec1[:, 2:5].max(axis=0)).all() and S.fits_mask(sched1, rec1, B, *caps).all()
            if mode == "exact":
                assert tuple(int(v) for v in need0) == caps == (st1.row_cap, st1.nnz_cap, st1.iso_cap)      # no padding row at all
            launches += _run_mode(st1, sub, rec1, per1, lab1, sched1, caps, mode, cache1, mode in with_assemble)
            continue
        caps = _capacities(S, rec, full, B, mode)
        sched = full
        if mode == "default":                                     # (the entries that name one graph more often than the default holds
            sched = full[S.fits_mask(full, rec, B, *caps)]        # are left to the schedule's own capacity, "odd")
        assert S.fits_mask(sched, rec, B, *caps).all(), (mode, caps)
        if mode == "odd":
            assert caps[0] % 4
        launches += _run_mode(st, objs, rec, per, lab, sched, caps, mode, cache, mode in with_assemble)
    return launches


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128])
def test_gather_launch_equals_the_restatement_word_for_word(B):
    """every word the launch writes or leaves, padding included, against the numpy restatement; the real prefixes against
    ``gat_triplet.assemble``; ``ids_out`` and ``label_out``; guards intact; every launch twice, bit for bit; the cursor and every ticket
    word after each launch.  B = 64 / 65 sit on the wave boundary of the prologue's scan; fin 3 (ldf 4) and fin 8 (ldf 8) alternate"""
    name = "mb3" if B % 2 else "mb8"
    assert _check_launches(name, B) == 2 * (4 + 2 + 2 + 4)


@pytest.mark.parametrize("B", [3, 5])
def test_gather_launch_on_pieces_of_several_chunks(B):
    """the "big" set: ``x`` of every piece and the entry arrays of the largest span several 2,048-word chunks, pieces start off 16
    bytes in rows and in entries"""
    full = M.schedule("big", B)
    assert _check_launches("big", B, modes=("default", "exact", "odd")) == 2 * (2 + 2 + len(full))


@pytest.mark.parametrize("B", [3, 1])
def test_b3_and_b1_equal_the_existing_gather_launches_bit_for_bit(B):
    """at the triplet / anchor launch's capacities (B times the largest piece): every array and ``ids_out``"""
    from two_stage_gnn_amd import gat_stream as S
    for name in ("mb3", "big"):
        top = [int(v) for v in S.size_records(M.dataset(name)).max(axis=0)]
        m, objs, st = _stream(name, B, row_cap=B * top[0], nnz_cap=B * top[1], iso_cap=B * top[2])
        caps = tuple(B * t for t in st.arena.top)
        assert (st.row_cap, st.nnz_cap, st.iso_cap) == caps == st.arena.caps
        sched = M.schedule(name, 3)[:, :B]
        old = "gat_triplet_gather_f32" if B == 3 else "gat_anchor_gather_f32"
        st.load(sched)
        new = [_launch(st, caps) for _ in sched]
        st.load(sched)
        for k, ids in enumerate(sched):
            got = _launch(st, caps, entry=old)
            _after(st, k + 1)
            assert got["ids"].tolist() == ids.tolist() == new[k]["ids"].tolist()
            for key in got:
                if key != "label":                                # (the existing launches write no labels)
                    assert np.array_equal(got[key], new[k][key]), (name, k, key)


@pytest.mark.parametrize("name,B", [("mb3", 4), ("mb8", 65), ("big", 3)])
def test_an_entry_that_does_not_fit_writes_nothing_and_advances_the_cursor(name, B):
    """called directly through the ABI (``load`` would refuse it) at capacities of ONE largest piece in one of the three, which the
    entry point takes: every guarded word stays untouched, the cursor advances by one, the ticket words are zero"""
    from two_stage_gnn_amd import gat_stream as S
    m, objs, st = _stream(name, B)
    rec = st.arena.records.astype(np.int64)
    sched = M.schedule(name, B)[:1]
    need = S.entry_sums(rec, sched)[0]
    top = np.array(st.arena.top)
    st.load(np.repeat(sched, 4, axis=0))
    fired = 0
    for c in range(3):
        caps = [int(v) for v in np.maximum(need, top)]
        caps[c] = int(top[c])
        if need[c] <= caps[c]:
            continue
        fired += 1
        got = _launch(st, tuple(caps))
        _after(st, fired)
        for key, v in got.items():
            pat = PAT if key in ("row_mult", "iso_w", "x") or key.startswith("iso_cols") else IPAT
            assert bool((v == pat).all()), (c, key)
    assert fired >= 1
    got = _launch(st, tuple(int(v) for v in np.maximum(need, top)))              # the same entry where it fits: written
    _after(st, fired + 1)
    assert got["ids"].tolist() == sched[0].tolist() and got["graph_ptr"][B] == need[0]


@pytest.mark.parametrize("B", [3, 65])
def test_a_schedule_word_past_n_graphs_is_clamped_into_the_records(B):
    """the raw entry point told that the table holds G - 2 records (it holds G): schedule words G - 1 and G - 2 — outside the launch's
    range, inside the allocation — must give, word for word in every array, in ``ids_out`` and in the labels, what the same schedule
    with every index replaced by min(index, G - 3) gives (csrc/stream_protocol.h, stream_entry_id).  B = 65: the words of threads 63 and
    64, one in each of the prologue's two waves"""
    m, objs, st = _stream("mb3", B)
    G = len(objs)
    sched = M.schedule("mb3", B)[:3].copy()
    sched[sched >= G - 2] = 5
    sched[0, 0], sched[0, B - 1] = G - 1, G - 2
    sched[1, B // 2] = G - 1
    sched[2, B - 2], sched[2, B - 1] = G - 2, G - 1
    want_ids = np.minimum(sched, G - 3)
    caps = tuple(B * t for t in st.arena.top)

    def run(schedule):
        st.load(schedule)
        got = [_launch(st, caps, n_graphs=G - 2) for _ in schedule]
        _after(st, len(schedule))
        return got
    stale, clamped = run(sched), run(want_ids)
    for k in range(len(sched)):
        assert clamped[k]["ids"].tolist() == want_ids[k].tolist() and clamped[k]["label"].tolist() == M.labels("mb3")[want_ids[k]].tolist()
        for key in clamped[k]:
            assert np.array_equal(stale[k][key], clamped[k][key]), (k, key)


# ------------------------------------------------------------------------------------------------ 2. the streamed step
def _run(m, fn):
    m.zero_grad(set_to_none=True)
    loss, ypred = fn()
    loss.backward()
    return loss.detach().clone(), ypred.detach().clone(), GS.U.grads(m)


_REF = {}


def _dense_reference(name, ids):
    """B separate B = 1 dense calls of a deep copy of the seeded module, loss = the mean of their cross-entropies, backward; and the
    same in plain torch on the CPU (oracle/dense_ref.gat_encoder) in float64 and float32 -> (module, ref64, cpu32), each (ypred [B, C],
    loss, {parameter: grad}); computed once per (dataset, entry): leave them unchanged"""
    from oracle import dense_ref as R
    key = (name, tuple(int(i) for i in ids))
    if key not in _REF:
        objs = [M.dataset(name)[i] for i in key[1]]
        y = torch.tensor([int(o.graph["label"]) for o in objs])
        m = copy.deepcopy(M.model(name))
        x, adj, sz = GS.U.dense_of(objs)
        yp = torch.cat([m(x[b:b + 1], adj[b:b + 1], sz[b:b + 1])[1] for b in range(len(objs))])
        loss = torch.stack([m.loss(yp[b:b + 1], y[b:b + 1].cuda()) for b in range(len(objs))]).mean()
        loss.backward()
        mod = (yp.detach().cpu(), loss.detach().cpu(), {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in m.named_parameters()})
        outs = [mod]
        for dt in (torch.float64, torch.float32):
            p = {k: v.detach().cpu().to(dt).clone().requires_grad_(True) for k, v in M.model(name).state_dict().items()}
            yp = torch.cat([R.gat_encoder(p, x[b:b + 1].cpu().to(dt), adj[b:b + 1].cpu().to(dt), final_dim="number_classes")[1]
                            for b in range(len(objs))])
            loss = torch.stack([F.cross_entropy(yp[b:b + 1], y[b:b + 1]) for b in range(len(objs))]).mean()
            loss.backward()
            outs.append((yp.detach(), loss.detach(), {k: (v.grad.detach() if v.grad is not None else None) for k, v in p.items()}))
        _REF[key] = tuple(outs)
    return _REF[key]


def _check_entry(name, k, ids, m, st):
    """the streamed step of the cursor's entry against ``eager_step``, the module and the float64 restatement; figures are printed"""
    ls, ps, gs = _run(m, st.step)
    assert st.ids_out.tolist() == ids.tolist() and st.label.tolist() == M.labels(name)[ids].tolist()
    le, pe, ge = _run(m, lambda: st.eager_step(ids))
    assert ps.shape == (len(ids), M.N_CLASSES)
    assert GS._same_bits(ps, pe) and GS._same_bits(ls, le), (k, float((ps - pe).abs().max()), float(ls), float(le))
    assert set(gs) == set(ge)
    worst = max(float((gs[n_] - ge[n_]).abs().max()) for n_ in ge)
    print("%s B %d entry %d: loss %.6f, max|grad| %.3e, max|streamed - exact| gradient entry %.3e"
          % (name, len(ids), k, float(ls), max(float(v.abs().max()) for v in ge.values()), worst))
    (pm, lm, gm), (p64, l64, g64), (p32, l32, g32) = _dense_reference(name, ids)
    torch.testing.assert_close(ps.cpu(), pm, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ls.cpu(), lm, rtol=1e-4, atol=1e-5)
    for key, q in m.named_parameters():
        assert (q.grad is None) == (gm[key] is None), key
        if gm[key] is not None:
            bound = 5e-3 * float(gm[key].abs().max()) + 1e-6
            for what, g_ in (("streamed", gs[key]), ("exact", ge[key])):
                err = float((g_.cpu() - gm[key]).abs().max())
                assert err <= bound, (k, what, key, err, bound)
    what = "%s B %d entry %d " % (name, len(ids), k)
    FY._check(what + "ypred", ps, p64, p32)
    FY._check(what + "loss", ls.reshape(1), l64.reshape(1), l32.reshape(1))
    for key, r64 in g64.items():
        if r64 is None:
            assert key not in gs or not bool(gs[key].any()), key
        else:
            FY._check(what + "grad " + key, gs[key], r64, g32[key])


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name,B", [("mb3", 4), ("mb8", 5), ("big", 3)])
def test_streamed_step_equals_the_exact_batch_the_module_and_float64(name, B, mode):
    """one streamed step per entry from equal parameters (eval mode; training mode with all dropouts 0), at the schedule's own
    capacity where an entry names a graph more often than the default capacity holds"""
    from two_stage_gnn_amd import gat_stream as S
    sched = M.schedule(name, B)
    kw = {}
    rec = S.size_records(M.dataset(name))
    if not S.fits_mask(sched, rec, B, *S.default_caps(rec, B)).all():
        kw = S.schedule_capacity(rec, sched)
    m, objs, st = _stream(name, B, mode, **kw)
    assert st.fits(sched).all()
    st.load(sched)
    for k, ids in enumerate(sched):
        _check_entry(name, k, ids, m, st)
    assert st.position() == len(sched)


def test_batch_of_128_equals_the_exact_batch():
    """B = 128 once (two waves of records, sixteen assembler launches on the eager side): ``ypred`` and the loss bit for bit, every
    gradient at the band of the module comparison"""
    m, objs, st = _stream("mb8", 128, "train")
    sched = M.schedule("mb8", 128)[:2]
    st.load(sched)
    for k, ids in enumerate(sched):
        ls, ps, gs = _run(m, st.step)
        le, pe, ge = _run(m, lambda: st.eager_step(ids))
        assert st.ids_out.tolist() == ids.tolist() and ps.shape == (128, M.N_CLASSES)
        assert GS._same_bits(ps, pe) and GS._same_bits(ls, le) and np.isfinite(float(ls))
        for key in ge:
            err, bound = float((gs[key] - ge[key]).abs().max()), 5e-3 * float(ge[key].abs().max()) + 1e-6
            assert err <= bound, (k, key, err, bound)


# ------------------------------------------------------------------------------------------------ 3. the reference's fixture
def _golden_model(g, prefix="p."):
    from two_stage_gnn_amd import gat_encoders as G
    fin, hid, emb, lab = (int(v) for v in g["dims"])
    m = G.DGATEncoderGraph(fin, hid, emb, lab, None, num_layers=int(g["num_layers"]), num_heads=[int(h) for h in g["heads"]],
                           final_dim=str(g["final_dim"])).cuda()
    m.load_state_dict({k: v.cuda() for k, v in params_of(g, prefix).items()}, strict=True)
    return m.train()


def _loop64(g, dtype):
    """the reference's loop (train.py:110-130) in plain torch on the CPU in ``dtype`` -> (losses, final parameters)"""
    from oracle import dense_ref as R
    dicts = FR.PR.golden_graphs(g)
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params_of(g, "p.").items() if v.is_floating_point()}
    opt = torch.optim.Adam(list(p.values()), lr=float(g["lr"]))
    losses = []
    for i in g["loop.order"]:
        d = dicts[int(i)]
        opt.zero_grad(set_to_none=True)
        x, adj = torch.as_tensor(d["feats"]).to(dtype)[None], torch.as_tensor(d["adj"]).to(dtype)[None]
        loss = F.cross_entropy(R.gat_encoder(p, x, adj, final_dim="number_classes")[1], torch.tensor([int(d["label"])]))
        loss.backward()
        torch.nn.utils.clip_grad_norm_([v for v in p.values() if v.grad is not None], float(g["clip"]))
        opt.step()
        losses.append(loss.detach().reshape(1))
    return losses, {k: v.detach() for k, v in p.items()}


def test_fixture_loop_at_b1_from_one_hipgraph():
    """six replays over the reference's schedule at B = 1 (exactly the reference's loop: clip 2.0, Adam lr 1e-3): every loss within
    8 x the distance of the reference's own fp32 run (the fixture) from the float64 restatement of its loop, the final parameters within
    2 T lr of the float64 loop's and of the fixture's, ``map_model`` (no gradient) unmoved"""
    from two_stage_gnn_amd import gat_stream as S, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    g = load_golden(NAME)
    objs = FR.golden_objects(g)
    assert len(objs) == 8 and str(g["final_dim"]) == "number_classes"
    order = np.asarray(g["loop.order"], dtype=np.int64)
    T, lr = len(order), float(g["lr"])
    m = _golden_model(g)
    st = S.MiniBatchStream(m, objs, 1, max_steps=T)
    rec = st.arena.records
    assert rec[0, 1] == rec[0, 2] == 16 and rec[2, 1] == 1 and st.labels.tolist() == [int(g["g%d.label" % i]) for i in range(8)]
    assert rec[3, 4] >= 2                                           # an isolated real node beside the ghost representative
    gs = GraphedStep(FlatTrainer(m, lr=lr, clip=float(g["clip"])), st.loss())
    assert gs.describe().startswith("one graph"), gs.describe()
    st.load(order.reshape(-1, 1))
    l64, p64 = _loop64(g, torch.float64)
    got = []
    for s, i in enumerate(order):
        gs.step()
        gs.synchronize()
        assert st.ids_out.tolist() == [int(i)]
        got.append(gs.loss_value())
        print("step %d: loss %.7f, reference %.7f" % (s, got[-1], float(g["loop.loss"][s])))
    assert st.position() == T
    mp.check_device_errors()
    for s in range(T):
        FY._check("loop loss %d" % s, torch.tensor([got[s]]), l64[s], torch.tensor(g["loop.loss"][s:s + 1]))
    start, final = params_of(g, "p."), params_of(g, "final.")
    worst = 0.0
    for k, q in m.named_parameters():
        if k.startswith("map_model"):
            assert torch.equal(q.detach().cpu(), start[k]), k      # unmoved: zero moments = Adam skipping it
            continue
        worst = max(worst, float((q.detach().cpu().double() - p64[k]).abs().max()), float((q.detach().cpu() - final[k]).abs().max()))
        assert float((q.detach().cpu() - start[k]).abs().max()) > lr, k              # (the steps trained it)
    print("max parameter difference after %d steps: %.3e (bound %.3e)" % (T, worst, 2 * T * lr))
    assert worst <= 2 * T * lr


def test_fixture_batches_of_four_are_four_reference_forwards():
    """B = 4 from the fixture's parameters: the rows of ``ypred`` are the reference's per-graph ``ypred``, the loss is the mean of its
    four losses and every gradient the mean of its four gradients (tests/test_gpu_gat_triplet.py's fixture bands: outputs and loss
    rtol 1e-4 / atol 1e-5, gradients rtol 2e-3 / atol 1e-4)"""
    from two_stage_gnn_amd import gat_stream as S
    g = load_golden(NAME)
    objs = FR.golden_objects(g)
    m = _golden_model(g)
    sched = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [3, 0, 7, 2]], dtype=np.int64)
    st = S.MiniBatchStream(m, objs, 4)
    st.load(sched)
    for ids in sched:
        for fn in (st.step, lambda: st.eager_step(ids)):
            loss, ypred, gs = _run(m, fn)
            np.testing.assert_allclose(ypred.cpu().numpy(), np.concatenate([g["b%d.ypred" % i] for i in ids]), rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(float(loss), np.mean([float(g["b%d.loss" % i]) for i in ids]), rtol=1e-4, atol=1e-5)
            for k, q in m.named_parameters():
                ref = np.mean([g["b%d.g.%s" % (i, k)] for i in ids], axis=0)
                got = gs[k].cpu().numpy() if k in gs else np.zeros_like(ref)
                np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-4, err_msg="%s %s" % (ids.tolist(), k))
        assert st.ids_out.tolist() == ids.tolist()


# ------------------------------------------------------------------------------------------------ 4. poisoned padding
@pytest.mark.parametrize("name,B", [("mb3", 4), ("big", 3)])
def test_poisoned_capacity_buffers_and_allocator_memory_change_nothing(name, B):
    """before every step both capacity buffers, ``ids_out`` and the labels hold NaN / -1 in every word and torch.empty hands the node
    memory that holds NaN: loss, ``ypred`` and every gradient are finite and bit for bit the clean run's"""
    from two_stage_gnn_amd import _native as nat, gat_stream as S
    sched = M.schedule(name, B)
    m, objs, st = _stream(name, B, "train", **S.schedule_capacity(S.size_records(M.dataset(name)), sched))
    st.load(sched)
    nat.trace = []
    try:
        clean = [_run(m, st.step) for _ in sched]
        sizes = sorted({a.untyped_storage().nbytes() for t in nat.trace for a in t[1] if isinstance(a, torch.Tensor)})
    finally:
        nat.trace = None
    assert len(sizes) > 8
    st.load(sched)
    for k, ids in enumerate(sched):
        st._ibuf.fill_(IPAT)
        st._fbuf.view(torch.int32).fill_(PAT)
        st.ids_out.fill_(IPAT)
        st.label.fill_(IPAT)
        GS._poison(sizes)
        loss, ypred, gs = _run(m, st.step)
        assert st.ids_out.tolist() == ids.tolist()
        assert np.isfinite(float(loss)) and bool(torch.isfinite(ypred).all()) and all(bool(torch.isfinite(v).all()) for v in gs.values())
        assert GS._same_bits(loss, clean[k][0]) and GS._same_bits(ypred, clean[k][1]), (k, float(loss), float(clean[k][0]))
        assert set(gs) == set(clean[k][2])
        for key, v in gs.items():
            assert GS._same_bits(v, clean[k][2][key]), (k, key, float((v - clean[k][2][key]).abs().max()))


# ------------------------------------------------------------------------------------------------ 5. the trace, no host in the loop
@pytest.mark.parametrize("name,B", [("mb8", 4), ("big", 3)])
def test_launch_trace_is_the_resident_exact_step_behind_one_gather_launch(name, B):
    """the library launches of a streamed step are those of the resident exact step (``gat_triplet.assemble`` aside) with
    ``gat_batch_gather_kernel`` in front: no capacity form of any layer kernel was needed"""
    from two_stage_gnn_amd import gat_triplet as GT
    m, objs, st = _stream(name, B, "train")
    sched = M.schedule(name, B)[:1]
    st.load(np.repeat(sched, 3, axis=0))
    for _ in range(2):                                            # (warm: allocator, library load, the resident pieces)
        _run(m, lambda: st.eager_step(sched[0]))
    _run(m, st.step)
    box = {}

    def resident():
        parts = [GT.resident_piece(objs[int(i)], st.device, st._cache) for i in sched[0]]
        box["b"] = GT.assemble(parts, st.device, st.heads)
    asm, _ = GS._traced(resident)
    y = torch.from_numpy(M.labels(name)[sched[0]].astype(np.int64)).cuda()
    m.zero_grad(set_to_none=True)
    res, _ = GS._traced(lambda: st._head(box["b"][0], box["b"][1], y)[0].backward())
    m.zero_grad(set_to_none=True)
    from two_stage_gnn_amd import _native as nat
    nat.trace = []
    try:
        st.loss()().backward()
        got, kernels = [t[0] for t in nat.trace], [t[2] for t in nat.trace]
    finally:
        nat.trace = None
    print("library launches of a streamed GAT mini-batch step (%s, B %d): %d\n%s" % (name, B, len(got), " ".join(got)))
    assert asm == ["gat_assemble_f32"] * -(-B // 8)
    assert got[0] == "gat_batch_gather_f32" and kernels[0] == "gat_batch_gather_kernel" and got[1:] == res
    assert got.count("gat_batch_gather_f32") == 1 and "gat_assemble_f32" not in got and len(res) >= 6
    assert got.count("gat_attn_fwd_f32") == 2 and "readout_max_fwd_f32" in got


def test_no_host_in_the_loop():
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    B = 4
    m, objs, st = _stream("mb8", B, "train")
    sched = M.schedule("mb8", B)
    st.load(sched)
    gs = GraphedStep(FlatTrainer(m, lr=1e-3, clip=2.0), st.loss())
    st.load(sched)
    T = len(st)
    gs.step()
    gs.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(T):
            gs.step()
        with pytest.raises(RuntimeError):
            gs.loss.cpu()                                         # (the mode is live: a copy to the host IS flagged)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    gs.synchronize()                                              # (the replays run on the step's own stream)
    assert st.position() == T + 1 and np.isfinite(gs.loss_value())


# ------------------------------------------------------------------------------------------------ 6. an epoch
def test_an_epoch_from_one_hipgraph_equals_uncaptured_streamed_steps():
    """``epoch_schedule`` on 37 graphs at B = 8: the full entries from ONE ``GraphedStep`` (clip 2.0, Adam: the reference's step), the
    remainder through ``eager_loss``; against uncaptured streamed steps of a deep-copied model — the same route run two ways, so rtol
    1e-5 / atol 1e-6 on every parameter (the rule of test_gpu_gat_stream's replay test).  ``ids_out`` walks the schedule and the
    parameters moved."""
    from two_stage_gnn_amd import gat_stream as S, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    from two_stage_gnn_amd.minibatch_stream import epoch_schedule
    B, G = 8, 37
    full, rest = epoch_schedule(G, B, np.random.default_rng(11))
    assert full.shape == (4, B) and rest.shape == (5,)
    m1, objs = M.model("mb8", "train"), M.dataset("mb8")[:G]
    st1 = S.MiniBatchStream(m1, objs, B, max_steps=len(full))
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    kw = dict(lr=1e-3, clip=2.0)

    def eager_step(tr, st, ids):
        tr.zero_grad()
        loss = st.eager_loss(ids)
        tr.backward(loss)
        tr.gather_grads()
        tr.apply()
        return float(loss.detach())
    st2 = S.MiniBatchStream(m2, objs, B)
    st2.load(full)
    tr2 = FlatTrainer(m2, **kw)
    step2 = st2.loss()
    for ids in full:
        tr2.step(step2)
        assert st2.ids_out.tolist() == ids.tolist()
    plain = eager_step(tr2, st2, rest)
    assert len(st1) == 1 and st1.fits(full).all()                               # (the warm-up entry: B copies of the one-node graph)
    tr1 = FlatTrainer(m1, **kw)
    gs = GraphedStep(tr1, st1.loss())                                           # (its warm-up steps consume the warm-up entry ...)
    assert gs.describe().startswith("one graph"), gs.describe()
    st1.load(full)                                                              # ... so the epoch starts here: cursor := 0
    for ids in full:
        gs.step()
        gs.synchronize()
        assert st1.ids_out.tolist() == ids.tolist()
    assert st1.position() == len(full) and np.isfinite(gs.loss_value())
    streamed = eager_step(tr1, st1, rest)
    mp.check_device_errors()
    assert abs(streamed - plain) <= 1e-5 * max(1.0, abs(plain))
    moved = 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6, msg=lambda s_, k=k: k + ": " + s_)
        moved += int(not torch.equal(p1.detach(), start[k]))
    assert moved >= 10


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_constructor_load_and_mine_refuse(monkeypatch):
    from two_stage_gnn_amd import gat_fused, gat_stream as S, gat_triplet, resident
    from two_stage_gnn_amd import gat_encoders as G
    objs = M.dataset("mb8")
    route = "eager route"
    with pytest.raises(TypeError, match="DGATEncoderGraph.*" + route):
        S.MiniBatchStream(object(), objs, 4)
    with pytest.raises(TypeError, match="DGATEncoderGraph.*" + route):
        S.MiniBatchStream(gat_triplet.tripletnet(M.model("mb8")), objs, 4)      # not a bare encoder
    with pytest.raises(TypeError, match="final_dim.*" + route):
        S.MiniBatchStream(M.model("mb8", final_dim="output_dim"), objs, 4)
    with pytest.raises(TypeError, match="GPU only.*" + route):
        S.MiniBatchStream(M.model("mb8", dev="cpu"), objs, 4)
    with monkeypatch.context() as mk:
        mk.setattr(resident, "RESIDENT", False)
        with pytest.raises(TypeError, match="RESIDENT.*" + route):
            S.MiniBatchStream(M.model("mb8"), objs, 4)
    with monkeypatch.context() as mk:
        mk.setattr(gat_fused, "FUSED", False)
        with pytest.raises(TypeError, match="heads_ok.*" + route):
            S.MiniBatchStream(M.model("mb8"), objs, 4)
    with monkeypatch.context() as mk:                              # a head DGATEncoderGraph.head would hand to library GEMMs
        mk.setattr(G, "FUSED_HEAD", False)
        with pytest.raises(TypeError, match="fused head launches.*" + route):
            S.MiniBatchStream(M.model("mb8"), objs, 4)
    five = G.DGATEncoderGraph(8, 8, 8, 3, None, num_layers=6, num_heads=[1, 2, 3, 4, 5, 5], neg_input_slopes=[0.2] * 6, dropouts=[0.0] * 6,
                              final_dim="number_classes").cuda()
    with pytest.raises(TypeError, match="four distinct head counts.*" + route):
        S.MiniBatchStream(five, objs, 4)
    deep = G.DGATEncoderGraph(8, 8, 8, 3, None, num_layers=5, num_heads=[2] * 5, neg_input_slopes=[0.2] * 5, dropouts=[0.0] * 5,
                              final_dim="number_classes").cuda()
    with pytest.raises(TypeError, match="at most 4 layers.*" + route):
        S.MiniBatchStream(deep, objs, 4)
    for mode in ("eval", "train"):                                 # dropout > 0 is refused whatever the mode
        with pytest.raises(TypeError, match="dropout.*" + route):
            S.MiniBatchStream(M.model("mb8", mode, dropouts=[0.0, 0.3]), objs, 4)
    for B in (0, 129):
        with pytest.raises(ValueError, match="outside 1..128.*" + route):
            S.MiniBatchStream(M.model("mb8"), objs, B)
    with pytest.raises(ValueError, match="3 features per node, the model takes 8"):
        S.MiniBatchStream(M.model("mb8"), M.dataset("mb3"), 4)
    for kw in (dict(row_cap=11), dict(nnz_cap=3), dict(iso_cap=1)):               # below ONE largest piece
        with pytest.raises(ValueError, match="largest piece.*" + route):
            S.MiniBatchStream(M.model("mb8"), objs, 4, **kw)
    bad = list(objs[:6])
    bad[2] = copy.deepcopy(bad[2])
    bad[2].graph["label"] = 3
    with pytest.raises(ValueError, match="graph 2: label 3 lies outside"):
        S.MiniBatchStream(M.model("mb8"), bad, 4)
    # an iso_cap past 64 columns per graph: the fused node declines the gathered batch's list (attention._isolated_list)
    with pytest.raises(TypeError, match="fused GAT node on the gathered batch.*" + route):
        S.MiniBatchStream(M.model("mb8"), objs, 4, iso_cap=64 * 4 + 1)
    assert S.MiniBatchStream(M.model("mb8"), objs, 4, iso_cap=64 * 4).iso_cap == 256
    m, objs, st = _stream("mb8", 4, max_steps=3)
    assert len(st) == 1 and st.position() == 0
    with pytest.raises(RuntimeError, match="no negative to mine"):
        st.mine(None, None, 1.0)
    sched = M.schedule("mb8", 4)
    with pytest.raises(ValueError, match="exceeds"):
        st.load(sched)                                             # four entries into a buffer of three
    assert st.load(sched[:3]) == 3
    with pytest.raises(ValueError, match="indices"):
        st.load(np.array([[0, 1, 2, 160]]))
    with pytest.raises(ValueError, match="shape"):
        st.load(np.array([[0, 1, 2]]))
    big = int(np.argmax(st.arena.records[:, 2] * (1 << 20) + st.arena.records[:, 3]))
    over = np.array([[0, 1, 2, 3], [big] * 4])                      # four times the largest graph: past the default capacity
    with pytest.raises(ValueError, match="schedule entry 1 .*" + route):
        st.load(over)
    assert st.fits(over).tolist() == [True, False]
    for bad_ids in (np.zeros(0, dtype=np.int64), np.arange(5), np.array([0.5]), np.array([160])):
        with pytest.raises(ValueError):
            st.eager_loss(bad_ids)
    # the warm-up schedule serves a step: the smallest graph B times
    m2, objs2, st2 = _stream("mb8", 4, max_steps=3)
    small = int(np.argmin(st2.arena.records[:, 2]))
    assert np.isfinite(float(st2.loss()().detach())) and st2.ids_out.tolist() == [small] * 4
    top = st2.arena.top
    with pytest.raises(ValueError, match="max_steps.*no graph"):
        _stream("mb8", 8, max_steps=2, row_cap=top[0])             # one largest piece: eight copies of no graph fit 12 rows
    # dropout that turns up after construction: step() refuses
    for hd in m2.modules():
        if isinstance(hd, G.DGATHead):
            hd.dropout = 0.25
    m2.train()
    with pytest.raises(RuntimeError, match="dropout.*" + route):
        st2.step()
    with pytest.raises(RuntimeError, match="load"):
        S.MiniBatchStream(M.model("mb8"), objs, 4).gather()
