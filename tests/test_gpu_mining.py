"""Hard / semi-hard negative mining on the GPU (csrc/mine.hip through ``tsgnn_mine_negatives_f32``, two_stage_gnn_amd/mining.py,
``ArenaStream.mine``).

(a) the reference's own fixtures (tests/golden/mining_*.npz) through the C ABI, both modes, exactly;
(b) the integer-valued synthetic cases of tests/mining_cases.py against ``mining_ref.mine_int``, exactly;
(c) the same launches on guarded buffers: the schedule inside a larger int32 buffer of -7 (at a word offset that is NOT a multiple of
    four), the embeddings with ld > dim, NaN in the row padding and in rows past n_graphs; every launch twice, bit for bit; the count;
(d) standard-normal embeddings, E = 64, two classes of 300: every choice passes ``mining_ref.acceptable`` with tau = 2 (E + 2) 2^-24
    (derived, see ``mining_ref.tau``) and at most 1% of the entries differ from float64's choice (tests/test_mining_host.py checks
    that fp32 numpy stays within that on the same seeds);
(e) ``embed_dataset`` -> ``load`` -> ``mine`` -> T replays of one ``GraphedStep`` for ``triplet_stream.TripletStream`` (inherits
    ``ArenaStream.__init__``) and ``gat_stream.TripletStream`` (has its own): ``ids_out`` walks the mined schedule, the replayed step's
    distances are bit for bit the eager drop-in's on the mined triplet, hardness 0 leaves the buffer alone, a second load + mine
    serves the same captured step;
(f) ``mine_negatives_torch`` on device tensors against the kernel on the cases of (b)."""
import copy

import numpy as np
import pytest
import torch

import mining_cases as MC
import mining_ref as MR
from conftest import load_golden

pytestmark = pytest.mark.gpu

FILL, PAD_WORDS, OFFSET = -7, 16, 13
MODES = [(MR.SEMI_HARD, "semi", 0.5), (MR.HARDEST, "hardest", 1)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Launch:
    """one problem on guarded device buffers; ``run(mode)`` restores the drawn schedule, launches and returns the [T, 3] result"""

    def __init__(self, emb, sched, class_of, class_ptr, members, extra_ld=4, extra_rows=3):
        from two_stage_gnn_amd import _native as nat
        self.nat = nat
        G, dim = emb.shape
        self.G, self.dim, self.T, self.C = G, dim, sched.shape[0], class_ptr.size - 1
        self.ld = (dim + 3) // 4 * 4 + extra_ld
        x = torch.full((G + extra_rows, self.ld), float("nan"), dtype=torch.float32, device="cuda")
        x[:G, :dim] = _dev(emb.astype(np.float32))
        self.x = x
        self.class_of, self.class_ptr, self.members = _dev(class_of.astype(np.int32)), _dev(class_ptr.astype(np.int32)), _dev(members.astype(np.int32))
        self.drawn = _dev(sched.astype(np.int32)).reshape(-1)
        self.buf = torch.full((OFFSET + 3 * self.T + PAD_WORDS,), FILL, dtype=torch.int32, device="cuda")
        self.view = self.buf[OFFSET:OFFSET + 3 * self.T]
        self.cnt = torch.full((3,), FILL, dtype=torch.int32, device="cuda")

    def run(self, mode, count=True):
        self.buf.fill_(FILL)
        self.view.copy_(self.drawn)
        self.cnt[1] = 0
        self.nat.call("mine_negatives_f32", self.x, self.ld, self.G, self.dim, self.class_of, self.class_ptr, self.members, self.C,
                      self.view, self.T, mode, self.cnt[1:2] if count else None)
        return self.buf.cpu().numpy().copy(), self.cnt.cpu().numpy().copy()

    def check_guards(self, buf, cnt, drawn):
        assert (buf[:OFFSET] == FILL).all() and (buf[OFFSET + 3 * self.T:] == FILL).all(), "guard words of the schedule overwritten"
        got = buf[OFFSET:OFFSET + 3 * self.T].reshape(self.T, 3)
        assert np.array_equal(got[:, :2], drawn[:, :2]), "columns 0 / 1 were written"
        assert cnt[0] == FILL and cnt[2] == FILL
        return got


# ------------------------------------------------------------------------------------------------ (a) the reference's fixtures
@pytest.mark.parametrize("name", ["mining_dense", "mining_sag"])
def test_fixtures_through_the_c_abi(name):
    z = load_golden(name)
    for ep in range(z["members"].shape[0]):
        rows = np.flatnonzero(z["epoch_of"] == ep)
        L = Launch(z["emb"], z["drawn"][rows], z["class_of"], z["class_ptr"], z["members"][ep])
        for mode, key, _ in MODES:
            buf, cnt = L.run(mode)
            got = L.check_guards(buf, cnt, z["drawn"][rows])
            np.testing.assert_array_equal(got, z[key][rows], err_msg="%s epoch %d %s" % (name, ep, key))
            assert cnt[1] == MR.changed(z["drawn"][rows], z[key][rows])


# ------------------------------------------------------------------------------------------------ (b) + (c) the synthetic cases
_LAUNCH = {}


def _case_launch(i):
    if i not in _LAUNCH:
        c = MC.build(i)
        _LAUNCH[i] = Launch(c.emb, c.sched, c.class_of, c.class_ptr, c.members)
    return _LAUNCH[i]


@pytest.mark.parametrize("mode", [MR.SEMI_HARD, MR.HARDEST])
@pytest.mark.parametrize("i", range(len(MC.CASES)), ids=MC.IDS)
def test_integer_valued_cases_are_exact(i, mode):
    c, L = MC.build(i), _case_launch(i)
    buf, _ = L.run(mode)
    got = buf[OFFSET:OFFSET + 3 * c.T].reshape(c.T, 3)
    want = MC.expected(i, mode)
    wrong = np.flatnonzero(got[:, 2] != want[:, 2])
    assert wrong.size == 0, "entries %s: got %s, want %s" % (wrong[:8].tolist(), got[wrong[:8]].tolist(), want[wrong[:8]].tolist())
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("mode", [MR.SEMI_HARD, MR.HARDEST])
@pytest.mark.parametrize("i", range(len(MC.CASES)), ids=MC.IDS)
def test_guarded_buffers_two_launches_and_the_count(i, mode):
    c, L = MC.build(i), _case_launch(i)
    assert L.ld > c.dim and bool(torch.isnan(L.x[:, c.dim:]).all()) and bool(torch.isnan(L.x[c.G:]).all())
    buf1, cnt1 = L.run(mode)
    buf2, cnt2 = L.run(mode)
    assert buf1.tobytes() == buf2.tobytes() and cnt1.tobytes() == cnt2.tobytes()
    got = L.check_guards(buf1, cnt1, c.sched)
    assert cnt1[1] == MR.changed(c.sched, MC.expected(i, mode)) == MR.changed(c.sched, got)
    # the count accumulates, and a launch without it writes the same schedule
    L.cnt[1] = 5
    L.view.copy_(L.drawn)
    L.nat.call("mine_negatives_f32", L.x, L.ld, L.G, L.dim, L.class_of, L.class_ptr, L.members, L.C, L.view, L.T, mode, L.cnt[1:2])
    assert int(L.cnt[1]) == 5 + cnt1[1]
    buf3, cnt3 = L.run(mode, count=False)
    assert buf3.tobytes() == buf1.tobytes() and cnt3[1] == 0


def test_a_mined_schedule_is_a_fixed_point_for_hardest():
    """mining the mined schedule again changes nothing in hardest mode (the mined negative is the minimum; it wins its ties)"""
    i = 4
    c, L = MC.build(i), _case_launch(i)
    buf, _ = L.run(MR.HARDEST)
    L.cnt[1] = 0
    L.nat.call("mine_negatives_f32", L.x, L.ld, L.G, L.dim, L.class_of, L.class_ptr, L.members, L.C, L.view, L.T, MR.HARDEST, L.cnt[1:2])
    assert int(L.cnt[1]) == 0 and L.buf.cpu().numpy().tobytes() == buf.tobytes()


# ------------------------------------------------------------------------------------------------ (d) real-valued embeddings
@pytest.mark.parametrize("mode", [MR.SEMI_HARD, MR.HARDEST])
@pytest.mark.parametrize("seed", MC.REAL_SEEDS)
def test_real_valued_embeddings_within_the_derived_band(seed, mode):
    c = MC.real_case(seed)
    t = MR.tau(c.dim)
    L = Launch(c.emb, c.sched, c.class_of, c.class_ptr, c.members)
    buf, cnt = L.run(mode)
    got = L.check_guards(buf, cnt, c.sched)
    ref = MR.mine(c.emb, c.sched, c.class_of, c.class_ptr, c.members, mode)
    differ = MR.changed(ref, got)
    print("seed %d mode %d: %d of %d entries differ from float64's choice; %d changed by mining" % (seed, mode, differ, c.T, int(cnt[1])))
    bad = [k for k in range(c.T) if not MR.acceptable(c.emb, c.sched[k], int(got[k, 2]), c.class_of, c.class_ptr, c.members, mode, t)]
    assert not bad, "entries outside the band: %s" % bad[:8]
    assert differ <= c.T // 100
    assert cnt[1] == MR.changed(c.sched, got)


# ------------------------------------------------------------------------------------------------ (f) the torch composition
@pytest.mark.parametrize("i", range(len(MC.CASES)), ids=MC.IDS)
def test_torch_composition_on_the_device_agrees_with_the_kernel(i):
    from two_stage_gnn_amd import mining as M
    c, L = MC.build(i), _case_launch(i)
    index = M.ClassIndex(c.class_of, c.class_ptr, c.members, range(c.C))
    emb, sched = L.x[:c.G, :c.dim], _dev(c.sched)
    assert M.kernel_ok(emb, index)
    for mode, _, hardness in MODES:
        buf, _ = L.run(mode)
        kernel = buf[OFFSET:OFFSET + 3 * c.T].reshape(c.T, 3)[:, 2]
        comp = M.mine_negatives_torch(emb, sched, index, hardness)
        assert comp.is_cuda and comp.dtype == torch.int32
        np.testing.assert_array_equal(comp.cpu().numpy(), kernel)
        # the public call: the strided view goes through as it is (16-byte rows), the kernel writes in place
        s = sched.clone()
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert M.mine_negatives(emb, s, index, hardness, n_changed=cnt) is s
        np.testing.assert_array_equal(s.cpu().numpy(), MC.expected(i, mode))
        assert int(cnt) == MR.changed(c.sched, MC.expected(i, mode))


def test_rows_wider_than_the_kernel_takes_go_through_the_composition():
    from two_stage_gnn_amd import _native as nat, mining as M
    rng = np.random.default_rng(3)
    G, dim = 40, 1028
    emb = rng.integers(-2, 3, size=(G, dim)).astype(np.float32)
    class_of = np.repeat([0, 1], 20).astype(np.int32)
    members = np.concatenate([rng.permutation(20), 20 + rng.permutation(20)]).astype(np.int32)
    index = M.ClassIndex(class_of, [0, 20, 40], members, "ab")
    sched = np.stack([np.arange(20), rng.integers(0, 20, 20), rng.integers(20, 40, 20)], 1).astype(np.int32)
    x = _dev(emb)
    assert not M.kernel_ok(x, index)
    for mode, _, hardness in MODES:
        s = _dev(sched)
        nat.trace = []
        try:
            M.mine_negatives(x, s, index, hardness)
            assert nat.trace == []
        finally:
            nat.trace = None
        np.testing.assert_array_equal(s.cpu().numpy(), MR.mine_int(emb, sched, class_of, index.class_ptr, members, mode))


def test_unaligned_embeddings_are_copied_to_16_byte_rows():
    """a [G, 5] tensor (stride 5: rows off 16 bytes) is what ``two_stage._rows16`` exists for"""
    from two_stage_gnn_amd import mining as M
    i = 2                                                                          # dim 5
    c = MC.build(i)
    index = M.ClassIndex(c.class_of, c.class_ptr, c.members, range(c.C))
    emb = _dev(c.emb)
    assert emb.stride(0) == 5
    s = _dev(c.sched)
    M.mine_negatives(emb, s, index, 2)
    np.testing.assert_array_equal(s.cpu().numpy(), MC.expected(i, MR.HARDEST))


# ------------------------------------------------------------------------------------------------ (e) through the streams
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _sage():
    import triplet_stream_util as U
    from two_stage_gnn_amd import dense_encoders as E, triplet, triplet_stream
    from two_stage_gnn_amd.triplet import MarginRankingLoss

    class A:
        bias = True
    torch.manual_seed(6)
    m = E.GcnEncoderGraph(U.FIN, 128, 128, 2, 3, bn=True, args=A(), final_dim="output_dim")
    with torch.no_grad():
        m.map_model.weight.mul_(0.25)                        # distances of a few units: the margin-10 hinge is active
    m = m.cuda()
    graphs = U.dataset()
    net = triplet.tripletnet(m)
    classes = {"even": [graphs[i] for i in (4, 0, 6, 2)], "odd": [graphs[i] for i in (5, 1, 3)]}
    sched = np.array([[0, 2, 1], [1, 5, 0], [2, 4, 3], [3, 1, 6], [4, 6, 5], [5, 3, 2], [6, 0, 1]], dtype=np.int64)
    crit, tgt = MarginRankingLoss(margin=10.0), torch.tensor([-1.0]).cuda()
    return m, net, triplet.tripletnet, graphs, triplet_stream.TripletStream(net, graphs), classes, sched, crit, tgt


def _gat():
    import gat_stream_util as U
    from two_stage_gnn_amd import gat_stream, gat_triplet
    m = U.model("small8", "l2", "train")
    objs = U.dataset("small8")
    net = gat_triplet.tripletnet(m)
    classes = {0: [objs[i] for i in (5, 0, 3, 1, 4, 2)], 1: [objs[i] for i in (10, 6, 9, 7, 8)]}
    sched = np.array([[0, 1, 6], [6, 7, 2], [2, 3, 8], [8, 9, 4], [4, 5, 10], [10, 6, 0], [1, 0, 7], [3, 2, 9]], dtype=np.int64)
    crit, tgt = gat_triplet.MarginRankingLoss(margin=U.MARGIN), torch.full((1,), -1.0, device="cuda")
    return m, net, gat_triplet.tripletnet, objs, gat_stream.TripletStream(net, objs), classes, sched, crit, tgt


@pytest.mark.parametrize("family", ["sage", "gat"])
def test_mined_epochs_through_a_graphed_step(family):
    from two_stage_gnn_amd import mining as M, two_stage
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    from two_stage_gnn_amd.triplet_stream import HEAD
    m, net, tripletnet, graphs, st, classes, sched, crit, tgt = (_sage if family == "sage" else _gat)()
    index = M.class_index(classes, graphs)
    T = len(sched)
    m2 = copy.deepcopy(m)                                     # the eager drop-in's model: the stream's parameters before every step
    net2 = tripletnet(m2)
    held = {}

    def step():
        out = st.embed()
        held["out"] = out                                     # (the capture's own output tensors: every replay rewrites them)
        return crit(out[0], out[1], tgt)
    with pytest.raises(RuntimeError, match="load"):
        st.mine(torch.zeros(len(graphs), 8, device="cuda"), index, 1)
    st.load(sched)
    gs = GraphedStep(FlatTrainer(m, lr=1e-3, clip=2.0), step)
    total_changed = 0
    for hardness, mode in ((1, MR.HARDEST), (0.5, MR.SEMI_HARD)):   # the second round: a second load + mine on the same captured step
        emb = two_stage.embed_dataset(net, graphs)
        assert emb.shape[0] == len(graphs) and emb.is_cuda
        assert st.load(sched) == T
        before = st._sched.clone()
        assert st.mine(emb, index, 0) is None and int(st.mine(emb, index, 0, count=True)) == 0
        assert torch.equal(st._sched, before)                 # hardness 0 leaves the buffer alone
        with pytest.raises(RuntimeError, match="graphs"):
            st.mine(emb[:-1], index, hardness)
        cnt = st.mine(emb, index, hardness, count=True)
        after = st._sched.cpu().numpy()
        assert np.array_equal(after[:HEAD], before.cpu().numpy()[:HEAD]) and np.array_equal(after[HEAD + 3 * T:], before.cpu().numpy()[HEAD + 3 * T:])
        mined = after[HEAD:HEAD + 3 * T].reshape(T, 3)
        assert np.array_equal(mined[:, :2], sched[:, :2]) and int(cnt) == MR.changed(sched, mined)
        total_changed += int(cnt)
        e64 = emb.cpu().numpy()
        ref = MR.mine(e64, sched, index.class_of, index.class_ptr, index.members, mode)
        print("%s hardness %s: mined %s (float64: %s), %d changed" % (family, hardness, mined[:, 2].tolist(), ref[:, 2].tolist(), int(cnt)))
        t = MR.tau(e64.shape[1])
        assert all(MR.acceptable(e64, sched[k], int(mined[k, 2]), index.class_of, index.class_ptr, index.members, mode, t) for k in range(T))
        assert st.position() == 0
        for k in range(T):
            m2.load_state_dict(m.state_dict())
            outd = net2(*[graphs[i] for i in mined[k]])
            torch.cuda.synchronize()
            gs.step()
            gs.synchronize()
            assert st.ids_out.tolist() == mined[k].tolist(), k
            for what, a, b in zip(("dist_p", "dist_n"), held["out"][:2], outd[:2]):
                assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (hardness, k, what, float(a), float(b))
        assert st.position() == T and np.isfinite(gs.loss_value())
    assert total_changed > 0                                  # mining did move negatives on these datasets
