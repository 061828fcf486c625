"""Host side of hard / semi-hard negative mining (two_stage_gnn_amd/mining.py, ArenaStream.mine, the entry point's refusals), no GPU.

The fixtures tests/golden/mining_{dense,sag}.npz hold what the reference's own samplers mined (scripts/gen_golden_mining.py):
tests/mining_ref.py must reproduce them exactly, and so must ``mine_negatives_torch`` on CPU tensors."""
import numpy as np
import pytest
import torch

import mining_ref as MR
from conftest import load_golden

FIXTURES = ["mining_dense", "mining_sag"]
MODES = [(MR.SEMI_HARD, "semi", 0.5), (MR.HARDEST, "hardest", 1)]


def _m():
    from two_stage_gnn_amd import mining
    return mining


def epochs(z):
    """-> [(rows of the epoch, its member list)]"""
    return [(np.flatnonzero(z["epoch_of"] == ep), z["members"][ep]) for ep in range(z["members"].shape[0])]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_what_the_generator_promises(name):
    z = load_golden(name)
    X = z["emb"]
    assert X.dtype == np.float32 and X.shape[1] == 24 and np.array_equal(X * 8, np.rint(X * 8)) and np.abs(X).max() <= 4
    assert np.array_equal(z["drawn"][:, :2], z["semi"][:, :2]) and np.array_equal(z["drawn"][:, :2], z["hardest"][:, :2])
    assert MR.changed(z["drawn"], z["semi"]) > 0 and MR.changed(z["drawn"], z["hardest"]) > 0
    th = ts = 0
    for rows, members in epochs(z):
        h, s = MR.tie_counts(X, z["drawn"][rows], z["class_of"], z["class_ptr"], members)
        th, ts = th + h, ts + s
    assert th >= 5 and ts >= 5 and [th, ts] == z["ties"].tolist()
    assert len(np.unique(X, axis=0)) < X.shape[0]                                  # identical rows exist


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode,key,hardness", MODES)
def test_mining_ref_reproduces_the_reference(name, mode, key, hardness):
    z = load_golden(name)
    for rows, members in epochs(z):
        args = (z["emb"], z["drawn"][rows], z["class_of"], z["class_ptr"], members, mode)
        want = z[key][rows]
        np.testing.assert_array_equal(MR.mine(*args), want)
        np.testing.assert_array_equal(MR.mine_loop(*args), want)
        np.testing.assert_array_equal(MR.mine_int(z["emb"] * 8, *args[1:]), want)
    with pytest.raises(ValueError):
        MR.mine_int(z["emb"] * 3, *args[1:])


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode,key,hardness", MODES)
def test_mine_negatives_torch_on_cpu_tensors(name, mode, key, hardness):
    M = _m()
    z = load_golden(name)
    emb = torch.from_numpy(z["emb"])
    for rows, members in epochs(z):
        index = M.ClassIndex(z["class_of"], z["class_ptr"], members, range(z["class_ptr"].size - 1))
        sched = torch.from_numpy(np.ascontiguousarray(z["drawn"][rows]))
        before = sched.clone()
        got = M.mine_negatives_torch(emb, sched, index, hardness, block=7)
        assert got.dtype == torch.int32 and torch.equal(sched, before)            # the schedule is not written
        np.testing.assert_array_equal(got.numpy(), z[key][rows][:, 2])
        cnt = torch.zeros(1, dtype=torch.int32)
        out = M.mine_negatives(emb, sched, index, hardness, n_changed=cnt)         # CPU tensors: the composition, in place
        assert out is sched
        np.testing.assert_array_equal(sched.numpy(), z[key][rows])
        assert int(cnt) == MR.changed(z["drawn"][rows], z[key][rows])
    same = before.clone()
    assert M.mine_negatives(emb, same, index, 0) is same and torch.equal(same, before)


def test_hardness_dispatch_is_the_references():
    M = _m()
    assert [M.mode_of(h) for h in (0, 0.0, -1, 0.5, 1, 1.0, 0.25, 2, 0.7)] == [0, 0, 0, 1, 2, 2, 2, 2, 2]


class Obj:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "Obj(%s)" % self.name


def test_class_index_against_hand_built_dictionaries():
    M = _m()
    g = [Obj(i) for i in range(7)]
    ci = M.class_index({"b": [g[4], g[0], g[6]], "a": [g[5]], "empty": [], "c": [g[2], g[1]]}, g)
    assert ci.keys == ["b", "a", "empty", "c"] and ci.n_graphs == 7 and ci.n_classes == 4
    assert ci.class_of.dtype == ci.class_ptr.dtype == ci.members.dtype == np.int32
    assert ci.class_of.tolist() == [0, 3, 3, -1, 0, 1, 0]                          # graph 3 is in no list
    assert ci.class_ptr.tolist() == [0, 3, 4, 4, 6] and ci.members.tolist() == [4, 0, 6, 5, 2, 1]
    # identity, not equality: an equal-looking other object is not the dataset's
    twin = Obj(0)
    with pytest.raises(ValueError, match=r"Obj\(0\)"):
        M.class_index({"a": [g[1]], "b": [twin]}, g)
    with pytest.raises(ValueError, match=r"Obj\(2\).*'a'.*'b'"):
        M.class_index({"a": [g[1], g[2]], "b": [g[2]]}, g)
    with pytest.raises(ValueError, match=r"Obj\(1\)"):
        M.class_index({"a": [g[1], g[1]], "b": [g[2]]}, g)
    with pytest.raises(ValueError, match="two classes"):
        M.class_index({"a": [g[1], g[2]]}, g)
    with pytest.raises(ValueError, match="two classes"):
        M.class_index({}, g)


def test_class_index_follows_the_samplers_list_order():
    """after ``schedule_of`` has drained a sampler its lists are in the epoch's order; the index must carry that order"""
    from two_stage_gnn_amd import triplet_stream as TS
    M = _m()
    g = [Obj(i) for i in range(6)]

    class Sampler:
        def __init__(self):
            self.graphs = {0: [g[0], g[1], g[2]], 1: [g[3], g[4], g[5]]}
            self.i = 0

        def shuffle(self):
            self.graphs[0].reverse(); self.graphs[1].reverse()
            self.i = 0

        def end(self):
            return self.i >= 2

        def sampler(self):
            self.i += 1
            return {"anchor": self.graphs[0][0], "pos": self.graphs[0][1], "neg": self.graphs[1][self.i]}
    s = Sampler()
    assert TS.schedule_of(s, g).tolist() == [[2, 1, 4], [2, 1, 3]]
    assert M.class_index(s.graphs, g).members.tolist() == [2, 1, 0, 5, 4, 3]


def test_mine_negatives_checks_its_arguments():
    M = _m()
    ci = M.ClassIndex([0, 0, 1, 1], [0, 2, 4], [0, 1, 2, 3], "ab")
    emb, s = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for bad_emb, bad_s in ((torch.zeros(3, 3), s), (torch.zeros(4), s), (emb, torch.zeros(2, 3, dtype=torch.int64)),
                           (emb, torch.zeros(2, 2, dtype=torch.int32)), (emb, torch.zeros(0, 3, dtype=torch.int32)),
                           (emb, torch.zeros(3, 2, dtype=torch.int32).t())):
        with pytest.raises(ValueError):
            M.mine_negatives(bad_emb, bad_s, ci, 1)


def test_entry_point_is_declared_and_validates_on_the_host():
    from two_stage_gnn_amd import _native as nat
    decl = nat.parse_header()
    assert [n for _, n in decl["tsgnn_mine_negatives_f32"][1]] == ["emb", "ld", "n_graphs", "dim", "class_of", "class_ptr", "members",
                                                                   "n_classes", "sched", "T", "mode", "n_changed", "stream"]
    assert [n for _, n in decl["tsgnn_mine_supported"][1]] == ["dim", "n_classes"]
    L = nat.lib()
    assert L.tsgnn_mine_supported(1, 2) == 1 and L.tsgnn_mine_supported(1024, 3) == 1
    assert L.tsgnn_mine_supported(1025, 2) == 0 and L.tsgnn_mine_supported(0, 2) == 0 and L.tsgnn_mine_supported(8, 1) == 0
    P = 1 << 20                                                                # (pointers are only tested here, never followed)
    call = lambda emb=P, ld=8, G=10, dim=6, cof=P, cptr=P, mem=P, C=2, sched=P, T=5, mode=1, cnt=None: \
        L.tsgnn_mine_negatives_f32(emb, ld, G, dim, cof, cptr, mem, C, sched, T, mode, cnt, None)
    EINVAL, EUNSUPPORTED = -1, -3
    assert call(emb=None) == EINVAL and call(cof=None) == EINVAL and call(cptr=None) == EINVAL and call(mem=None) == EINVAL
    assert call(sched=None) == EINVAL
    assert call(T=0) == EINVAL and call(T=-1) == EINVAL and call(G=0) == EINVAL and call(C=1) == EINVAL and call(dim=0) == EINVAL
    assert call(mode=0) == EINVAL and call(mode=3) == EINVAL and call(mode=-1) == EINVAL
    assert call(ld=4) == EINVAL and call(ld=5, dim=6) == EINVAL                # ld < dim
    assert call(emb=P + 4) == EUNSUPPORTED and call(emb=P + 8) == EUNSUPPORTED  # off 16 bytes
    assert call(ld=6) == EUNSUPPORTED and call(ld=7) == EUNSUPPORTED            # ld % 4
    assert call(ld=1028, dim=1025) == EUNSUPPORTED                              # past the widest row
    assert call(G=1 << 31) == EUNSUPPORTED and call(T=(1 << 31) // 3 + 1) == EUNSUPPORTED


def test_arena_stream_mine_refuses_without_a_device():
    from two_stage_gnn_amd import triplet_stream as TS, post_train as PT
    M = _m()
    ci = M.ClassIndex([0, 0, 1, 1], [0, 2, 4], [0, 1, 2, 3], "ab")
    emb = torch.zeros(4, 8)
    s = TS.TripletStream.__new__(TS.TripletStream)
    s.B, s._sched, s.T, s.arena, s.device = 3, None, 0, TS.Arena(n_graphs=4), torch.device("cpu")
    with pytest.raises(RuntimeError, match="load"):
        s.mine(emb, ci, 1)
    s._sched, s.T = torch.zeros(TS.HEAD + 6, dtype=torch.int32), 2
    with pytest.raises(RuntimeError, match="4 graphs"):
        s.mine(torch.zeros(3, 8), ci, 1)
    with pytest.raises(RuntimeError, match="4 graphs"):
        s.mine(torch.zeros(8), ci, 1)
    with pytest.raises(ValueError, match="class index"):
        s.mine(torch.zeros(5, 8), M.ClassIndex([0, 0, 1, 1, 1], [0, 2, 5], [0, 1, 2, 3, 4], "ab"), 1)
    p = PT.PostTrainStream.__new__(PT.PostTrainStream)
    p.B, p._sched, p.T, p.arena, p.device = 1, torch.zeros(TS.HEAD + 2, dtype=torch.int32), 2, TS.Arena(n_graphs=4), torch.device("cpu")
    with pytest.raises(RuntimeError, match="triplet"):
        p.mine(emb, ci, 1)


# ---------------------------------------------------------------------------- the synthetic cases the GPU file runs the kernel on
def test_synthetic_cases_cover_the_grid_and_contain_what_they_claim():
    import mining_cases as MC
    dims, sizes, ncls, Ts, found = set(), set(), set(), set(), set()
    for i, (dim, sz, T, kind) in enumerate(MC.CASES):
        c = MC.build(i)
        dims.add(dim); sizes.update(sz); ncls.add(len(sz)); Ts.add(T)
        assert c.emb.shape == (sum(sz), dim) and np.array_equal(c.emb, np.rint(c.emb)) and np.abs(c.emb).max() < 512        # (squares sum far below 2^24)
        for k in range(c.C):
            lst = c.members[c.class_ptr[k]:c.class_ptr[k + 1]]
            assert sorted(lst.tolist()) == list(range(c.class_ptr[k], c.class_ptr[k + 1]))
            assert lst.size == 1 or lst.tolist() != sorted(lst.tolist())          # a permutation that differs from index order
        assert (c.class_of[c.sched[:, 0]] == c.class_of[c.sched[:, 1]]).all() and (c.class_of[c.sched[:, 0]] != c.class_of[c.sched[:, 2]]).all()
        here = MC.scenarios(i)
        if kind == "crafted":
            assert here >= MC.REQUIRED, (i, MC.REQUIRED - here)
            semi, hard = MC.expected(i, MR.SEMI_HARD), MC.expected(i, MR.HARDEST)
            last = c.members[c.class_ptr[-2]:]
            want = [last[p] for p in c.special]
            assert semi[:4, 2].tolist() == want and hard[:4, 2].tolist() == want
            assert semi[4, 2] == c.sched[4, 2] and hard[5, 2] == c.sched[5, 2] and hard[6, 2] == last[1]
        found |= here
        # the three arithmetics agree on integer-valued rows
        for mode in (MR.SEMI_HARD, MR.HARDEST):
            args = (c.emb, c.sched, c.class_of, c.class_ptr, c.members, mode)
            np.testing.assert_array_equal(MR.mine(*args), MC.expected(i, mode))
            np.testing.assert_array_equal(MR.mine_f32(*args), MC.expected(i, mode))
    assert dims == {1, 3, 4, 5, 64, 130, 1024} and sizes >= {1, 2, 63, 64, 65, 129} and ncls == {2, 3} and Ts == {1, 3, 4, 5, 257}
    assert found >= MC.REQUIRED


@pytest.mark.parametrize("i", range(3))
def test_mine_negatives_torch_on_the_synthetic_cases(i):
    import mining_cases as MC
    M = _m()
    i = (2, 4, 8)[i]                                                               # three classes; T = 257; a crafted case
    c = MC.build(i)
    index = M.ClassIndex(c.class_of, c.class_ptr, c.members, range(c.C))
    for mode, hardness in ((MR.SEMI_HARD, 0.5), (MR.HARDEST, 3)):
        got = M.mine_negatives_torch(torch.from_numpy(c.emb), torch.from_numpy(c.sched), index, hardness)
        np.testing.assert_array_equal(got.numpy(), MC.expected(i, mode)[:, 2])


@pytest.mark.parametrize("seed", [5, 6])
def test_real_valued_inputs_keep_fp32_within_one_percent_of_float64(seed):
    """the condition test_gpu_mining.py puts on its real-valued inputs, checked where no GPU is needed: fp32 numpy differs from the
    float64 reference in at most 1% of the entries for the committed seeds, and every fp32 choice passes the acceptance predicate"""
    import mining_cases as MC
    assert seed in MC.REAL_SEEDS
    c = MC.real_case(seed)
    t = MR.tau(c.dim)
    assert t == 2 * 66 * 2.0 ** -24
    for mode in (MR.SEMI_HARD, MR.HARDEST):
        args = (c.emb, c.sched, c.class_of, c.class_ptr, c.members, mode)
        ref, f32 = MR.mine(*args), MR.mine_f32(*args)
        differ = MR.changed(ref, f32)
        print("seed %d mode %d: %d of %d entries differ between fp32 numpy and float64; mining changed %d" % (seed, mode, differ, c.T, MR.changed(c.sched, ref)))
        assert differ <= c.T // 100 and MR.changed(c.sched, ref) > c.T // 2
        assert all(MR.acceptable(c.emb, c.sched[k], int(f32[k, 2]), c.class_of, c.class_ptr, c.members, mode, t) for k in range(c.T))
        # the predicate is not vacuous: the drawn negative is refused wherever mining clearly changes it
        refused = sum(not MR.acceptable(c.emb, c.sched[k], int(c.sched[k, 2]), c.class_of, c.class_ptr, c.members, mode, t) for k in range(c.T))
        assert refused >= MR.changed(c.sched, ref) - c.T // 100
