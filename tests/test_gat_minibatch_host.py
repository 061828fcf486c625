"""gat_stream's mini-batch stream without a GPU: the numpy restatement of the gather launch (tests/gat_minibatch_util.launch_np) against
the block-diagonal batch written out from ``pack_host``'s pieces (``gat_triplet.assemble``'s layout) on the [:R] / [:E] / [:I] prefixes
and against the padding contract behind them, the default capacities and ``schedule_capacity`` against a brute-force loop, every
refusal of ``check_fit``, and the entry point's declaration and host-side validator, one case per return code."""
import numpy as np
import pytest

import gat_minibatch_util as M
import gat_stream_util as U
import test_gat_triplet_host as H

BS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128)


def _plain_batch(objs, ids):
    """the packed batch of ``ids`` from ``pack_host``'s dicts, graph after graph (what ``gat_triplet.assemble`` lays out)"""
    from two_stage_gnn_amd import gat_triplet as GT
    ps = [GT.pack_host(objs[int(i)]) for i in ids]
    row0 = np.concatenate([[0], np.cumsum([p["nr"] for p in ps])])
    e0 = np.concatenate([[0], np.cumsum([p["nnz"] for p in ps])])
    cat = lambda key, add: np.concatenate([p[key] + a for p, a in zip(ps, add)]).astype(np.int32)
    rp = np.concatenate([p["rowptr"][:-1] + e for p, e in zip(ps, e0)] + [[e0[-1]]]).astype(np.int32)
    rpt = np.concatenate([p["rowptr_t"][:-1] + e for p, e in zip(ps, e0)] + [[e0[-1]]]).astype(np.int32)
    mult = np.concatenate([np.where(np.arange(p["nr"]) < p["n"], 1.0, float(p["mult"])) for p in ps]).astype(np.float32)
    return {"rowptr": rp, "rowptr_t": rpt, "col": cat("col", row0), "col_t": cat("col_t", row0), "src_e_t": cat("src_e_t", e0),
            "inv": cat("inv_e_t", e0), "graph_ptr": row0.astype(np.int32), "row_graph": np.repeat(np.arange(len(ps)), [p["nr"] for p in ps]),
            "row_slot": np.concatenate([np.arange(p["nr"]) for p in ps]), "iso_idx": cat("iso_rows", row0),
            "iso_w": np.concatenate([p["iso_w"] for p in ps]).astype(np.float32).view(np.int32),
            "iso_ptr": np.concatenate([[0], np.cumsum([p["k"] for p in ps])]).astype(np.int32),
            "row_mult": mult.view(np.int32), "x": np.concatenate([p["feats"] for p in ps]).view(np.int32).reshape(-1)}


@pytest.mark.parametrize("name,B", [("mb3", 1), ("mb3", 5), ("mb8", 33), ("mb8", 65), ("mb3", 128), ("big", 3), ("big", 5)])
def test_restatement_against_the_plain_batch_and_the_padding_contract(name, B):
    from two_stage_gnn_amd import gat_stream as S
    objs = M.dataset(name)
    rec, per = M.pieces(objs)
    lab = M.labels(name)
    ldf = per[0]["ldf"]
    assert ldf == (M.FIN[name] + 3) // 4 * 4
    caps = S.default_caps(rec, B)
    for ids in M.schedule(name, B):
        need = S.entry_sums(rec, ids[None])[0]
        for cap in (caps, tuple(int(v) for v in need)):           # the default, and exactly the entry's own sums: no padding row
            if (need > np.array(cap)).any():
                continue
            Rc, Ec, Ic = cap
            got = M.launch_np(rec, per, lab, ids, Rc, Ec, Ic, ldf, [2])
            want = _plain_batch(objs, ids)
            R, E, I = (int(v) for v in need)
            for key, w in want.items():
                assert np.array_equal(got[key][:w.size], w), (key, ids[:4])
            assert (got["rowptr"][R:] == E).all() and (got["rowptr_t"][R:] == E).all()
            assert not got["x"][R * ldf:].any() and not got["row_mult"][R:].any() and not got["iso_cols2"][2 * R:].any()
            assert (got["row_graph"][R:] == B - 1).all() and not got["row_slot"][R:].any()
            assert got["graph_ptr"][B] == R and got["iso_ptr"][B] == I
            for key in ("col", "col_t", "src_e_t", "inv"):
                assert (got[key][E:] == -1).all(), key
            assert (got["iso_idx"][I:] == -1).all() and (got["iso_w"][I:] == np.int64(0x7FC0BEEF)).all()
            assert got["ids"].tolist() == ids.tolist() and got["label"].tolist() == lab[ids].tolist() and got["label"].dtype == np.int64
            # the indicator: the columns without an edge, times what they stand for, and the list of exactly those rows
            iso = got["iso_cols2"].view(np.float32).reshape(Rc, 2)[:R]
            assert np.array_equal(iso[:, 0], iso[:, 1]) and np.array_equal(np.flatnonzero(iso[:, 0]), got["iso_idx"][:I])
            assert np.array_equal(iso[got["iso_idx"][:I], 0], got["iso_w"][:I].view(np.float32))
    # an entry that does not fit writes nothing
    ids = M.schedule(name, B)[0]
    need = S.entry_sums(rec, ids[None])[0]
    for short in range(3):
        if need[short] == 0:
            continue
        cap = [int(v) for v in need]
        cap[short] -= 1
        got = M.launch_np(rec, per, lab, ids, cap[0], cap[1], cap[2], ldf, [2])
        assert all((v == -1).all() for k, v in got.items() if k in M.INT_NAMES + ["ids", "label"])
        assert all((got[k] == np.int64(0x7FC0BEEF)).all() for k in ("row_mult", "iso_w", "x", "iso_cols2"))


def test_datasets_hold_what_the_tests_need():
    from two_stage_gnn_amd import gat_stream as S
    for name in ("mb3", "mb8"):
        objs = M.dataset(name)
        rec = S.size_records(objs)
        assert len(objs) == 160 and rec.shape == (160, 3)
        ns = [int(o.graph["num_nodes"]) for o in objs]
        assert sorted(set(ns)) == list(range(1, 13)) and set(M.labels(name).tolist()) == {0, 1, 2}
        assert (rec[np.array(ns) == 12, 0] == 12).all() and (rec[np.array(ns) == 5, 0] == 6).all()      # n == Nmax: no ghost row
        assert (rec[:, 1] == 0).sum() > 13                                         # edge-less graphs beside the one-node graphs
        asym = [i for i, o in enumerate(objs) if not np.array_equal(o.graph["adj"], o.graph["adj"].T)]
        assert len(asym) > 20                                                      # directed graphs
        ar = S.pack_arena(objs, batch=1)
        assert np.array_equal(ar.records[:, 2:5], rec)
        for B in BS:
            sched = M.schedule(name, B)
            assert sched.shape == (4, B) and len(set(sched[0].tolist())) == B
            assert S.fits_mask(sched, rec, B, *S.default_caps(rec, B)).all(), B
            need = S.entry_sums(rec, sched)
            assert need[1, 0] < need[0, 0] or B == 1                               # the second entry is smaller: stale rows would show
    big = S.size_records(M.dataset("big"))
    assert big[:, 0].max() * 8 > 2048 and big[:, 1].max() > 2 * 2048               # x and the entry arrays span several chunks


def test_default_capacities_and_schedule_capacity_against_a_brute_force_loop():
    from two_stage_gnn_amd import gat_stream as S
    objs = M.dataset("mb3")
    rec = S.size_records(objs)
    ar = S.pack_arena(objs, batch=1)
    for B in (1, 3, 32, 128):
        want = tuple(sum(sorted(rec[:, c].tolist(), reverse=True)[:B]) for c in range(3))
        assert S.default_caps(rec, B) == want == S.default_caps(ar.records, B)     # (an arena's records [G, 8] serve as well)
        sched = M.schedule("mb3", B)
        top = [0, 0, 0]
        for ids in sched:
            for c in range(3):
                top[c] = max(top[c], sum(int(rec[i, c]) for i in ids))
        floor = [int(rec[:, c].max()) for c in range(3)]
        got = S.schedule_capacity(rec, sched)
        assert got == {"row_cap": max(top[0], floor[0]), "nnz_cap": max(top[1], floor[1]), "iso_cap": max(top[2], floor[2])}
        assert S.fits_mask(sched, rec, B, **got).all()
        assert all(got[k] <= d for k, d in zip(("row_cap", "nnz_cap", "iso_cap"), want))
    few = rec[:5]                                                                  # fewer graphs than the batch: the largest stands in
    assert S.default_caps(few, 8) == tuple(int(few[:, c].sum() + 3 * few[:, c].max()) for c in range(3))
    lone = np.array([[0, 0]], dtype=np.int64)                                      # never below the largest piece
    assert S.schedule_capacity(rec, lone) == {"row_cap": int(rec[:, 0].max()), "nnz_cap": int(rec[:, 1].max()), "iso_cap": int(rec[:, 2].max())}
    with pytest.raises(ValueError, match="records"):
        S.default_caps(np.zeros((4, 5)), 2)


def test_check_fit_refusals():
    from two_stage_gnn_amd import gat_stream as S
    rec = S.size_records(M.dataset("mb3"))
    B = 4
    caps = S.default_caps(rec, B)
    good = M.schedule("mb3", B)
    assert S.check_fit(good, rec, B, *caps).dtype == np.int32 and S.check_fit(good, rec, B, *caps).tolist() == good.tolist()
    for bad, what in ((np.zeros((4, 3), dtype=np.int64), "shape"), (np.zeros((0, 4), dtype=np.int64), "shape"),
                      (np.zeros(4, dtype=np.int64), "shape"), (np.zeros((2, 4)), "integer"),
                      (np.array([[0, 1, 2, -1]]), "indices"), (np.array([[0, 1, 2, 160]]), "indices")):
        with pytest.raises(ValueError, match=what):
            S.check_fit(bad, rec, B, *caps)
        with pytest.raises(ValueError, match=what):
            S.fits_mask(bad, rec, B, *caps)
    big = int(np.argmax(rec[:, 0] * (1 << 20) + rec[:, 1]))                        # the largest graph four times: past the default capacity
    over = np.array([good[0], [big] * B, good[1]])
    assert S.fits_mask(over, rec, B, *caps).tolist() == [True, False, True]
    with pytest.raises(ValueError, match="schedule entry 1 has %d rows.*capacity.*eager route" % (B * rec[big, 0])):
        S.check_fit(over, rec, B, *caps)
    need = S.entry_sums(rec, good)
    for c, name in enumerate(("row_cap", "nnz_cap", "iso_cap")):                   # each capacity on its own refuses
        kk = int(np.argmax(need[:, c]))
        cap = list(caps)
        cap[c] = int(need[kk, c]) - 1
        first = int(np.flatnonzero(need[:, c] > cap[c])[0])
        with pytest.raises(ValueError, match="schedule entry %d .*%s %d" % (first, name, cap[c])):
            S.check_fit(good, rec, B, *cap)
        cap[c] += 1
        assert S.fits_mask(good[kk:kk + 1], rec, B, *cap).all()


def test_entry_point_is_declared_and_validates_on_the_host():
    """fails where the symbol does not exist: TSGNN_EINVAL (-1) for null pointers, B outside 1..128, a header whose B differs, capacities
    below one largest piece; TSGNN_EUNSUPPORTED (-3) for the int32 limits, the alignments and a grid of 2^31 workgroups"""
    from two_stage_gnn_amd import _native as nat
    decl = nat.parse_header()
    assert "tsgnn_gat_batch_gather_f32" in decl
    names = [n for _, n in decl["tsgnn_gat_batch_gather_f32"][1]]
    assert names == ["records", "n_graphs", "arena", "arena_words", "max_nr", "max_nnz", "max_k", "labels", "sched", "sched_cap", "state",
                     "ticket", "B", "desc", "ids_out", "label_out", "stream"]
    old = [n for _, n in decl["tsgnn_gat_triplet_gather_f32"][1]]
    assert [n for n in names if n not in ("B", "labels", "label_out")] == old
    L = nat.lib()
    P = 1 << 20                                                                    # (pointers are only tested here, never followed)
    d = H._desc(K=0, R=36, E=90, I=12, B=5)
    call = lambda d_=d, rec=P, n=4, ar=P, words=100, nr=12, nnz=30, k=4, lab=P, sched=P, cap=5, state=P, tk=P, B=5, ids=P, lo=P: \
        L.tsgnn_gat_batch_gather_f32(rec, n, ar, words, nr, nnz, k, lab, sched, cap, state, tk, B, d_.ctypes.data if d_ is not None else None,
                                     ids, lo, None)
    for kw in ("rec", "ar", "lab", "sched", "state", "tk", "ids", "lo", "d_"):      # a null pointer
        assert call(**{kw: None}) == -1, kw
    assert call(B=0) == -1 and call(B=129) == -1 and call(B=-3) == -1              # B outside 1..128
    assert call(B=4) == -1 and call(d_=H._desc(K=0, R=36, E=90, I=12, B=3)) == -1  # a header whose B differs
    assert call(n=0) == -1 and call(cap=0) == -1 and call(nr=0) == -1 and call(nnz=-1) == -1 and call(k=13) == -1 and call(words=0) == -1
    assert call(nr=37) == -1 and call(nnz=91) == -1 and call(k=13, nr=13) == -1    # a capacity below ONE largest piece
    assert call(d_=H._desc(K=0, R=36, E=90, I=12, B=5, ldf=6)) == -1               # rows off 16 bytes
    miss = H._desc(K=0, R=36, E=90, I=12, B=5)
    miss[19] = 0
    assert call(d_=miss) == -1                                                     # a missing output
    # capacities of ONE largest piece pass the validator's capacity check (the next refusal is an alignment)
    assert call(d_=H._desc(K=0, R=12, E=30, I=4, B=5), rec=P + 4) == -3
    assert call(rec=P + 4) == -3 and call(ar=P + 8) == -3 and call(state=P + 8) == -3 and call(lo=P + 4) == -3      # off 16 / 8 bytes
    assert call(words=1 << 31) == -3 and call(cap=(1 << 31) // 5) == -3            # the int32 limits
    wide = H._desc(K=0, R=1 << 28, E=90, I=12, B=5, ldf=8)
    assert call(d_=wide) == -3                                                     # R ldf reaches 2^31
    huge = H._desc(K=0, R=(1 << 29) - 8, E=1 << 30, I=12, B=128)
    assert call(d_=huge, B=128, nr=1 << 24, nnz=0) == -3                           # B max_nr reaches 2^31
    assert call(d_=huge, B=128, nr=12, nnz=1 << 24) == -3                          # B max_nnz reaches 2^31
    # (a grid of 2^31 workgroups lies behind these limits: R ldf < 2^31 and B max_nnz < 2^31 keep a piece below 2^23 chunks, so the
    # entry point's own grid refusal cannot be reached from outside and has no case here)
