"""The reference of the capacity-batch contraction kernels (tests/contract_cap_ref.py) anchored to the oracle and to float64 autograd,
and the host side of the entry points (csrc/contract_cap.hip): the envelope at its edges, the slab bound, argument checks that
return before anything is launched.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import contract_cap_ref as C
import triplet_stream_util as U
from oracle import dense_ref as R

ENTRY_POINTS = ("tsgnn_contract_cap_supported", "tsgnn_contract_cap_slabs", "tsgnn_ell_rowsum_f32", "tsgnn_contract_cap_bwd_f32")


def _case(ids, nmax, K, F, seed=3, dtype=torch.float64, row_cap=None):
    graphs = U.dataset(nmax=nmax)
    sizes = [U.SIZES[i] for i in ids]
    row_cap = (len(ids) * 48 + 31) // 32 * 32 if row_cap is None else row_cap
    adjs = [graphs[i].graph["adj"] for i in ids]
    gp = C.layout(sizes, row_cap)
    ell, tp, tc, ntail = C.neighbours(adjs, sizes, row_cap, nmax, U.ELL_W)
    gen = torch.Generator().manual_seed(seed)
    Rr, n_tot = row_cap + nmax, int(gp[len(ids)])
    S = torch.rand(Rr, K, generator=gen, dtype=torch.float64)
    Z = torch.randn(Rr, F, generator=gen, dtype=torch.float64)
    S[n_tot:], Z[n_tot:] = 0, 0
    return dict(graphs=graphs, ids=ids, sizes=sizes, adjs=adjs, gp=gp, ell=ell, tp=tp, tc=tc, ntail=ntail, S=S.to(dtype), Z=Z.to(dtype),
                row_cap=row_cap, nmax=nmax, n_tot=n_tot, B=len(ids), gen=gen)


@pytest.mark.parametrize("ids,nmax", [([0, 2, 4], 48), ([1, 5, 3], 64), ([1, 1, 1], 48), ([0], 64)])
def test_reference_equals_the_oracle_contraction_graph_by_graph(ids, nmax):
    c = _case(ids, nmax, 12, 20)
    assert (c["ntail"] > 0) == (0 in ids)
    AS = C.rowsum(c["ell"], c["tp"], c["tc"], c["n_tot"], c["S"])
    xo, ao, ro, arg = C.forward(c["S"], c["Z"], AS, c["gp"], c["B"], c["row_cap"], nmax)
    for b, (i, n) in enumerate(zip(ids, c["sizes"])):
        r0 = int(c["gp"][b])
        a = torch.from_numpy(c["adjs"][b][:n, :n]).double()[None]
        x_ref, a_ref = R.diffpool_contract(c["S"][r0:r0 + n][None], c["Z"][r0:r0 + n][None], a)
        torch.testing.assert_close(xo[b], x_ref[0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ao[b], a_ref[0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(AS[r0:r0 + n], a[0] @ c["S"][r0:r0 + n], rtol=1e-12, atol=1e-12)
        # the readout: the max over the reference's masked [nmax, F] embeddings (encoders.py:353), padded slots being zero rows
        zp = torch.zeros(nmax, c["Z"].size(1), dtype=torch.float64)
        zp[:n] = c["Z"][r0:r0 + n]
        val, idx = zp.max(dim=0)
        assert torch.equal(ro[b], val)
        want = torch.where(idx < n, idx + r0, torch.full_like(idx, c["row_cap"] + n))
        assert torch.equal(arg[b].long(), want)
    assert not AS[c["n_tot"]:].any()


@pytest.mark.parametrize("ids,nmax", [([0, 2, 4], 64), ([1, 1, 1], 48), ([0], 48)])
def test_reference_backward_equals_float64_autograd(ids, nmax):
    """autograd through the DENSE formulation A' = S^T A S (two uses of S): its gradient is the reference's AS (dA' + dA'^T) — the
    identity the backward kernel rests on (A = A^T, unit weights) — and through the max readout with its zero ghost row"""
    c = _case(ids, nmax, 8, 12)
    K, F, B = 8, 12, c["B"]
    c["Z"][int(c["gp"][0]):int(c["gp"][1]), 0] = -c["Z"][int(c["gp"][0]):int(c["gp"][1]), 0].abs() - 0.1    # column 0 of graph 0: all negative
    S, Z = c["S"].clone().requires_grad_(True), c["Z"].clone().requires_grad_(True)
    gx, ga, gr = (torch.randn(B, K, F, generator=c["gen"], dtype=torch.float64), torch.randn(B, K, K, generator=c["gen"], dtype=torch.float64),
                  torch.randn(B, F, generator=c["gen"], dtype=torch.float64))
    loss = 0
    ghost_wins = real_wins = 0
    for b, n in enumerate(c["sizes"]):
        r0 = int(c["gp"][b])
        a = torch.from_numpy(c["adjs"][b][:n, :n]).double()
        assert torch.equal(a, a.t()) and set(a.unique().tolist()) <= {0.0, 1.0}
        x_b, a_b = R.diffpool_contract(S[r0:r0 + n][None], Z[r0:r0 + n][None], a[None])
        zp = torch.cat([Z[r0:r0 + n], torch.zeros(nmax - n, F, dtype=torch.float64)])
        loss = loss + (x_b[0] * gx[b]).sum() + (a_b[0] * ga[b]).sum() + (zp.max(dim=0)[0] * gr[b]).sum()
    loss.backward()
    AS = C.rowsum(c["ell"], c["tp"], c["tc"], c["n_tot"], c["S"])
    _, _, _, arg = C.forward(c["S"], c["Z"], AS, c["gp"], B, c["row_cap"], nmax)
    for b, n in enumerate(c["sizes"]):
        ghost_wins += int((arg[b] >= c["row_cap"]).sum())
        real_wins += int((arg[b] < c["row_cap"]).sum())
    assert real_wins > 0 and (ghost_wins > 0) == (c["sizes"][0] < nmax)
    dZ, dS = C.backward(c["S"], c["Z"], AS, gx, ga, c["gp"], B, dro=gr, arg=arg)
    torch.testing.assert_close(dZ, Z.grad, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(dS, S.grad, rtol=1e-11, atol=1e-11)
    assert not dZ[c["n_tot"]:].any() and not dS[c["n_tot"]:].any()
    dZ0, _ = C.backward(c["S"], c["Z"], AS, gx, ga, c["gp"], B)
    assert not torch.equal(dZ0, dZ)


def test_header_declares_and_library_exports_the_entry_points():
    from two_stage_gnn_amd import _native as nat
    decls = nat.parse_header()
    nat.build()
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in decls, name
        assert hasattr(L, name), name
    assert [p[1] for p in decls["tsgnn_contract_cap_supported"][1]] == ["K", "F"]
    assert [p[1] for p in decls["tsgnn_contract_cap_slabs"][1]] == ["row_cap", "B"]


def test_envelope_at_its_edges():
    from two_stage_gnn_amd import _native as nat
    ok = nat.lib().tsgnn_contract_cap_supported
    assert ok(4, 4) == 1 and ok(128, 384) == 1 and ok(100, 384) == 1 and ok(12, 96) == 1 and ok(100, 192) == 1
    assert ok(0, 4) == 0 and ok(4, 0) == 0 and ok(-4, 4) == 0
    assert ok(132, 384) == 0 and ok(128, 388) == 0 and ok(6, 96) == 0 and ok(12, 98) == 0 and ok(2, 4) == 0 and ok(4, 2) == 0
    # the consumer's range (dense_stack_pg takes [B, K, F] of the result at every accepted (K, F))
    pg = nat.lib().tsgnn_dense_pg_supported
    assert all(pg(3, K, F, 64) == 1 for K, F in ((4, 4), (128, 384), (100, 192)))


@pytest.mark.parametrize("sizes", [[1, 1, 1], [33, 33, 33], [48, 1, 33], [32, 32, 32], [1], [96], [31, 33, 32, 1, 64, 2, 5, 28]])
def test_slab_bound_covers_every_batch(sizes):
    from two_stage_gnn_amd import _native as nat
    slabs = nat.lib().tsgnn_contract_cap_slabs
    B, n = len(sizes), sum(sizes)
    for row_cap in (n, (n + 31) // 32 * 32, n + 100):
        bound = slabs(row_cap, B)
        assert bound == (row_cap + 31) // 32 + B
        assert C.slab_count(sizes) <= bound
    assert slabs(-1, 3) == -1 and slabs(96, 0) == -1 and slabs(96, 9) == -1


def test_invalid_arguments_return_before_any_launch():
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    rs = lambda **kw: L.tsgnn_ell_rowsum_f32(*[kw.get(k, d) for k, d in (
        ("ell", one), ("W", 16), ("tail_ptr", one), ("tail_col", one), ("tail_cap", 8), ("graph_ptr", one), ("B", 3), ("row_cap", 160),
        ("nmax", 48), ("S", one), ("ldS", 12), ("K", 12), ("out", one), ("ldo", 12), ("stream", None))])
    for bad in (dict(ell=None), dict(graph_ptr=None), dict(S=None), dict(out=None), dict(tail_col=None), dict(tail_cap=0), dict(B=0), dict(B=9),
                dict(row_cap=0), dict(nmax=0), dict(W=12), dict(K=0)):
        assert rs(**bad) == -1, bad
    for bad in (dict(K=132, ldS=132, ldo=132), dict(K=10), dict(ldS=8), dict(ldo=8), dict(ldS=13), dict(S=odd), dict(out=odd), dict(ell=odd)):
        assert rs(**bad) == -3, bad
    bw = lambda **kw: L.tsgnn_contract_cap_bwd_f32(*[kw.get(k, d) for k, d in (
        ("S", one), ("ldS", 12), ("Z", one), ("ldZ", 96), ("AS", one), ("ldAS", 12), ("dxo", one), ("dao", one), ("graph_ptr", one), ("B", 3),
        ("K", 12), ("F", 96), ("row_cap", 160), ("nmax", 48), ("dZ", one), ("lddZ", 96), ("dS", one), ("lddS", 12), ("ro_dout", None),
        ("ro_ldo", 0), ("ro_arg", None), ("split", 0), ("stream", None))])
    for bad in (dict(S=None), dict(Z=None), dict(AS=None), dict(dxo=None), dict(dao=None), dict(graph_ptr=None), dict(dZ=None), dict(dS=None),
                dict(B=0), dict(B=9), dict(row_cap=0), dict(nmax=0), dict(split=-1), dict(split=5), dict(ro_dout=one), dict(ro_arg=one),
                dict(ro_dout=one, ro_arg=one, ro_ldo=95)):
        assert bw(**bad) == -1, bad
    for bad in (dict(K=132, ldS=132, ldAS=132, lddS=132), dict(F=388, ldZ=388, lddZ=388), dict(K=6), dict(F=98), dict(ldS=8), dict(ldZ=92),
                dict(ldAS=8), dict(lddZ=92), dict(lddS=8), dict(ldZ=97), dict(S=odd), dict(Z=odd), dict(AS=odd), dict(dxo=odd), dict(dao=odd),
                dict(dZ=odd), dict(dS=odd)):
        assert bw(**bad) == -3, bad
