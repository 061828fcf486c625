"""The capacity-batch contraction kernels (csrc/contract_cap.hip) one by one through the C ABI against tests/contract_cap_ref.py
(float64; the bound is tests/fp32_yardstick.py's 8 x the reference's own fp32 rounding), on capacity layouts built from the graphs
of tests/triplet_stream_util.py: sizes [48, 1, 33], [1, 1, 1] and the graph with a CSR tail alone (B = 1); nmax 48 (the largest
graph fills every slot: ghost_slots = nmax) and 64 (ghost_slots = 49 < nmax); (K, F) at a partial MFMA tile and at both ends of
the envelope.  Every output sits in a guarded buffer with a leading dimension wider than its rows; the padding rows of S, Z and AS
hold NaN; rows >= n_tot of AS, dS and dZ must be bitwise zero; a second run, and every `split`, must give the same bits."""
import functools

import numpy as np
import pytest
import torch

import contract_cap_ref as C
import fp32_yardstick as Y
import guard_buf as G
import triplet_stream_util as U

pytestmark = pytest.mark.gpu

KF = [(4, 4), (12, 96), (16, 96), (100, 192), (100, 384), (128, 384)]
BATCHES = {"48-1-33": [0, 1, 2], "1-1-1": [1, 1, 1], "tail-b1": [0]}
CASES = [(name, nmax, K, F) for name in BATCHES for nmax in (48, 64) for K, F in KF]
PAD = 4                                 # floats of leading dimension beyond the row, in every output


def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


@functools.lru_cache(maxsize=None)
def _dataset(nmax):
    return U.dataset(nmax=nmax)


@functools.lru_cache(maxsize=None)
def _case(name, nmax, K, F):
    """inputs (float32, CPU), the layout, and the reference in float64 and in float32 — computed once, shared by the tests, never
    modified"""
    ids = BATCHES[name]
    graphs = _dataset(nmax)
    sizes = [U.SIZES[i] for i in ids]
    B = len(ids)
    row_cap = (B * 48 + 31) // 32 * 32
    gp = C.layout(sizes, row_cap)
    ell, tp, tc, ntail = C.neighbours([graphs[i].graph["adj"] for i in ids], sizes, row_cap, nmax, U.ELL_W)
    assert (ntail > 0) == (0 in ids)
    R, n_tot = row_cap + nmax, int(gp[B])
    gen = torch.Generator().manual_seed(1000 * K + F + nmax + len(name))
    S = torch.softmax(torch.randn(R, K, generator=gen), dim=1)
    Z = torch.randn(R, F, generator=gen)
    for b in range(B):
        Z[int(gp[b]):int(gp[b + 1]), 0] = -Z[int(gp[b]):int(gp[b + 1]), 0].abs() - 0.1      # column 0: no real row beats the zero ghost row
    S[n_tot:], Z[n_tot:] = 0, 0                                                              # (the ghost rows of masked operands)
    dxo, dao, dro = torch.randn(B, K, F, generator=gen), torch.randn(B, K, K, generator=gen), torch.randn(B, F, generator=gen)
    ref = {}
    for dt in (torch.float64, torch.float32):
        s, z = S.to(dt), Z.to(dt)
        AS = C.rowsum(ell, tp, tc, n_tot, s)
        xo, ao, ro, arg = C.forward(s, z, AS, gp, B, row_cap, nmax)
        dZ, dS = C.backward(s, z, AS, dxo.to(dt), dao.to(dt), gp, B, dro=dro.to(dt), arg=arg)
        dZ0, _ = C.backward(s, z, AS, dxo.to(dt), dao.to(dt), gp, B)
        ref[dt] = dict(AS=AS, xo=xo, ao=ao, ro=ro, arg=arg, dZ=dZ, dS=dS, dZ0=dZ0)
    assert torch.equal(ref[torch.float64]["arg"], ref[torch.float32]["arg"])
    arg = ref[torch.float64]["arg"]
    ghost, real = int((arg >= row_cap).sum()), int((arg < row_cap).sum())
    assert real > 0 and (ghost > 0) == any(n < nmax for n in sizes)          # a ghost-row winner and a real winner
    return dict(ids=ids, sizes=sizes, B=B, row_cap=row_cap, nmax=nmax, R=R, n_tot=n_tot, gp=gp, ell=ell, tp=tp, tc=tc, S=S, Z=Z,
                dxo=dxo, dao=dao, dro=dro, r64=ref[torch.float64], r32=ref[torch.float32])


def _device_inputs(c):
    """S, Z, AS (the float32 reference's) with NaN in the padding rows [n_tot, row_cap), the layout and the neighbour arrays"""
    n_tot, row_cap = c["n_tot"], c["row_cap"]
    out = {}
    for k, t in (("S", c["S"]), ("Z", c["Z"]), ("AS", c["r32"]["AS"])):
        t = t.clone()
        t[n_tot:row_cap] = float("nan")
        out[k] = t.cuda()
    for k in ("gp", "ell", "tp", "tc"):
        out[k] = torch.from_numpy(np.ascontiguousarray(c[k])).cuda()
    return out


def _all(rows, ld, cols):
    return G._owned(rows, ld, 0, rows, 0, cols)


def _zero_bits(out, r0, cols):
    """rows >= r0 of the guarded buffer: every word of the row's first `cols` columns is the bit pattern of +0.0"""
    bits = out.bits[:out.rows * out.ld].view(out.rows, out.ld)[r0:, :cols]
    return not bool(bits.ne(0).any())


@pytest.mark.parametrize("name,nmax,K,F", CASES)
def test_rowsum(name, nmax, K, F):
    c = _case(name, nmax, K, F)
    d = _device_inputs(c)
    outs = []
    for _ in range(2):
        o = G.Out(c["R"], K + PAD)
        _nat().call("ell_rowsum_f32", d["ell"], U.ELL_W, d["tp"], d["tc"], d["tc"].numel(), d["gp"], c["B"], c["row_cap"], nmax, d["S"], K, K,
                    o.mat, K + PAD)
        o.rest_untouched("AS", _all(c["R"], K + PAD, K))
        outs.append(o)
    Y._check("AS", outs[0].mat[:, :K], c["r64"]["AS"], c["r32"]["AS"])
    assert _zero_bits(outs[0], c["n_tot"], K)                          # stored, not computed: the NaN of S's padding rows stays there
    assert torch.equal(outs[0].bits, outs[1].bits)
    # without a tail the table alone is summed
    if 0 not in c["ids"]:
        o = G.Out(c["R"], K + PAD)
        _nat().call("ell_rowsum_f32", d["ell"], U.ELL_W, None, None, 0, d["gp"], c["B"], c["row_cap"], nmax, d["S"], K, K, o.mat, K + PAD)
        assert torch.equal(o.bits, outs[0].bits)


@pytest.mark.parametrize("name,nmax,K,F", CASES)
def test_forward_products_and_folded_readout(name, nmax, K, F):
    """tsgnn_ragged_tn_direct_ro_f32 on the capacity layout: graph_ptr read on the device, ghost row = row_cap + size"""
    c = _case(name, nmax, K, F)
    d = _device_inputs(c)
    B = c["B"]
    runs = []
    for _ in range(2):
        xo, ao, ro = G.Out(B * K, F), G.Out(B * K, K), G.Out(B, F + PAD)
        arg = torch.full((B * F + G.GUARD,), 12345, dtype=torch.int32, device="cuda")
        _nat().call("ragged_tn_direct_ro_f32", d["S"], K, K, d["gp"], B, d["Z"], F, F, xo.mat, d["AS"], K, K, ao.mat, ro.mat, F + PAD, arg,
                    nmax, c["row_cap"], 1)
        xo.rest_untouched("X'", _all(B * K, F, F)); ao.rest_untouched("A'", _all(B * K, K, K)); ro.rest_untouched("readout", _all(B, F + PAD, F))
        assert bool((arg[B * F:] == 12345).all())
        runs.append((xo, ao, ro, arg))
    xo, ao, ro, arg = runs[0]
    r64, r32 = c["r64"], c["r32"]
    Y._check("X'", xo.mat.view(B, K, F), r64["xo"], r32["xo"])         # (no NaN: the padding rows were not read)
    Y._check("A'", ao.mat.view(B, K, K), r64["ao"], r32["ao"])
    Y._check("readout", ro.mat[:, :F], r64["ro"], r32["ro"])
    assert torch.equal(arg[:B * F].view(B, F).cpu(), r64["arg"])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.bits if isinstance(a, G.Out) else a, b.bits if isinstance(b, G.Out) else b)


@pytest.mark.parametrize("name,nmax,K,F", CASES)
def test_backward(name, nmax, K, F):
    c = _case(name, nmax, K, F)
    d = _device_inputs(c)
    B, R, n_tot = c["B"], c["R"], c["n_tot"]
    dxo, dao = c["dxo"].cuda(), c["dao"].cuda()
    wide = torch.full((B, F + 8), float("nan"), device="cuda")        # the readout's gradient: a column slice of a wider buffer
    wide[:, 4:4 + F] = c["dro"].cuda()
    dro, arg = wide[:, 4:4 + F], c["r64"]["arg"].cuda()

    def run(split, ro=True):
        dZ, dS = G.Out(R, F + PAD), G.Out(R, K + PAD)
        _nat().call("contract_cap_bwd_f32", d["S"], K, d["Z"], F, d["AS"], K, dxo, dao, d["gp"], B, K, F, c["row_cap"], nmax, dZ.mat, F + PAD,
                    dS.mat, K + PAD, dro if ro else None, dro.stride(0) if ro else 0, arg if ro else None, split)
        dZ.rest_untouched("dZ", _all(R, F + PAD, F)); dS.rest_untouched("dS", _all(R, K + PAD, K))
        return dZ, dS
    dZ, dS = run(0)
    r64, r32 = c["r64"], c["r32"]
    Y._check("dZ", dZ.mat[:, :F], r64["dZ"], r32["dZ"])
    Y._check("dS", dS.mat[:, :K], r64["dS"], r32["dS"])
    assert _zero_bits(dZ, n_tot, F) and _zero_bits(dS, n_tot, K)       # padding and ghost rows: stored zeros, whatever S, Z, AS hold there
    for split in (0, 1, 2, 4):                                         # a second run, and every way of dealing the tiles: the same bits
        dZ2, dS2 = run(split)
        assert torch.equal(dZ2.bits, dZ.bits) and torch.equal(dS2.bits, dS.bits), split
    dZ0, dS0 = run(0, ro=False)
    Y._check("dZ without the readout", dZ0.mat[:, :F], r64["dZ0"], r32["dZ0"])
    assert torch.equal(dS0.bits, dS.bits) and not torch.equal(dZ0.bits, dZ.bits)
