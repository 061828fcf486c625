"""The graph-level head kernels (csrc/head.hip) one by one through their C entry points against tests/head_ref.py in float64.

Every output lives in a buffer prefilled with one NaN bit pattern, with a row stride wider than the row where the entry point takes a
stride, and guard words behind it (guard_buf.Out; integer outputs: IntOut).  After a launch
  (1) every float the launch owns is held to the rule of tests/fp32_yardstick.py at K = 8 — the yardstick is head_ref's own float32 run on
      the CPU, never the kernel; for the forward entry points the worse of two such runs that differ in summation order only, see
      _fwd_refs() —, decoded maxima and winners are compared with torch.equal;
  (2) everything else — row padding, rows behind the launch's, guard words, the inputs a launch must not change — is bit for bit what was
      put there.
The backward tests name the kernel they expect (nat.last_kernel()) from the rule documented at head2_bwd_launch, restated in
_bwd_kernel() below, not by asking the library: the second-generation kernel head2_bwd2_kernel<64|128> needs ldo and lddo to be
multiples of 4, 16-byte aligned out / dout, P / 4 <= 512 and its LDS within 159 KB; else head2_bwd_kernel.  <128>: the dU role's chunk —
the caller's with a host map; without one 128 when the launch would exceed the device's compute units (compact: other + ceil(n_real / 64)
+ B + 4 > CUs; dense: (B + 1) ceil(max_nodes / 64) + other > CUs + CUs / 5; other = B + ceil(E / 4) + 1).

Worst  max|hip - ref64| / yardstick  per entry point over this module (bound 8), measured on an MI355X (256 compute units):
    head2_fwd_f32            2.55   (P4 E16 C2 B1, y)              packed_head_fwd_f32      1.60
    head2_fwd_ro_f32         0.94                                  packed_head_fwd_z_f32    2.09
    readout_head_fwd_f32     1.37                                  softmax_ce_f32           1.33   (B37 C6, dlogits)
    head2_bwd_f32            3.11   (gen 1, B300 P64 E20 C3, db2)  head2_bwd_ce_f32         3.75   (gen 1, B300 P64 E20 C3, db1)
    head2_bwd_ro_f32         1.09                                  head2_bwd_du_f32         2.28   (dense, P2048 E32 F4, the clamped row)
    head2_bwd_du_map_f32     3.53   (dense grid sized from the CU count, the clamped row)
With the library-order float32 run alone as the forward yardstick every cell but one was within 2.9; head2_fwd_f32 P128 E1 C6 B1 (vec,
ONE element) stood at 8.6: see _fwd_refs().

Found by this module: a host map that lists FEWER graph == B entries than ceil(max_nodes / du_chunk) leaves padding rows unwritten
(200 padding rows, 64-row chunks: 128 rows with one entry of three, 64 with two) — the zero-fill strides by that count whatever the list
holds.  No caller passes such a list; include/tsgnn.h and head.hip now ask for every chunk 0 .. ceil(max_nodes / du_chunk) - 1, the
case test_head2_bwd_du_capacity_padded pins.
"""
import math

import numpy as np
import pytest
import torch

import head_ref as H
import slot_ref as S
from fp32_yardstick import _check, _yardstick
from guard_buf import GUARD, PAT, Out, _du_ref, _owned

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
IPAT = -7                                # fill of integer outputs
QPAT = 0x5A5A5A5A5A5A5A5A                # fill of 64-bit words a launch must not touch
D, S32 = torch.float64, torch.float32


def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


def _rc(name, *args):
    """the entry point's return code (call() raises on anything but 0)"""
    nat = _nat()
    return getattr(nat.lib(), "tsgnn_" + name)(*[nat._arg(a) for a in args], nat.stream_handle())


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1, 7919, 104729, 1299709, 15485863))) % (1 << 31))


def _strided(t, ld):
    """an INPUT [rows, ld] on the device: t in the first columns, NaN in the padding"""
    b = torch.full((t.size(0), ld), float("nan"), dtype=torch.float32)
    b[:, :t.size(1)] = t
    return b.cuda()


def _c(t):
    return None if t is None else t.cuda()


class IntOut:
    """n int32 on the device, every word IPAT, GUARD words behind"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + GUARD,), IPAT, dtype=torch.int32, device="cuda")

    def get(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert bool((b[self.n:] == IPAT).all()), "%s: guard words overwritten" % what
        return b[:self.n]

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == IPAT).all().item())


def _flat(rows, w):
    """an output without a stride argument: [rows, w] and one more row that is not the launch's"""
    return Out(rows + 1, w)


def _check_flat(what, O, rows, ref64, ref32):
    torch.cuda.synchronize()
    w = O.ld
    _check(what, O.mat[:rows].reshape(ref64.shape), ref64, ref32)
    O.rest_untouched(what, _owned(O.rows, w, 0, rows, 0, w))


def _untouched(*outs):
    torch.cuda.synchronize()
    return all(bool((o.bits == PAT).all().item()) for o in outs if o is not None)


def _weights(P, E, C, gen):
    """W1 / sqrt(P), W2 / sqrt(E): logits of order 1, so that softmax rows are not saturated"""
    r = lambda *s: torch.randn(*s, generator=gen)
    return r(E, P) / math.sqrt(P), r(E), r(C, E) / math.sqrt(E), r(C)


# ============================================================================= (a) head2_fwd_f32, head2_fwd_ro_f32
def _fwd_refs(out, w1, b1, w2, b2):
    """-> (vec64, y64), (vec32, y32).  The float32 run of head_ref is taken in two summation orders (the library's matmul; pairwise), and
    each tensor's yardstick is the run with the larger error: a tensor of ONE element (B = 1, E = 1) is one sample of a rounding error,
    and the first order alone measured 2.5e-8 on a vec = 0.896 - 0.743 whose products sum to 8.0 in magnitude — the pairwise order, on
    the CPU, is already 6.2 times that.  Still the reference's own float32 rounding, never the kernel; K stays 8"""
    r64 = H.head_fwd(out, w1, b1, w2, b2)
    runs = [H.head_fwd(out, w1, b1, w2, b2, dtype=S32, order=o) for o in ("lib", "tree")]
    return r64, tuple(max((r[i] for r in runs), key=lambda t: _yardstick(r64[i], t)) for i in range(2))


def _check_fwd(what, V, Y, B, ref64, ref32):
    _check_flat(what + " vec", V, B, ref64[0], ref32[0])
    _check_flat(what + " y", Y, B, ref64[1], ref32[1])


@pytest.mark.parametrize("E", [1, 5, 16, 128, 130])
@pytest.mark.parametrize("P", [4, 128, 384, 516])
def test_head2_fwd(P, E):
    """P = 4: one float4 lane; 516: more than two passes of 64 lanes; E = 130: a second j0 pass of the 8 x 16 rows; C = 18 > 16 waves"""
    nat = _nat()
    for C in (1, 2, 6, 18):
        for B in (1, 3):
            for bias in (True, False):
                gen = _gen(P, E, C, B, bias)
                out = torch.randn(B, P, generator=gen)
                w1, b1, w2, b2 = _weights(P, E, C, gen)
                if not bias:
                    b1 = b2 = None
                ref64, ref32 = _fwd_refs(out, w1, b1, w2, b2)
                ldo, V, Y = P + 4, _flat(B, E), _flat(B, C)
                nat.call("head2_fwd_f32", _strided(out, ldo), ldo, w1.cuda(), _c(b1), w2.cuda(), _c(b2), B, P, E, C, V.mat, Y.mat)
                assert nat.last_kernel() == "head2_fwd_kernel"
                _check_fwd("head2_fwd_f32 P%d E%d C%d B%d bias%d" % (P, E, C, B, bias), V, Y, B, ref64, ref32)


def _ro_level(B, N, F, gen):
    """z [B * N + 2, F]: ties (the lowest row wins), all-negative columns, graph B - 1 all negative"""
    z = torch.randn(B * N + 2, F, generator=gen)
    z[:, 2] = -z[:, 2].abs() - 0.5
    z[(B - 1) * N:B * N] = -z[(B - 1) * N:B * N].abs() - 0.125
    if N > 1:
        z[0, 0] = z[1, 0] = 9.0
        z[2 * N - 1, 1] = z[2 * N - 2, 1] = 9.0
    return z


@pytest.mark.parametrize("F", [4, 64])
@pytest.mark.parametrize("N", [1, 16, 17, 64])
def test_head2_fwd_ro(N, F):
    """the DiffPool tail: columns [c0, P) of out are the launch's (the level's maxima), [0, c0) its input; N = 16: one batch of rows,
    17: one row into the second, 64: the last full batch"""
    nat, B, c0, E, C = _nat(), 3, 8, 5, 2
    P, ldz = c0 + F, F + 4
    ldo = P + 4
    for bias in (True, False):
        gen = _gen(N, F, bias)
        z, base = _ro_level(B, N, F, gen), torch.randn(B, c0, generator=gen)
        w1, b1, w2, b2 = _weights(P, E, C, gen)
        if not bias:
            b1 = b2 = None
        ro_out, ro_arg = H.ro_tail(z, B, N)
        full = torch.cat([base, ro_out], 1)
        ref64, ref32 = _fwd_refs(full, w1, b1, w2, b2)
        O, A, V, Y = Out(B + 1, ldo), IntOut(B * F), _flat(B, E), _flat(B, C)
        O.mat[:B, :c0] = base.cuda()
        nat.call("head2_fwd_ro_f32", O.mat, ldo, w1.cuda(), _c(b1), w2.cuda(), _c(b2), B, P, E, C, V.mat, Y.mat, _strided(z, ldz), ldz, N,
                 c0, F, A.buf)
        assert nat.last_kernel() == "head2_fwd_kernel(ro)"
        what = "head2_fwd_ro_f32 N%d F%d bias%d" % (N, F, bias)
        _check_fwd(what, V, Y, B, ref64, ref32)
        o = O.mat.cpu()
        assert torch.equal(o[:B, c0:P], ro_out), what + ": maxima"
        assert torch.equal(o[:B, :c0], base), what + ": columns [0, c0) changed"
        O.rest_untouched(what + " out", _owned(O.rows, ldo, 0, B, 0, P))
        arg = A.get(what).view(B, F)
        assert torch.equal(arg, ro_arg), what + ": winners"
        assert bool((ro_out[:, 2] < 0).all()) and bool((ro_out[B - 1] < 0).all())
        if N > 1:
            assert int(arg[0, 0]) == 0 and int(arg[1, 1]) == 2 * N - 2


def test_head2_fwd_ro_unsupported():
    """N = 65: TSGNN_EUNSUPPORTED before any launch"""
    B, c0, F, E, C, N = 3, 8, 4, 5, 2, 65
    P = c0 + F
    gen = _gen(65)
    w1, b1, w2, b2 = _weights(P, E, C, gen)
    O, A, V, Y = Out(B + 1, P + 4), IntOut(B * F), _flat(B, E), _flat(B, C)
    z = torch.randn(B * N, F + 4, generator=gen).cuda()
    assert _rc("head2_fwd_ro_f32", O.mat, P + 4, w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), B, P, E, C, V.mat, Y.mat, z, F + 4, N, c0, F,
               A.buf) == EUNSUPPORTED
    assert _untouched(O, V, Y) and A.untouched()


# ============================================================================= (b) packed_head_fwd_f32, packed_head_fwd_z_f32
def _slot_tests():
    import test_gpu_slot_kernels as T
    return T


def _packed_case(B, Lyr, Fh, Fl):
    """packed words of Lyr layers over a no-ghost layout (B = 7: a graph without nodes -> words of 0), by head_ref.packed_max: ties in
    layer 0, an all-negative layer 1 (a single layer: all negative); one more word zeroed by hand (a column without a candidate)"""
    T = _slot_tests()
    nmax = 5
    Lay = S.Layout(T._readout_sizes(B, nmax, False, "random"), nmax, 0)
    kinds = ["ties", "allneg", "random", "random", "allneg"] if Lyr > 1 else ["allneg"]
    widths = [Fh] * (Lyr - 1) + [Fl]
    words = [H.packed_max(T._readout_input(kinds[l], Lay, w, 31 * l + B + Fh), Lay) for l, w in enumerate(widths)]
    words[0][0, 3] = 0
    packed = H.pack_layers(words)
    out, arg = H.decode_packed(packed, B, Lyr, Fh, Fl)
    assert bool((arg == -1).any()) and bool((out < 0).any())
    if Lyr > 1:
        assert bool((out[:, Fh:2 * Fh] <= 0).all())
    if B == 7:
        assert bool((arg.view(-1)[4 * widths[0]:5 * widths[0]] == -1).all())        # graph 4 has no node
    return packed, out, arg


def _words(t, n):
    """t (int64 [n]) followed by GUARD words of QPAT, on the device"""
    return torch.cat([t, torch.full((GUARD,), QPAT, dtype=torch.int64)]).cuda()


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("Lyr,Fh,Fl", [(1, 8, 8), (3, 36, 20), (3, 128, 128), (5, 128, 12)])
def test_packed_head_fwd(Lyr, Fh, Fl, B):
    """(5, 128, 12): P = 524 > 512, the streamed float4 columns; E = 17: not a multiple of 16; C = 18: the class loop leaves the register
    copy of W2.  The _z variant zeroes what it decoded and clear[0 .. clear_n) (5000 words: more than one pass of B x 1024 threads at
    B = 1) and nothing behind; the plain variant leaves packed as it was"""
    nat = _nat()
    P = (Lyr - 1) * Fh + Fl
    packed, out_ref, arg_ref = _packed_case(B, Lyr, Fh, Fl)
    n, ldo, i = packed.numel(), P + 4, 0
    for E in (1, 17, 128):
        for C in (2, 6, 18):
            for zero in (False, True):
                bias = (i % 2 == 0) != zero
                gen = _gen(P, E, C, B, zero)
                w1, b1, w2, b2 = _weights(P, E, C, gen)
                if not bias:
                    b1 = b2 = None
                ref64, ref32 = _fwd_refs(out_ref, w1, b1, w2, b2)
                pk, O, A, V, Y = _words(packed, n), Out(B + 1, ldo), IntOut(n), _flat(B, E), _flat(B, C)
                tail = [w1.cuda(), _c(b1), w2.cuda(), _c(b2), E, C, V.mat, Y.mat]
                if zero:
                    clear_n = (0, 1, 5000)[i % 3]
                    clear = torch.full((clear_n + GUARD,), QPAT, dtype=torch.int64).cuda()
                    nat.call("packed_head_fwd_z_f32", pk, B, Lyr, Fh, Fl, O.mat, ldo, A.buf, *tail, clear, clear_n)
                    name = "packed_head_fwd_z_f32"
                else:
                    nat.call("packed_head_fwd_f32", pk, B, Lyr, Fh, Fl, O.mat, ldo, A.buf, *tail)
                    name = "packed_head_fwd_f32"
                assert nat.last_kernel() == "packed_head_fwd_kernel<8>"
                what = "%s L%d Fh%d Fl%d B%d E%d C%d bias%d" % (name, Lyr, Fh, Fl, B, E, C, bias)
                _check_fwd(what, V, Y, B, ref64, ref32)
                assert torch.equal(O.mat[:B, :P].cpu(), out_ref), what + ": decoded maxima"
                O.rest_untouched(what + " out", _owned(O.rows, ldo, 0, B, 0, P))
                assert torch.equal(A.get(what), arg_ref), what + ": winners"
                pk = pk.cpu()
                assert bool((pk[n:] == QPAT).all()), what + ": words behind packed"
                if zero:
                    assert bool((pk[:n] == 0).all()), what + ": decoded words not zeroed"
                    clear = clear.cpu()
                    assert bool((clear[:clear_n] == 0).all()) and bool((clear[clear_n:] == QPAT).all()), what + ": clear_n %d" % clear_n
                else:
                    assert torch.equal(pk[:n], packed), what + ": packed changed"
            i += 1


def test_packed_head_fwd_unsupported():
    """E = 129 > 8 rows x 16 waves: both variants refuse before any launch"""
    B, Lyr, Fh, Fl, E, C = 1, 1, 8, 8, 129, 2
    packed, _, _ = _packed_case(B, Lyr, Fh, Fl)
    w1, b1, w2, b2 = _weights(8, E, C, _gen(129))
    for zero in (False, True):
        pk, O, A, V, Y = _words(packed, 8), Out(B + 1, 12), IntOut(8), _flat(B, E), _flat(B, C)
        extra = [_words(torch.zeros(0, dtype=torch.int64), 0), 0] if zero else []
        assert _rc("packed_head_fwd_z_f32" if zero else "packed_head_fwd_f32", pk, B, Lyr, Fh, Fl, O.mat, 12, A.buf, w1.cuda(), b1.cuda(),
                   w2.cuda(), b2.cuda(), E, C, V.mat, Y.mat, *extra) == EUNSUPPORTED
        assert _untouched(O, V, Y) and A.untouched() and torch.equal(pk.cpu()[:8], packed)


# ============================================================================= (c) readout_head_fwd_f32
def _last_layer_input(kind, Lay, F, seed):
    """the last layer has no slot batch-norm: all its ghost rows are equal (the kernel scans the first one only)"""
    x = _slot_tests()._readout_input(kind, Lay, F, seed)
    if Lay.n_ghost:
        x[Lay.n_real:] = x[Lay.n_real].clone()
        if kind == "ghostmax":
            x[Lay.n_real:] = 100.0
        if kind == "ties":
            x[Lay.n_real:, 2] = 60.0                                   # equal to the last real row's of every graph: the real row wins
    return x


RO_KINDS = [("random", True), ("random", False), ("allneg", False), ("ties", True), ("ties", False), ("ghostmax", True)]


@pytest.mark.parametrize("Fl", [4, 20, 128])
@pytest.mark.parametrize("kind,ghosts", RO_KINDS)
@pytest.mark.parametrize("nmax", [5, 64, 130, 260])
def test_readout_head_fwd(nmax, kind, ghosts, Fl):
    """B = 7, L = 3, Fh = 36: layers 0 and 1 decoded from packed, the last layer scanned from its rows (130 / 260 rows: two / three passes
    of 128), then the head.  Without ghost rows graph 4 has no node"""
    nat, T = _nat(), _slot_tests()
    B, Lyr, Fh, E, C = 7, 3, 36, 17, 6
    P, PH = (Lyr - 1) * Fh + Fl, (Lyr - 1) * Fh
    sizes = T._readout_sizes(B, nmax, ghosts, kind)
    Lay = S.Layout(sizes, nmax, nmax if ghosts else 0)
    xs = [T._readout_input(kind, Lay, Fh, 100 * l + nmax + Fl) for l in range(Lyr - 1)]
    xl = _last_layer_input(kind, Lay, Fl, 977 + nmax + Fl)
    words = [H.packed_max(x, Lay) for x in xs]
    # (the last layer's section of packed is not an input of this launch: poison)
    packed = H.pack_layers(words + [np.full((B, Fl), QPAT, dtype=np.uint64)])
    out_ref, arg_ref = H.decode_packed(H.pack_layers(words + [np.zeros((B, Fl), dtype=np.uint64)]), B, Lyr, Fh, Fl)
    for l, x in enumerate(xs):
        o, a = S.readout_max(x, Lay)
        assert torch.equal(out_ref[:, l * Fh:(l + 1) * Fh], o) and torch.equal(arg_ref[l * B * Fh:(l + 1) * B * Fh].view(B, Fh), a)
    o, a = S.readout_max(xl, Lay)
    out_ref[:, PH:], arg_ref[PH * B:] = o, a.reshape(-1)
    if kind == "ghostmax":
        assert bool((a >= Lay.n_real).any())
    if not ghosts:
        assert sizes[4] == 0 and bool((a[4] == -1).all())
    gen = _gen(nmax, Fl, ghosts, len(kind))
    w1, b1, w2, b2 = _weights(P, E, C, gen)
    ref64, ref32 = _fwd_refs(out_ref, w1, b1, w2, b2)
    n, ldo, ldv = packed.numel(), P + 4, Fl + 4
    pk, O, A, V, Y = _words(packed, n), Out(B + 1, ldo), IntOut(n), _flat(B, E), _flat(B, C)
    nat.call("readout_head_fwd_f32", pk, B, Lyr, Fh, Fl, _strided(xl, ldv), ldv, T.c_ptr(Lay.graph_ptr), Lay.n_real, nmax, Lay.n_ghost, O.mat,
             ldo, A.buf, w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), E, C, V.mat, Y.mat)
    assert nat.last_kernel() == "readout_head_fwd_kernel"
    what = "readout_head_fwd_f32 nmax%d %s ghosts%d Fl%d" % (nmax, kind, ghosts, Fl)
    _check_fwd(what, V, Y, B, ref64, ref32)
    assert torch.equal(O.mat[:B, :P].cpu(), out_ref), what + ": maxima"
    O.rest_untouched(what + " out", _owned(O.rows, ldo, 0, B, 0, P))
    assert torch.equal(A.get(what), arg_ref), what + ": winners"
    assert torch.equal(pk.cpu()[:n], packed), what + ": packed changed"


@pytest.mark.parametrize("Fh,Fl", [(36, 132), (35, 6)], ids=["Fl132", "Fl6"])
def test_readout_head_fwd_unsupported(Fh, Fl):
    """Fl > 128 and Fl % 4 != 0 (P % 4 == 0 in both): refused before any launch"""
    T = _slot_tests()
    B, Lyr, nmax, E, C = 2, 3, 5, 5, 2
    P = (Lyr - 1) * Fh + Fl
    assert P % 4 == 0
    Lay = S.Layout([5, 2], nmax, nmax)
    w1, b1, w2, b2 = _weights(P, E, C, _gen(Fl))
    pk, O, A, V, Y = _words(torch.zeros(B * P, dtype=torch.int64), B * P), Out(B + 1, P + 4), IntOut(B * P), _flat(B, E), _flat(B, C)
    ldv = (Fl + 7) // 4 * 4
    assert _rc("readout_head_fwd_f32", pk, B, Lyr, Fh, Fl, torch.zeros(Lay.rows, ldv).cuda(), ldv, T.c_ptr(Lay.graph_ptr), Lay.n_real, nmax,
               nmax, O.mat, P + 4, A.buf, w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), E, C, V.mat, Y.mat) == EUNSUPPORTED
    assert _untouched(O, V, Y) and A.untouched()


# ============================================================================= (d) backward without dU
def _bwd_kernel(B, P, E, C, ldo, lddo, ce, du_F=None, du_chunk=64):
    """the kernel head2_bwd_launch picks, from the rule in the module docstring (pointers here are 16-byte aligned)"""
    if ldo % 4 or lddo % 4 or P // 4 > 512:
        return "head2_bwd_kernel"
    up4 = lambda k: (k + 3) // 4 * 4
    P4 = P // 4
    Gr, Gw = min(16, 1024 // P4), max(1, min(8, 768 // P4))
    role = max(up4(E) + Gr * P, 4 * up4(B) + Gw * 4 * P, 16)
    if du_F is not None:
        role = max(role, up4(E) + (Gr + 1) * du_F)
    lds = 4 * role + (4 * (up4(B * C) + up4(B)) if ce else 0)
    return "head2_bwd2_kernel<%d>" % du_chunk if lds <= 160 * 1024 - 1024 else "head2_bwd_kernel"


class BwdCase:
    """operands of one backward launch (float32 on the CPU) and its references, per (ce, dvec, biases)"""

    def __init__(self, B, P, E, C, seed):
        gen = _gen(B, P, E, C, seed)
        self.B, self.P, self.E, self.C = B, P, E, C
        self.out = torch.randn(B, P, generator=gen)
        self.w1, b1, self.w2, b2 = _weights(P, E, C, gen)
        self.vec, self.y = H.head_fwd(self.out, self.w1, b1, self.w2, b2, dtype=S32)        # what a forward launch left
        self.label = torch.randint(0, C, (B,), generator=gen)
        self.dy = torch.randn(B, C, generator=gen) / B
        self.dvec = torch.randn(B, E, generator=gen) / B
        self._refs = {}

    def ref(self, ce, full):
        """(float64, float32) of (dout, dw1, db1, dw2, db2, normparts, loss | None); full: dvec and both bias gradients present"""
        if (ce, full) not in self._refs:
            r = []
            for dt in (D, S32):
                loss, dy = H.softmax_ce(self.y, self.label, dtype=dt) if ce else (None, self.dy)
                r.append(H.head_bwd(self.out, self.vec, dy, self.dvec if full else None, self.w1, self.w2, has_b1=full, has_b2=full,
                                    dtype=dt) + (loss,))
            self._refs[(ce, full)] = r
        return self._refs[(ce, full)]


class BwdOuts:
    def __init__(self, c, lddo, full, normparts=True):
        B, P, E, C = c.B, c.P, c.E, c.C
        self.c, self.lddo, self.full = c, lddo, full
        self.dout, self.dw1, self.dw2 = Out(B + 1, lddo), _flat(E, P), _flat(C, E)
        self.db1, self.db2 = (_flat(1, E), _flat(1, C)) if full else (None, None)
        self.parts = _flat(1, (E + 3) // 4 + 1) if normparts else None
        self.loss = _flat(1, 1)

    def m(self, o):
        return None if o is None else o.mat

    def grads(self):
        """the entry points' [dout, lddo, dw1, db1, dw2, db2, normparts]"""
        return [self.dout.mat, self.lddo, self.dw1.mat, self.m(self.db1), self.dw2.mat, self.m(self.db2), self.m(self.parts)]

    def check(self, what, ce):
        c = self.c
        r64, r32 = c.ref(ce, self.full)
        torch.cuda.synchronize()
        _check(what + " dout", self.dout.mat[:c.B, :c.P], r64[0], r32[0])
        self.dout.rest_untouched(what + " dout", _owned(c.B + 1, self.lddo, 0, c.B, 0, c.P))
        _check_flat(what + " dw1", self.dw1, c.E, r64[1], r32[1])
        _check_flat(what + " dw2", self.dw2, c.C, r64[3], r32[3])
        if self.full:
            _check_flat(what + " db1", self.db1, 1, r64[2], r32[2])
            _check_flat(what + " db2", self.db2, 1, r64[4], r32[4])
        if self.parts is not None:
            _check_flat(what + " normparts", self.parts, 1, r64[5], r32[5])
        if ce:
            _check_flat(what + " loss", self.loss, 1, r64[6].reshape(1), r32[6].reshape(1))
        else:
            assert _untouched(self.loss), what + ": loss written without the folded loss"

    def untouched(self):
        return _untouched(self.dout, self.dw1, self.dw2, self.db1, self.db2, self.parts, self.loss)


def _bwd_inputs(c, ldo, full):
    return _strided(c.out, ldo), c.vec.cuda(), (c.dvec.cuda() if full else None), c.w1.cuda(), c.w2.cuda()


def _ce_loss_bits(c):
    """the loss tsgnn_softmax_ce_f32 returns for the same logits, as bits"""
    loss, dl = torch.zeros(1, device="cuda"), torch.empty(c.B, c.C, device="cuda")
    _nat().call("softmax_ce_f32", c.y.cuda(), c.C, c.label.cuda(), c.B, c.C, loss, dl)
    return loss.cpu().view(torch.int32)


BWD_SHAPES = [(1, 4, 1, 1), (3, 128, 5, 2), (32, 384, 128, 2), (37, 320, 130, 6), (9, 2048, 40, 5), (300, 64, 20, 3)]


@pytest.mark.parametrize("gen", [2, 1], ids=["gen2", "gen1"])
@pytest.mark.parametrize("B,P,E,C", BWD_SHAPES)
def test_head2_bwd(B, P, E, C, gen):
    """head2_bwd_f32 and head2_bwd_ce_f32 on both kernel generations (the first through ldo = lddo = P + 2), the same operands.
    (37, 320, 130, 6): 12 row groups of 80 lanes leave 64 lanes idle, the last weight block is partial, C > 4 leaves the pick4 select;
    (9, 2048, 40, 5): 2 row groups -> two batches of W1 rows, one graph group -> three batches of graphs; (300, 64, 20, 3): 4B > 1024
    (i != tid) and B > 256 (the loss reduction's stride loop).  With / without dvec, bias gradients and normparts"""
    nat = _nat()
    c = BwdCase(B, P, E, C, 1)
    ld = P + 4 if gen == 2 else P + 2
    expect = _bwd_kernel(B, P, E, C, ld, ld, False)
    assert expect == ("head2_bwd2_kernel<64>" if gen == 2 else "head2_bwd_kernel")
    for ce in (False, True):
        for full in (True, False):
            out, vec, dvec, w1, w2 = _bwd_inputs(c, ld, full)
            o = BwdOuts(c, ld, full, normparts=full)
            if ce:
                nat.call("head2_bwd_ce_f32", out, ld, vec, c.y.cuda(), c.label.cuda(), o.loss.mat, dvec, w1, w2, B, P, E, C, *o.grads())
            else:
                nat.call("head2_bwd_f32", out, ld, vec, c.dy.cuda(), dvec, w1, w2, B, P, E, C, *o.grads())
            assert nat.last_kernel() == _bwd_kernel(B, P, E, C, ld, ld, ce) == expect
            o.check("head2_bwd%s_f32 gen%d B%d P%d E%d C%d full%d" % ("_ce" if ce else "", gen, B, P, E, C, full), ce)
            if ce and gen == 2:
                # head.hip: "summed exactly as tsgnn_softmax_ce_f32 sums it ... agree to the bit"
                assert torch.equal(o.loss.mat[0].cpu().view(torch.int32), _ce_loss_bits(c)), "folded loss != tsgnn_softmax_ce_f32's bits"


def test_head2_bwd_unsupported():
    """B = 1025: refused before any launch"""
    B, P, E, C = 1025, 4, 1, 1
    c = BwdCase(B, P, E, C, 2)
    out, vec, dvec, w1, w2 = _bwd_inputs(c, P + 4, True)
    o = BwdOuts(c, P + 4, True)
    assert _rc("head2_bwd_f32", out, P + 4, vec, c.dy.cuda(), dvec, w1, w2, B, P, E, C, *o.grads()) == EUNSUPPORTED
    assert _rc("head2_bwd_ce_f32", out, P + 4, vec, c.y.cuda(), c.label.cuda(), o.loss.mat, dvec, w1, w2, B, P, E, C, *o.grads()) == EUNSUPPORTED
    assert o.untouched()


@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("B", [1, 37, 300])
def test_softmax_ce(B, C):
    """tsgnn_softmax_ce_f32 itself, logits with ld > C; row 0 holds +80 / -80 (without the max subtraction expf overflows)"""
    nat, ld = _nat(), C + 3
    gen = _gen(B, C)
    y = torch.randn(B, C, generator=gen)
    y[0, 0], y[0, C - 1] = -80.0, 80.0
    label = torch.randint(0, C, (B,), generator=gen)
    label[0] = 0
    (l64, d64), (l32, d32) = H.softmax_ce(y, label), H.softmax_ce(y, label, dtype=S32)
    Lo, Dl = _flat(1, 1), _flat(B, C)
    nat.call("softmax_ce_f32", _strided(y, ld), ld, label.cuda(), B, C, Lo.mat, Dl.mat)
    what = "softmax_ce_f32 B%d C%d" % (B, C)
    _check_flat(what + " loss", Lo, 1, l64.reshape(1), l32.reshape(1))
    _check_flat(what + " dlogits", Dl, B, d64, d32)


@pytest.mark.parametrize("F", [4, 64])
@pytest.mark.parametrize("N", [1, 17, 64])
def test_head2_bwd_ro(N, F):
    """the DiffPool tail's backward: dz[b * N + n, f] = dout[b, c0 + f] at the winner, exactly 0 elsewhere (arg -1: the whole column),
    every element of every row written; dy given and the loss folded in; dy AND the loss, or neither: EINVAL; the first generation's
    strides: EUNSUPPORTED"""
    nat, B, c0, E, C = _nat(), 3, 8, 5, 2
    P, lddz = c0 + F, F + 4
    ld = P + 4
    c = BwdCase(B, P, E, C, 3 + N)
    gen = _gen(N, F)
    arg = (torch.arange(B)[:, None] * N + torch.randint(0, N, (B, F), generator=gen)).to(torch.int32)
    arg[1, 0] = arg[2, F - 1] = -1
    argd = arg.cuda()
    structural0 = arg.long().repeat_interleave(N, dim=0) != torch.arange(B * N)[:, None]
    out, vec, dvec, w1, w2 = _bwd_inputs(c, ld, True)
    for ce in (False, True):
        o, DZ = BwdOuts(c, ld, True), Out(B * N + 1, lddz)
        cea = [c.y.cuda(), c.label.cuda(), o.loss.mat] if ce else [None, None, None]
        nat.call("head2_bwd_ro_f32", out, ld, vec, None if ce else c.dy.cuda(), dvec, w1, w2, B, P, E, C, *o.grads(), argd, c0, F, N, DZ.mat,
                 lddz, *cea)
        assert nat.last_kernel() == _bwd_kernel(B, P, E, C, ld, ld, ce) == "head2_bwd2_kernel<64>"
        what = "head2_bwd_ro_f32 N%d F%d ce%d" % (N, F, ce)
        o.check(what, ce)
        r64, r32 = c.ref(ce, True)
        _check(what + " dz", DZ.mat[:B * N, :F], H.ro_tail_bwd(r64[0][:, c0:], arg, B, N), H.ro_tail_bwd(r32[0][:, c0:], arg, B, N))
        DZ.rest_untouched(what + " dz", _owned(DZ.rows, lddz, 0, B * N, 0, F))
        assert bool((DZ.mat[:B * N, :F].cpu()[structural0] == 0).all()), what + ": a row that did not win is not exactly 0"
    o, DZ = BwdOuts(c, ld, True), Out(B * N + 1, lddz)
    ce3 = [c.y.cuda(), c.label.cuda(), o.loss.mat]
    head = [out, ld, vec]
    mid = [dvec, w1, w2, B, P, E, C, *o.grads(), argd, c0, F, N, DZ.mat, lddz]
    assert _rc("head2_bwd_ro_f32", *head, c.dy.cuda(), *mid, *ce3) == EINVAL
    assert _rc("head2_bwd_ro_f32", *head, None, *mid, None, None, None) == EINVAL
    o1 = BwdOuts(c, P + 2, True)
    mid1 = [dvec, w1, w2, B, P, E, C, *o1.grads(), argd, c0, F, N, DZ.mat, lddz]
    assert _rc("head2_bwd_ro_f32", _strided(c.out, P + 2), P + 2, vec, c.dy.cuda(), *mid1, None, None, None) == EUNSUPPORTED
    assert o.untouched() and o1.untouched() and _untouched(DZ)


# ============================================================================= (e) the dU role
DU_SIZES = [30, 1, 100, 0, 64, 65, 129]          # a one-node graph, an empty one, an exact chunk, one row into the next, three 64-row chunks


class DuOperands:
    """the last layer's rows as the dU role reads them: v normalised (row 1: a clamped norm), rinv, winners arg [B, F] — real rows of the
    graph, ghost winners (row n_real + size_b, where that ghost row exists), -1, two equal-size graphs on one ghost row where the sizes
    have such a pair — and the row bookkeeping of a batch with `pad` rows of no graph behind the real ones"""

    def __init__(self, sizes, n_ghost, pad, F, seed):
        B = len(sizes)
        gp = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(sizes, out=gp[1:])
        self.sizes, self.B, self.F, self.n_ghost, self.gp = list(sizes), B, F, n_ghost, torch.from_numpy(gp)
        self.n_data, self.n_real = int(gp[B]), int(gp[B]) + pad
        gen = _gen(seed, F, n_ghost, pad, B)
        u = torch.randn(self.n_real + n_ghost, F, dtype=D, generator=gen)
        self.clamped = 1 if sizes[0] >= 2 else None
        if self.clamped is not None:
            u[1] = u[1].abs() * (0.5e-12 / u[1].norm())
        nrm = u.norm(dim=1, keepdim=True).clamp(min=1e-12)
        self.v, self.rinv = (u / nrm).float(), (1.0 / nrm[:, 0]).float()
        if self.clamped is not None:
            assert float(self.rinv[1]) >= S.CLAMPED
        sz = torch.as_tensor(np.asarray(sizes, dtype=np.int64))
        arg = self.gp[:-1, None] + (torch.rand(B, F, generator=gen) * sz[:, None]).long()
        pick = torch.rand(B, F, generator=gen)
        arg = torch.where((pick < 0.3) & (sz < n_ghost)[:, None], (self.n_real + sz)[:, None].expand(B, F), arg)
        arg = torch.where(pick > 0.9, torch.full_like(arg, -1), arg)
        arg = torch.where((sz == 0)[:, None] & (arg < self.n_real), torch.full_like(arg, -1), arg)        # an empty graph has no real row
        if self.clamped is not None:
            arg[0, 1] = 1
        seen = {}
        for b, s in enumerate(sizes):                                  # the first two graphs of equal size both win that ghost row
            if s in seen and s < n_ghost:
                arg[seen[s], 0] = arg[b, 0] = self.n_real + s
                break
            seen.setdefault(s, b)
        self.arg = arg.to(torch.int32)
        real = (self.arg >= 0) & (self.arg < self.n_real)
        assert bool((self.arg[real] >= self.gp[:-1, None].expand(B, F)[real]).all()) and bool((self.arg[real] < self.gp[1:, None].expand(B, F)[real]).all())

    def ref(self, dout64, dout32, off):
        a = (self.v, self.rinv, self.arg)
        b = (off, self.gp, self.n_real, self.n_ghost)
        return _du_ref(*a, dout64, *b, D), _du_ref(*a, dout32, *b, S32)

    def du_map(self, chunk, pad_blocks):
        ent = [(b << 8) | k for b, s in enumerate(self.sizes) for k in range(max(1, -(-s // chunk)))]
        ent += [(self.B << 8) | k for k in range(pad_blocks)]
        return torch.tensor(ent, dtype=torch.int32).cuda(), len(ent)


def _ncu():
    return torch.cuda.get_device_properties(torch.device("cuda")).multi_processor_count


def _du_chunk_rule(form, B, E, n_real, max_nodes):
    """the chunk the entry point picks itself (dense and compact forms), from the device's compute-unit count"""
    ncu, other = _ncu(), B + (E + 3) // 4 + 1
    if form == "compact" and B <= 64:
        return 128 if other + (n_real + 63) // 64 + B + 4 > ncu else 64
    return 128 if (B + 1) * ((max_nodes + 63) // 64) + other > ncu + ncu // 5 else 64


def _run_du(c, d, off, form, ce, what, expect=None):
    """one launch with the dU role on BwdCase c / DuOperands d -> the guarded dU buffer, after every output was checked.
    form: map64 | map128 (tsgnn_head2_bwd_du_map_f32 with a host list), dense (tsgnn_head2_bwd_du_f32), compact (n_map = -1)"""
    nat = _nat()
    B, P, E, C, F = c.B, c.P, c.E, c.C, d.F
    ld, ldv, lddu = P + 4, F + 4, F + 8
    max_nodes = max(d.sizes)
    out, vec, dvec, w1, w2 = _bwd_inputs(c, ld, True)
    o, DU = BwdOuts(c, ld, True), Out(d.n_real + B + 3, lddu)
    head = [out, ld, vec] + ([c.y.cuda(), c.label.cuda(), o.loss.mat, None] if ce else [None, None, None, c.dy.cuda()])
    rows = [T32(d.gp), d.n_real, d.n_ghost, max_nodes, _strided(d.v, ldv), ldv, d.rinv.cuda(), d.arg.cuda(), off, F, DU.mat, lddu]
    args = head + [dvec, w1, w2, B, P, E, C] + o.grads() + rows
    if form.startswith("map"):
        chunk = int(form[3:])
        m, n = d.du_map(chunk, -(-max_nodes // chunk) if d.n_real > d.n_data else 0)
        nat.call("head2_bwd_du_map_f32", *args, m, n, chunk)
    else:
        chunk = _du_chunk_rule(form, B, E, d.n_real, max_nodes)
        if form == "dense":
            nat.call("head2_bwd_du_f32", *args)
        else:
            nat.call("head2_bwd_du_map_f32", *args, None, -1, 64)
    name = _bwd_kernel(B, P, E, C, ld, ld, ce, du_F=F, du_chunk=chunk)
    assert nat.last_kernel() == name, (what, nat.last_kernel(), name)
    if expect is not None:
        assert name == expect, (what, name)
    o.check(what, ce)
    r64, r32 = c.ref(ce, True)
    du64, du32 = d.ref(r64[0], r32[0], off)
    torch.cuda.synchronize()
    nr = d.n_real + B
    keep = torch.ones(nr, dtype=torch.bool)
    if d.clamped is not None:                                           # (a clamped row's gradient is 1e12 times the others': its own scale)
        keep[d.clamped] = False
        _check(what + " du (clamped row)", DU.mat[:nr, :F].cpu()[~keep], du64[~keep], du32[~keep])
    _check(what + " du", DU.mat[:nr, :F].cpu()[keep], du64[keep], du32[keep])
    assert bool((DU.mat[d.n_data:d.n_real, :F].cpu() == 0).all()), what + ": a padding row is not exactly 0"
    DU.rest_untouched(what + " du", _owned(DU.rows, lddu, 0, nr, 0, F))
    return DU


def T32(t):
    return t.to(torch.int32).cuda()


DU_FORMS = ["map64", "map128", "dense", "compact"]


@pytest.mark.parametrize("F", [4, 64, 128])
@pytest.mark.parametrize("P,E", [(384, 128), (128, 5), (2048, 32)])
@pytest.mark.parametrize("form", DU_FORMS)
def test_head2_bwd_du(form, P, E, F):
    """the dU rows of the last layer from the head's backward launch, operands built directly: every block-resolution form, the segment
    at the front and at the end of dout's row, dy given and the loss folded in, ghost rows for every graph (130), none for the largest
    graph (129 = its size) and none at all; dout, the weight gradients and normparts as without the role"""
    B, C = len(DU_SIZES), 3
    c = BwdCase(B, P, E, C, 5)
    for off in sorted({0, P - F}):
        for ce in (False, True):
            for n_ghost in (130, 129, 0):
                d = DuOperands(DU_SIZES, n_ghost, 0, F, off + ce)
                if n_ghost:
                    assert bool((d.arg >= d.n_real).any()) and bool((d.arg == -1).any())
                _run_du(c, d, off, form, ce, "head2_bwd_du%s_f32 %s P%d E%d F%d off%d ce%d ghost%d" % (
                    "" if form == "dense" else "_map", form, P, E, F, off, ce, n_ghost),
                    expect="head2_bwd2_kernel<%s>" % form[3:] if form.startswith("map") else None)


@pytest.mark.parametrize("form", DU_FORMS)
def test_head2_bwd_du_unsupported(form):
    """(P, E) = (2048, 64): more W1 rows than one batch of the role's two row groups: refused, nothing written"""
    B, P, E, C, F = len(DU_SIZES), 2048, 64, 3, 64
    c, d = BwdCase(B, P, E, C, 6), DuOperands(DU_SIZES, 130, 0, F, 1)
    ld = P + 4
    out, vec, dvec, w1, w2 = _bwd_inputs(c, ld, True)
    o, DU = BwdOuts(c, ld, True), Out(d.n_real + B + 3, F + 8)
    args = [out, ld, vec, None, None, None, c.dy.cuda(), dvec, w1, w2, B, P, E, C] + o.grads() + [
        T32(d.gp), d.n_real, d.n_ghost, max(d.sizes), _strided(d.v, F + 4), F + 4, d.rinv.cuda(), d.arg.cuda(), 0, F, DU.mat, F + 8]
    if form.startswith("map"):
        m, n = d.du_map(int(form[3:]), 0)
        rc = _rc("head2_bwd_du_map_f32", *args, m, n, int(form[3:]))
    elif form == "dense":
        rc = _rc("head2_bwd_du_f32", *args)
    else:
        rc = _rc("head2_bwd_du_map_f32", *args, None, -1, 64)
    assert rc == EUNSUPPORTED and o.untouched() and _untouched(DU)


def _many_sizes(B):
    return [(3, 1, 0, 7, 3, 70, 12, 64)[i % 8] for i in range(B)]


@pytest.mark.parametrize("B", [64, 65])
def test_head2_bwd_du_compact_B(B):
    """n_map = -1 at B = 64 — every lane of the resolving wave owns a graph — and at B = 65, where the entry point falls to the dense grid;
    graphs 0 and 4 (3 nodes each) both win ghost row n_real + 3"""
    P, E, C, F = 128, 5, 2, 64
    sizes = _many_sizes(B)
    c, d = BwdCase(B, P, E, C, 7), DuOperands(sizes, 71, 0, F, 2)
    assert int(d.arg[0, 0]) == int(d.arg[4, 0]) == d.n_real + 3
    _run_du(c, d, P - F, "compact", True, "head2_bwd_du_map_f32 compact B%d" % B)


@pytest.mark.parametrize("form", ["dense", "compact"])
def test_head2_bwd_du_chunk_from_cu_count(form):
    """batches sized from the device's compute-unit count so that the entry point itself takes 128-row chunks (the only cases of this
    module above a few hundred rows)"""
    ncu = _ncu()
    if form == "dense":
        B, P, E, C, F = 32, 384, 128, 2, 64
        other = B + (E + 3) // 4 + 1
        big = 64 * ((max(ncu + ncu // 5 - other, 0)) // (B + 1) + 1) - 12     # the smallest chunk count over the limit, not a multiple of 128
        sizes = [big] + [3 + (5 * i) % 37 for i in range(B - 1)]
    else:
        B, P, E, C, F = 3, 128, 5, 2, 4
        other = B + (E + 3) // 4 + 1
        n = 64 * max(ncu - other - B - 4, 1) + 40
        sizes = [n // 3, n - n // 3 - 600, 600]
    c, d = BwdCase(B, P, E, C, 8), DuOperands(sizes, max(sizes) + 1, 0, F, 3)
    assert _du_chunk_rule(form, B, E, d.n_real, max(sizes)) == 128
    _run_du(c, d, P - F, form, False, "head2_bwd_du_map_f32 %s chunk from %d CUs" % (form, ncu), expect="head2_bwd2_kernel<128>")


@pytest.mark.parametrize("pad", [1, 31, 32, 33, 200])
@pytest.mark.parametrize("form", ["map64", "map128", "dense", "compact"])
def test_head2_bwd_du_capacity_padded(form, pad):
    """graph_ptr[B] < n_real: every padding row is exactly 0 over [0, F), rows at and beyond n_real + B are untouched.  Host map: the
    padding rows are listed as graph == B, chunks 0 .. ceil(max_nodes / du_chunk) - 1 — the count the zero-fill strides by"""
    B, P, E, C, F = len(DU_SIZES), 128, 5, 2, 64
    c, d = BwdCase(B, P, E, C, 9), DuOperands(DU_SIZES, 130, pad, F, 4)
    _run_du(c, d, P - F, form, False, "head2_bwd_du_map_f32 %s pad%d" % (form, pad))


def test_head2_bwd_du_capacity_padded_compact_stride():
    """the compact form has ceil(n_real / 64) + B + 4 workgroups less the batch's pairs for the padding rows; 1,000 of them are more than
    32 per such workgroup: the zero-fill takes its stride"""
    B, P, E, C, F, pad = len(DU_SIZES), 128, 5, 2, 64, 1000
    c, d = BwdCase(B, P, E, C, 9), DuOperands(DU_SIZES, 130, pad, F, 4)
    assert _du_chunk_rule("compact", B, E, d.n_real, max(DU_SIZES)) == 64
    pad_blocks = (d.n_real + 63) // 64 + B + 4 - sum(max(1, -(-s // 64)) for s in DU_SIZES)
    assert pad > 32 * pad_blocks
    _run_du(c, d, P - F, "compact", False, "head2_bwd_du_map_f32 compact pad%d" % pad)


def test_graphbatch_du_map():
    """GraphBatch.du_map: every non-empty (graph, chunk) once, chunk 0 of every graph, nothing else; 64-row chunks while other_blocks +
    the 64-row chunk count stays within the compute units, else 128"""
    from two_stage_gnn_amd.graph import GraphBatch
    g = GraphBatch.structure_only(DU_SIZES, max(DU_SIZES), "cuda", ghosts=False)
    ncu = _ncu()
    n64 = sum(max(1, -(-s // 64)) for s in DU_SIZES)
    seen = set()
    for other in (1, ncu - n64, ncu - n64 + 1, ncu + 5):
        if other < 1:
            continue
        m, n, chunk = g.du_map(other)
        assert chunk == (64 if other + n64 <= ncu else 128)
        seen.add(chunk)
        ent = m.cpu().tolist()
        want = [(b << 8) | k for b, s in enumerate(DU_SIZES) for k in range(max(1, -(-s // chunk)))]
        assert n == len(ent) == len(set(ent)) and sorted(ent) == sorted(want)
        assert all((b << 8) in ent for b in range(len(DU_SIZES)))
    assert seen == {64, 128}
