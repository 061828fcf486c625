"""Host-side plumbing that needs no GPU: the column buffer that replaces torch.cat of the levels' readouts, the deferred-loss
context, the C-ABI's workspace-size helpers (encoders.py:203,388-391; train.py:121-129)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_readout_columns_alias_the_buffer_and_route_gradients():
    """ReadoutColumns: every part is written in place into its column block, join() IS the concatenation (no copy), and the
    gradient of a part is the matching column slice of the buffer's gradient (read in place: same storage)"""
    from two_stage_gnn_amd import message_passing as mp

    class Write(torch.autograd.Function):                  # stands for a readout launch that writes its block in place
        @staticmethod
        def forward(ctx, x, into):
            into.t.copy_(x * 2.0)
            return into.t

        @staticmethod
        def backward(ctx, d):
            Write.seen.append((d.data_ptr(), tuple(d.shape), d.stride()))
            return d * 2.0, None
    Write.seen = []
    cols = mp.ReadoutColumns(3, 12, torch.device("cpu"))
    xs = [torch.randn(3, 4, requires_grad=True) for _ in range(3)]
    parts = [Write.apply(x, cols.take(4)) for x in xs]
    assert all(not p._is_view() for p in parts)            # aliases of the storage, not autograd views of the buffer
    out = cols.join(parts)
    assert out.data_ptr() == cols.buf.data_ptr() and out.shape == (3, 12)
    torch.testing.assert_close(out.detach(), torch.cat([x.detach() * 2.0 for x in xs], dim=1))
    w = torch.arange(36.0).reshape(3, 12)
    (out * w).sum().backward()
    for k, x in enumerate(xs):
        torch.testing.assert_close(x.grad, 2.0 * w[:, 4 * k:4 * k + 4])
    assert sorted(s[2] for s in Write.seen) == [(12, 1)] * 3            # column slices of ONE [3, 12] gradient, not copies
    # blocks that do not fit, or are not 16-byte aligned: take() says so and join() concatenates
    cols2 = mp.ReadoutColumns(2, 8, torch.device("cpu"))
    a = cols2.take(4)
    assert a is not None and cols2.take(8) is None and cols2.take(4) is None
    p0, p1 = torch.ones(2, 4), torch.zeros(2, 4)
    assert torch.equal(cols2.join([p0, p1]), torch.cat([p0, p1], dim=1))
    assert mp.ReadoutColumns(2, 6, torch.device("cpu")).take(3) is None


def test_deferred_loss_context_restores_the_flag():
    from two_stage_gnn_amd import message_passing as mp
    assert mp.CE_DEFER is False
    with mp.deferred_loss():
        assert mp.CE_DEFER is True
        with mp.deferred_loss():
            assert mp.CE_DEFER is True
        assert mp.CE_DEFER is True
    assert mp.CE_DEFER is False
    with pytest.raises(RuntimeError):
        with mp.deferred_loss():
            raise RuntimeError("x")
    assert mp.CE_DEFER is False
    # off the GPU the library's losses are torch's (nothing is deferred, nothing is launched)
    logits, label = torch.randn(5, 3, requires_grad=True), torch.tensor([0, 2, 1, 1, 0])
    with mp.deferred_loss():
        torch.testing.assert_close(mp.cross_entropy(logits, label), torch.nn.functional.cross_entropy(logits, label))
        logp = torch.log_softmax(logits, -1)
        torch.testing.assert_close(mp.nll_loss(logp, label), torch.nn.functional.nll_loss(logp, label))


def test_workspace_size_helpers():
    """host-only entry points of the C ABI: sizes the callers allocate from (include/tsgnn.h)"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    assert L.tsgnn_readout_max_ws_words(16, 64, 192) == 1                      # <= 64 slots: one launch, no workspace
    assert L.tsgnn_readout_max_ws_words(16, 512, 192) == 16 * 192 + 8          # packed maxima + the graphs' ticket counters
    assert L.tsgnn_readout_max_ws_words(0, 512, 192) == 0 and L.tsgnn_readout_max_ws_words(1 << 20, 4096, 4096) == -1
    assert L.tsgnn_ragged_tn_direct_supported(64, 512) == 1 and L.tsgnn_ragged_tn_direct_supported(129, 512) == 0
    assert L.tsgnn_ragged_tn_direct_supported(64, 5000) == 0


def test_wgrad_sets_closing_reduction_bookkeeping(monkeypatch):
    """mp.WgradSets, the closing weight-gradient reduction of the fused backward nodes: every slice is taken from the sink once,
    sunk gradients go back to autograd as None, the shares are asked for only when every gradient went to the sink and the record
    count allows it, and the parameters are marked normed only when the launcher reports that the shares were left"""
    from two_stage_gnn_amd import message_passing as mp

    class Sink:
        def __init__(self, params):
            self.views = {id(p): torch.zeros(p.shape) for p in params}
            self.taken = []
            self.normed = set()

        def take(self, param, shape):
            self.taken.append(id(param))
            v = self.views.get(id(param))
            return v if v is not None and tuple(v.shape) == tuple(shape) else None

    def launcher(flag):
        def launch(sets, norm_sink=None):
            launch.calls.append((list(sets), norm_sink))
            return flag and norm_sink is not None
        launch.calls = []
        return launch

    w, b, w2 = torch.ones(3, 2), torch.ones(3), torch.ones(2, 2)

    def run(sink, flag, params, nsets=2, **kw):
        monkeypatch.setattr(mp, "GRAD_SINK", sink)
        launch = launcher(flag)
        red = mp.WgradSets(launch, **kw)
        bufs = [red.grad(p, tuple(p.shape) if p is not None else (3,)) for p in params]
        for k in range(nsets):
            red.add(("set", k))
        out = [red.autograd_grad(t) for t in bufs]
        red.close()
        return bufs, out, launch.calls

    # every gradient from the sink: each slice taken once, None to autograd, shares asked for and the parameters marked normed
    sink = Sink([w, b, w2])
    bufs, out, calls = run(sink, True, [w, b, None, w2])
    assert sorted(sink.taken) == sorted([id(w), id(b), id(w2)])
    assert [t is sink.views[id(p)] for t, p in zip(bufs, (w, b))] == [True, True] and bufs[2] is None
    assert out == [None, None, None, None]
    assert calls == [([("set", 0), ("set", 1)], sink)]
    assert sink.normed == {w.data_ptr(), b.data_ptr(), w2.data_ptr()}
    # the launcher did not leave the shares: nothing is marked normed
    sink = Sink([w, b])
    _, _, calls = run(sink, False, [w, b])
    assert calls[0][1] is sink and sink.normed == set()
    # one gradient the sink does not hold: a new buffer, returned to autograd; no shares
    sink = Sink([w])
    bufs, out, calls = run(sink, True, [w, b])
    assert out[0] is None and out[1] is bufs[1] and bufs[1].shape == (3,) and bufs[1] is not sink.views[id(w)]
    assert calls[0][1] is None and sink.normed == set()
    # more records than the shares allow for: no shares, the same single launch
    sink = Sink([w, b])
    _, out, calls = run(sink, True, [w, b], nsets=5, max_sets_with_shares=4)
    assert out == [None, None] and len(calls) == 1 and len(calls[0][0]) == 5 and calls[0][1] is None and sink.normed == set()
    _, _, calls = run(Sink([w, b]), True, [w, b], nsets=4, max_sets_with_shares=4)
    assert calls[0][1] is not None
    # buffers the caller allocated itself (no grad()): the sink is left alone
    sink = Sink([w])
    _, _, calls = run(sink, True, [])
    assert calls[0][1] is None and sink.taken == [] and sink.normed == set()
    # no sink installed: new buffers, all returned to autograd; nothing recorded -> no launch
    bufs, out, calls = run(None, True, [w, b])
    assert out[0] is bufs[0] and out[1] is bufs[1] and calls[0][1] is None
    assert run(Sink([w]), True, [w], nsets=0)[2] == []
