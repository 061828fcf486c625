"""Host side of the per-graph pooled-level layers (csrc/dense_stack_pg.hip, dense_stack_pg.py): declarations and exports, the envelope,
argument checks that run before anything is launched, and the routing predicate.  No GPU."""
import ctypes

import torch

ENTRY_POINTS = ("tsgnn_dense_pg_supported", "tsgnn_dense_pg_layer_fwd_f32", "tsgnn_dense_pg_layer_bwd_f32", "tsgnn_dense_pg_dx_f32")


def test_header_declares_and_library_exports_the_entry_points():
    from two_stage_gnn_amd import _native as nat
    decls = nat.parse_header()
    nat.build()
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in decls, name
        assert hasattr(L, name), name
    assert [p[1] for p in decls["tsgnn_dense_pg_supported"][1]] == ["B", "K", "fin", "n"]


def test_envelope_truth_table():
    from two_stage_gnn_amd import _native as nat
    ok = nat.lib().tsgnn_dense_pg_supported
    assert ok(3, 100, 192, 64) == 1 and ok(1, 4, 4, 4) == 1
    assert ok(3, 100, 384, 128) == 1 and ok(32, 128, 384, 128) == 1               # the widest shape, hidden 128 at the two-stage defaults
    assert ok(3, 6, 192, 64) == 0 and ok(3, 132, 192, 64) == 0                     # K = 6, K = 132
    assert ok(3, 100, 6, 64) == 0 and ok(3, 100, 192, 132) == 0                    # fin = 6, n = 132
    assert ok(3, 100, 388, 64) == 0 and ok(3, 100, 192, 6) == 0 and ok(0, 100, 192, 64) == 0 and ok(3, 0, 192, 64) == 0


def test_null_pointers_are_invalid_before_any_launch():
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    assert L.tsgnn_dense_pg_layer_fwd_f32(None, 192, None, None, 64, None, 3, 100, 192, 64, 1, None, None, None, None, None, None, 64, None) == -1
    assert L.tsgnn_dense_pg_layer_bwd_f32(None, None, 64, None, None, 64, None, None, None, None, 192, None, 64, None, 3, 100, 192, 64, 1,
                                          None, None, None, 0, None) == -1
    assert L.tsgnn_dense_pg_dx_f32(None, None, 3, 100, 192, None, 192, None) == -1
    # a leading dimension shorter than the row is invalid as well, whatever the pointers
    one = ctypes.c_void_p(16)
    assert L.tsgnn_dense_pg_dx_f32(one, one, 3, 100, 192, one, 100, None) == -1
    # ... and a shape outside the envelope is "unsupported", decided on the host
    assert L.tsgnn_dense_pg_dx_f32(one, one, 3, 6, 192, one, 192, None) == -3
    assert L.tsgnn_dense_pg_layer_fwd_f32(one, 192, one, one, 132, None, 3, 100, 192, 132, 1, None, None, None, None, None, one, 132, None) == -3


def test_eligible_refuses_what_the_kernels_do_not_compute():
    from two_stage_gnn_amd import dense_encoders as E, dense_stack_pg as PG
    mk = lambda **kw: [E.GraphConv(8, 8, normalize_embedding=True, **kw).cpu() for _ in range(2)]
    x, adj = torch.zeros(3, 8, 8), torch.zeros(3, 8, 8)
    assert PG.convs_ok(mk()) and not PG.eligible(x, adj, mk())                     # CPU tensors: no device, no route
    assert not PG.convs_ok(mk(add_self=True)) and not PG.convs_ok(mk(dropout=0.5))
    assert not PG.eligible(x, adj, mk(add_self=True))
    assert not PG.eligible(x, adj, mk(dropout=0.5))
    assert hasattr(E, "PER_GRAPH_DENSE") and E.PER_GRAPH_DENSE is True
