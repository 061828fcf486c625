"""tsgnn_gather_rowgemm_st_mode_f32 (include/tsgnn.h: layer 0's launch with the path of its B operand named) refuses on the host,
before anything is launched: a b_mode outside 0..2, the direct mode where it does not apply, and what tsgnn_gather_rowgemm_st_f32
already refuses.  No GPU needed."""
EINVAL, EUNSUPPORTED = -1, -3
P = 1 << 20                        # a 16-byte aligned non-NULL address (pointers are only inspected here, never followed)


def _args(b_mode, K=92, N=128, ldx=None, tail_col=None, **kw):
    # (ell, ell_w, tail_ptr, tail_col, x, ldx, b, ldb, bias, c, ldc, rinv, zout, ldz, rows, K, N, fill_rows, row_slot, sums, ghost,
    #  panel_units, pack_desc, b_mode, stream)
    ld = ldx if ldx is not None else (K + 3) // 4 * 4
    a = [P, 16, P, tail_col, P, ld, P, 128, P, P, 128, P, P, ld, 1000, K, N, 8, P, P, P, 0, None, b_mode, None]
    for k, v in kw.items():
        a[int(k[1:])] = v
    return a


def test_mode_entry_refuses_on_the_host():
    """the default arguments carry a tail pointer without tail columns — EINVAL, the LAST host check before the launch: a call that
    meets an earlier refusal answers with that one"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    fn, old = L.tsgnn_gather_rowgemm_st_mode_f32, L.tsgnn_gather_rowgemm_st_f32
    for mode in (0, 1, 2):
        assert fn(*_args(mode)) == EINVAL                          # accepted up to the tail check
    # b_mode outside 0..2: EINVAL even where every valid mode answers EUNSUPPORTED
    for mode in (0, 1, 2):
        assert fn(*_args(mode, N=96)) == EUNSUPPORTED
    for mode in (-1, 3, 7):
        assert fn(*_args(mode, N=96)) == EINVAL
        assert fn(*_args(mode, tail_col=P)) == EINVAL              # (otherwise launchable arguments: refused before the launch)
    # the direct mode where it does not apply
    for N in (32, 64, 96):
        assert fn(*_args(2, N=N, tail_col=P)) == EUNSUPPORTED
    assert fn(*_args(2, K=132, tail_col=P)) == EUNSUPPORTED
    assert fn(*_args(2, K=256, tail_col=P)) == EUNSUPPORTED
    # what the old entry refuses, the mode entry refuses the same way in every mode
    cases = [dict(a0=None), dict(a4=None), dict(a6=None), dict(a18=None), dict(a19=None), dict(a14=0), dict(a17=-1),       # EINVAL
             dict(a5=88), dict(a10=124),                                                                               # ldx < K, ldc < N
             dict(a1=5), dict(a1=24, tail_col=P), dict(a1=32),                                                         # table widths / schedule + tail
             dict(N=132, a10=132), dict(N=96), dict(K=132), dict(a7=126), dict(a0=P + 4), dict(a19=P + 8),             # EUNSUPPORTED
             dict(a13=90), dict(a12=P + 4), dict(a9=P + 8), dict(a8=P + 4), dict(a10=130), dict(N=126)]
    for kw in cases:
        want = old(*(_args(0, **kw)[:23] + [None]))
        assert want in (EINVAL, EUNSUPPORTED), (kw, want)
        for mode in (0, 1, 2):
            assert fn(*_args(mode, **kw)) == want, (kw, mode)
