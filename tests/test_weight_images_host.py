"""The trailing arguments that carry fragment-major weight images (csrc/pack_body.h, csrc/rowgemm_body.h BIMG) are validated on the
host, before anything is launched: the pack descriptor of tsgnn_gather_rowgemm_st_f32, the image of tsgnn_sage_layer_fwd_bn_f32 and of
tsgnn_sage_layer_bwd_f32.  No GPU needed."""
import numpy as np

EINVAL, EUNSUPPORTED = -1, -3
P = 1 << 20                        # a 16-byte aligned non-NULL address (pointers are only inspected here, never followed)


def _fwd_bn_args(w_img, tail_col=None):
    # (ell, ell_w, tail_ptr, tail_col, x, ldx, w, ldw, bias, v, ldv, rinv, zout, ldz, rows, K, fill_rows, graph_ptr, slot_count, B, nslots,
    #  n_ghost, packed, packed_out, row_graph, sums_in, ghost_in, mean_out, rstd_out, row_slot, sums_out, ghost_out, ro_map, ro_map_ch,
    #  panel_units, w_img, stream)
    return (P, 16, P, tail_col, P, 128, P, 128, P, P, 128, P, P, 128, 1000, 128, 8, P, P, 4, 8, 8, P, None, None, P, P, P, P, P, P, P,
            None, 0, 0, w_img, None)


def _bwd_args(w_img, tail_col=None):
    # (ell, ell_w, tail_ptr, tail_col, du, lddu, w, ldw, dxs, lddxs, z, ldz, rows, nslab, rows_per_slab, bias_only_rows, ws, panel_units,
    #  w_img, stream)
    return (P, 16, P, tail_col, P, 128, P, 128, P, 128, P, 128, 1000, 4, 256, 8, P, 0, w_img, None)


def _st_args(desc, tail_col=None):
    # (ell, ell_w, tail_ptr, tail_col, x, ldx, b, ldb, bias, c, ldc, rinv, zout, ldz, rows, K, N, fill_rows, row_slot, sums, ghost,
    #  panel_units, pack_desc, stream)
    return (P, 16, P, tail_col, P, 92, P, 128, P, P, 128, P, P, 92, 1000, 92, 128, 8, P, P, P, 0, desc, None)


def test_image_arguments_validate_on_the_host():
    """every call below is refused on the host, and WHICH refusal it meets tells how far it got: a tail pointer without tail columns is
    EINVAL and is checked after the image / the descriptor, so a call that reaches it had its image (NULL, or aligned) accepted"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    for fn, args in ((L.tsgnn_sage_layer_fwd_bn_f32, _fwd_bn_args), (L.tsgnn_sage_layer_bwd_f32, _bwd_args)):
        assert fn(*args(None)) == EINVAL                           # NULL image: accepted, the tail check answers
        assert fn(*args(P)) == EINVAL                              # aligned image: accepted
        for off in (4, 8, 12):
            assert fn(*args(P + off)) == EUNSUPPORTED              # misaligned image: refused before the tail check
    st = L.tsgnn_gather_rowgemm_st_f32
    assert st(*_st_args(None)) == EINVAL                           # NULL descriptor: accepted, the tail check answers

    def desc(*sets):
        return np.asarray([len(sets)] + [v for s in sets for v in s], np.int64)
    good = (P, 128, 128, 128, 1, P)                                # (w, ldw, K, N, kn, out)
    d = desc(good, good[:4] + (0, P + 65536))
    assert st(*_st_args(d.ctypes.data)) == EINVAL                  # a good descriptor: accepted (the tail check again)
    d = desc(good[:5] + (P + 8,))
    assert st(*_st_args(d.ctypes.data)) == EUNSUPPORTED            # misaligned image
    for bad in (good[:1] + (64,) + good[2:],                       # leading dimension shorter than a row
                (0,) + good[1:], good[:5] + (0,),                  # no matrix / no image
                good[:2] + (129,) + good[3:], good[:3] + (0,) + good[4:]):
        d = desc(bad)
        assert st(*_st_args(d.ctypes.data)) == EINVAL
        assert st(*_st_args(d.ctypes.data, tail_col=P)) == EINVAL   # (a consistent tail: the answer is the descriptor parser's)
    none = np.asarray([0], np.int64)
    many = desc(*([good] * 9))
    for d in (none, many):                                         # set counts outside 1..8
        assert st(*_st_args(d.ctypes.data, tail_col=P)) == EINVAL
    d = desc(good)
    assert st(*_st_args(d.ctypes.data + 4, tail_col=P)) == EINVAL  # the descriptor itself misaligned
