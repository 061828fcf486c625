// The row body of the SAGPool streams' gather launches (sag_stream.hip: 3 graphs per entry or 1; sag_batch_stream.hip: B <= 128): one
// row of the capacity-padded batch sag_stack's node reads — its columns, its row pointer, its gcn_norm coefficients and its feature
// row — from the graph the caller found for it.  8 lanes per row, 32 rows per workgroup; the four rows of a 32-lane group leave their
// row pointers and coefficients as one 16-byte store each through the group's first lane.  One writer per word, plain vector stores
// (16 bytes wherever the destination's alignment is known: the feature rows, four rows' row pointers and coefficients per store; the
// columns land at a data-dependent offset and go out as coalesced dwords).
#pragma once
#include "common.h"

constexpr int SAG_EG = 8;                 // lanes per row
constexpr int SAG_ROWS = 256 / SAG_EG;    // rows per workgroup

// the arena's sections, the capacities and the batch's arrays: what both launches' argument structs embed
struct SagRowIo {
  const int32_t *rowptr, *col;            // graph g's n + 1 row pointers (graph-local) start at first row + g
  const float* feats; int64_t ldf; int ld4;
  int64_t row_cap, nnz_cap;
  int32_t *rowptr_out, *col_out; float* x; int64_t ldx; float *dinv, *self_w;
};

// a row r (any row of the grid: rows past row_cap only skip their stores), lane sub of its 8, lane of the wave, and its graph: the
// graph's rows start at g0 and its entries at eb; first row / first entry / index: the graph's record.  real: r is a row of that graph
// (and r < row_cap).  e_tot: the batch's entries, e_end = min(e_tot, nnz_cap): no row pointer leaves col_out.
struct SagRow {
  int64_t r; int sub, lane; bool real;
  int g0, eb, row0, ent0, gid, e_tot, e_end;
};

// every lane of the wave calls it (a ballot and shuffles inside)
__device__ __forceinline__ void sag_gather_row(const SagRowIo& a, const SagRow& w) {
  const int64_t r = w.r;
  const int sub = w.sub, lane = w.lane, g0 = w.g0;
  const bool real = w.real;
  const bool in_cap = r < a.row_cap;
  const int lr = (int)(r - g0);
  int e0 = 0, e1 = 0;
  if (real) {
    const int32_t* rp = a.rowptr + (int64_t)w.row0 + w.gid + lr;
    e0 = rp[0]; e1 = rp[1];
  }
  bool has_self = false;
  for (int e = e0 + sub; e < e1; e += SAG_EG) {
    const int c = a.col[(int64_t)w.ent0 + e];
    has_self |= (c == lr);
    const int64_t o = (int64_t)w.eb + e;
    if (o < a.nnz_cap) a.col_out[o] = c + g0;
  }
  has_self = ((unsigned)(__ballot(has_self) >> (lane & ~(SAG_EG - 1))) & ((1u << SAG_EG) - 1u)) != 0u;
  float di = 0.f, sw = 0.f;
  if (real) gcn_norm_coef(e1 - e0, has_self, di, sw);
  // (an entry that fits never reaches the clamp; one that does not — refused by the host's load — leaves pointers inside col_out)
  int rp_out = real ? w.eb + e0 : w.e_tot;
  rp_out = rp_out < w.e_end ? rp_out : w.e_end;
  {
    const int q0 = lane & ~31;                              // the 32-lane group's first lane: rows r .. r + 3 of a multiple of four
    const int4 rp4 = make_int4(rp_out, __shfl(rp_out, q0 + 8, 64), __shfl(rp_out, q0 + 16, 64), __shfl(rp_out, q0 + 24, 64));
    const float4 di4 = make_float4(di, __shfl(di, q0 + 8, 64), __shfl(di, q0 + 16, 64), __shfl(di, q0 + 24, 64));
    const float4 sw4 = make_float4(sw, __shfl(sw, q0 + 8, 64), __shfl(sw, q0 + 16, 64), __shfl(sw, q0 + 24, 64));
    if ((lane & 31) == 0 && in_cap) {
      if (r + 3 < a.row_cap) {
        *reinterpret_cast<int4*>(a.rowptr_out + r) = rp4;
        *reinterpret_cast<float4*>(a.dinv + r) = di4;
        *reinterpret_cast<float4*>(a.self_w + r) = sw4;
      } else {                                              // the last rows of a capacity that is no multiple of four
        const int rp_[4] = {rp4.x, rp4.y, rp4.z, rp4.w};
        const float di_[4] = {di4.x, di4.y, di4.z, di4.w}, sw_[4] = {sw4.x, sw4.y, sw4.z, sw4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (r + u < a.row_cap) {
            a.rowptr_out[r + u] = rp_[u];
            a.dinv[r + u] = di_[u];
            a.self_w[r + u] = sw_[u];
          }
      }
    }
  }
  if (in_cap) {
    const float4* src = reinterpret_cast<const float4*>(a.feats + ((int64_t)w.row0 + lr) * a.ldf);
    for (int c4 = sub; c4 < a.ld4; c4 += SAG_EG) {
      const float4 v = real ? src[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(a.x + r * a.ldx + 4 * c4) = v;
    }
  }
}
