// The row body of the GraphSage streams' gather launches (triplet_stream.hip: B <= 8 graphs per entry; batch_stream.hip: B <= 128):
// one row of the capacity-padded batch (csrc/ingest.hip: rows [0, n) real, [n, row_cap) padding of a dummy graph, [row_cap, +nmax)
// ghost slots) from the graph the caller found for it.  32 lanes per row (expand_row_lane's shape, csrc/ingest_rider.h).  Lane q of a
// row: q < ell_w/4 four entries of the row's neighbour table (and of its slot-annotated copy), q == ell_w/4 the row maps, the tail
// pointer, the row's share of the CSR tail and — on a ghost row — its slot's count, the lanes after that the feature row (float4 each,
// looping).
#pragma once
#include "common.h"

// the arena's sections, the capacities and the batch's arrays: what both launches' argument structs embed
struct SageRowIo {
  const int32_t *rowptr, *col, *tptr, *tcol;   // graph g's row pointers are rowptr[first row + g ..][n + 1]
  const float* feats; int64_t ldf; int ld4;    // feats == nullptr (ONE_HOT launches only): one-hot rows of node_label, ld4 float4 per row
  const int32_t* node_label;
  int B, nmax, ell_w; int64_t row_cap, tail_cap;
  int32_t *slot_count, *row_graph, *row_slot, *ell, *tail_ptr, *tail_col, *ell_slots, *tail_slots;
  float* x; int64_t ldx;
};

// a row r < row_cap + nmax and its graph: entry b of the batch, whose rows start at g0 and whose tail entries at t0 (t_tot: the batch's
// tail entries); first row / first entry / first tail entry / index: the graph's record.  real: r is a row of graph b (and r < row_cap)
struct SageRow {
  int64_t r; int q; bool real;
  int b, g0, t0, t_tot, row0, ent0, tail0, gid;
};

// ghost_count(s): how many graphs of the entry HAVE slot s; evaluated on the q == ell_w/4 lane of a ghost row only
template <bool ONE_HOT, class GhostCount>
__device__ __forceinline__ void sage_gather_row(const SageRowIo& a, const SageRow& w, GhostCount ghost_count) {
  const int64_t r = w.r, total_rows = a.row_cap + a.nmax;
  const int q = w.q, g0 = w.g0, row0 = w.row0, gid = w.gid;
  const bool real = w.real;
  const int lr = (int)(r - g0);
  const int EQ = a.ell_w >> 2;
  if (q < EQ) {
    int4 v = make_int4(-1, -1, -1, -1), s = v;
    if (real) {
      const int32_t* rp = a.rowptr + (int64_t)row0 + gid + lr;
      const int e0 = rp[0], d = rp[1] - e0;
      const int32_t* c = a.col + (int64_t)w.ent0 + e0;
      const int k = 4 * q;
      if (k < d) { const int j = c[k]; v.x = j + g0; s.x = (j << 20) | v.x; }
      if (k + 1 < d) { const int j = c[k + 1]; v.y = j + g0; s.y = (j << 20) | v.y; }
      if (k + 2 < d) { const int j = c[k + 2]; v.z = j + g0; s.z = (j << 20) | v.z; }
      if (k + 3 < d) { const int j = c[k + 3]; v.w = j + g0; s.w = (j << 20) | v.w; }
    }
    *reinterpret_cast<int4*>(a.ell + r * a.ell_w + 4 * q) = v;
    if (a.ell_slots) *reinterpret_cast<int4*>(a.ell_slots + r * a.ell_w + 4 * q) = s;
  } else if (q == EQ) {
    if (r < a.row_cap) {
      a.row_graph[r] = real ? w.b : a.B;                    // (padding rows of the capacity: the dummy graph, no slot)
      a.row_slot[r] = real ? lr : -1;
    } else {
      a.slot_count[r - a.row_cap] = ghost_count((int)(r - a.row_cap));
    }
    int e_lo = 0, e_hi = 0;
    if (real) {
      const int32_t* tp = a.tptr + (int64_t)row0 + gid + lr;
      e_lo = tp[0]; e_hi = tp[1];
    }
    // (an entry that fits never reaches the clamps; one that does not — refused by the host's load — leaves pointers inside tail_col)
    const int64_t tp_r = real ? (int64_t)w.t0 + e_lo : (int64_t)w.t_tot;
    const int32_t t_end = (int32_t)((int64_t)w.t_tot < a.tail_cap ? (int64_t)w.t_tot : a.tail_cap);
    a.tail_ptr[r] = tp_r < a.tail_cap ? (int32_t)tp_r : (int32_t)a.tail_cap;
    if (r == total_rows - 1) a.tail_ptr[total_rows] = t_end;
    for (int e = e_lo; e < e_hi; ++e) {                     // rows with more than ell_w neighbours: few
      const int64_t o = (int64_t)w.t0 + e;
      if (o >= a.tail_cap) break;
      const int j = a.tcol[(int64_t)w.tail0 + e];
      a.tail_col[o] = j + g0;
      if (a.tail_slots) a.tail_slots[o] = (j << 20) | (j + g0);
    }
  } else if (!ONE_HOT || a.feats) {
    const float4* src = reinterpret_cast<const float4*>(a.feats + ((int64_t)row0 + lr) * a.ldf);
    for (int c4 = q - EQ - 1; c4 < a.ld4; c4 += 32 - EQ - 1) {
      const float4 v = real ? src[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(a.x + r * a.ldx + 4 * c4) = v;
    }
  } else {
    // one-hot rows of the TU "node-label" features (train.py:227-231): 1 in column node_label, +0 elsewhere
    const int lab = real ? a.node_label[(int64_t)row0 + lr] : -1;
    for (int c4 = q - EQ - 1; c4 < a.ld4; c4 += 32 - EQ - 1) {
      const int c = 4 * c4;
      const float4 v = make_float4(lab == c ? 1.f : 0.f, lab == c + 1 ? 1.f : 0.f, lab == c + 2 ? 1.f : 0.f, lab == c + 3 ? 1.f : 0.f);
      *reinterpret_cast<float4*>(a.x + r * a.ldx + 4 * c4) = v;
    }
  }
}
