// Mini-batch stream: a NEW mini-batch of B graphs every replay of one hipGraph (train.py:104-131: DataLoader(shuffle=True) -> model ->
// cross-entropy -> clip -> Adam, once per optimiser step).  The contract is csrc/triplet_stream.hip's — the same arena, the same
// [G, 8] records, the same [HEAD | schedule] buffer with its cursor (csrc/stream_protocol.h), the same capacity-padded outputs and
// the same row body (csrc/sage_gather_row.h) — for entries of up to 128 graphs: what that kernel does by walking all B records in
// every thread (B <= 8) is done here once per workgroup in LDS.
//
//   prologue   the first B threads load the entry's records; the first two waves form the inclusive prefix sums of n and ntail with
//              wave shuffles (wave 1 adds wave 0's total through LDS), and — in the workgroups that hold ghost rows — the count of
//              graphs with n > s for the workgroup's (at most 8) ghost slots by one ballot per slot: n is in the register of the
//              thread that loaded the record, so a slot's count costs no LDS read per graph.
//   per row    a binary search over the prefix (at most 7 LDS reads, the same address in all 32 lanes of a row) finds the row's
//              graph; one 16-byte LDS read fetches that graph's offsets.
//
// Dependent loads of a row: cursor -> schedule entry -> records -> row pointers -> columns, as before; the features need the first
// three only, and in the one-hot mode the node's label instead of a table row.
#include "sage_gather_row.h"
#include "stream_protocol.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int BS_REC = 8;                 // int32 words of a record: n, nnz, ntail, first row, first entry, first tail entry, id, 0

struct BatchGatherArgs {
  const int32_t* rec; int64_t n_graphs;   // [n_graphs][BS_REC]
  const int32_t* labels;                  // [n_graphs]
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  int32_t *graph_ptr, *ids_out; int64_t* label_out;
  SageRowIo io;
};

// 8 rows per block, the lanes' roles as sage_gather_row.h has them
__global__ __launch_bounds__(256) void batch_gather_kernel(BatchGatherArgs a) {
  __shared__ int4 off_s[STREAM_MAX_B];    // first row, first entry, first tail entry, id
  __shared__ int pre_n[STREAM_MAX_B + 1], pre_t[STREAM_MAX_B + 1];      // exclusive prefix sums of n / ntail over the entry's graphs
  __shared__ int wtot_s[2][2];            // wave totals of n / ntail
  __shared__ int cnt_s[2][8];             // per wave: graphs that HAVE this workgroup's k-th row as a slot
  __shared__ long long cur_s;
  const SageRowIo io = a.io;            // (a copy: the arguments are fetched once at entry, not in the branch that uses each)
  const int tid = threadIdx.x;
  const int64_t r_blk = (int64_t)blockIdx.x * 8;
  int n_i = 0, t_i = 0;
  if (tid < io.B) {
    long long cur;
    const int64_t id = stream_entry_id(a.state, a.sched, a.sched_cap, a.n_graphs, io.B, tid, cur);
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + id * BS_REC);
    const int4 r1 = *reinterpret_cast<const int4*>(a.rec + id * BS_REC + 4);
    n_i = r0.x; t_i = r0.z;
    off_s[tid] = make_int4(r0.w, r1.x, r1.y, (int)id);
    if (tid == 0) cur_s = cur;
    if (blockIdx.x == 0) {                                  // the batch's own small arrays: one writer per word
      a.ids_out[tid] = (int32_t)id;
      a.label_out[tid] = (int64_t)a.labels[id];
    }
  }
  if (tid < STREAM_MAX_B && r_blk + 7 >= io.row_cap) {      // (uniform over the workgroup) rows of ghost slots: how many graphs HAVE slot s
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t s = r_blk + k - io.row_cap;
      const unsigned long long m = __ballot(s >= 0 && (int64_t)n_i > s);
      if ((tid & 63) == 0) cnt_s[tid >> 6][k] = __popcll(m);
    }
  }
  two_wave_prefix(n_i, t_i, tid, wtot_s, pre_n, pre_t);

  SageRow w;
  w.r = r_blk + (tid >> 5);
  w.q = tid & 31;
  const int n_tot = pre_n[io.B];
  w.t_tot = pre_t[io.B];
  if (blockIdx.x == 0 && tid <= io.B + 1) {                 // (graph B: the dummy graph of the padding rows)
    const int64_t p = tid <= io.B ? (int64_t)pre_n[tid] : io.row_cap;
    a.graph_ptr[tid] = (int32_t)(p < io.row_cap ? p : io.row_cap);
  }
  if (w.r >= io.row_cap + io.nmax) return;
  // the graph whose rows hold r: the last k with pre_n[k] <= r (every graph has a row, so the prefix is strictly increasing);
  // a trip count that depends on B alone
  int lo = 0, hi = io.B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)pre_n[mid] <= w.r) lo = mid; else hi = mid;
  }
  w.real = w.r < (int64_t)n_tot && w.r < io.row_cap;        // (r < row_cap: the host validator's word, repeated)
  w.b = lo;
  w.g0 = pre_n[lo]; w.t0 = pre_t[lo];
  const int4 o4 = off_s[lo];
  w.row0 = o4.x; w.ent0 = o4.y; w.tail0 = o4.z; w.gid = o4.w;
  // (ghost slot r - row_cap: the prologue's ballots counted it)
  sage_gather_row<true>(io, w, [k = tid >> 5](int) { return cnt_s[0][k] + cnt_s[1][k]; });
  // This workgroup READ the cursor before its first barrier (the value went through LDS), so thread 0 — a neighbour-table lane of a
  // row below total_rows, which never returns early — may draw the workgroup's ticket; here, behind its stores, so that no wave waits
  // for the atomic's round trip in front of its work.  A slot of 32 DD graphs has ~1,400 workgroups: the sharded ticket.
  if (tid == 0) stream_ticket_sharded(a.ticket, a.state, cur_s);
}

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_batch_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t off_rowptr, int64_t off_col,
                           int64_t off_tail_ptr, int64_t off_tail_col, int64_t arena_words, const float* feats, int64_t ldf,
                           const int32_t* node_label, int fin, const int32_t* labels, int64_t max_n, int64_t max_tail,
                           const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket, int B, int nmax, int64_t row_cap,
                           int64_t tail_cap, int ell_w, int32_t* graph_ptr, int32_t* slot_count, int32_t* row_graph, int32_t* row_slot,
                           int32_t* ell, int32_t* tail_ptr, int32_t* tail_col, int32_t* ell_slots, int32_t* tail_slots, float* x,
                           int64_t ldx, int32_t* ids_out, int64_t* label_out, tsgnn_stream_t stream) {
  if (!records || !arena || !labels || !sched || !state || !ticket || !graph_ptr || !slot_count || !row_graph || !row_slot || !ell ||
      !tail_ptr || !tail_col || !x || !ids_out || !label_out || (ell_slots == nullptr) != (tail_slots == nullptr))
    return TSGNN_EINVAL;
  if ((feats == nullptr) == (node_label == nullptr)) return TSGNN_EINVAL;       // a feature table or the nodes' labels, not both
  if (B < 1 || B > STREAM_MAX_B || sched_cap <= 0 || n_graphs <= 0 || nmax <= 0 || row_cap <= 0 || tail_cap < 1 || max_n < 1 || max_tail < 0 ||
      (ell_w != 4 && ell_w != 8 && ell_w != 16))
    return TSGNN_EINVAL;
  if (feats ? ldf <= 0 : (fin < 1 || ldx != ((int64_t)fin + 3) / 4 * 4)) return TSGNN_EINVAL;
  // every graph of the arena fits a slot on its own and within nmax slots (max_n and max_tail are the caller's word, as the arena
  // is).  Whether an ENTRY fits is the uploader's check (minibatch_stream.MiniBatchStream.load): the kernel clamps, so an entry that
  // does not fit cannot write outside the arrays.
  if (row_cap < max_n || tail_cap < max_tail || max_n > nmax) return TSGNN_EINVAL;
  if (off_rowptr < 0 || off_col < off_rowptr || off_tail_ptr < off_col || off_tail_col < off_tail_ptr || arena_words < off_tail_col)
    return TSGNN_EINVAL;
  if (row_cap + nmax >= ((int64_t)1 << 31) / ell_w || sched_cap >= ((int64_t)1 << 31) / B || tail_cap >= ((int64_t)1 << 31))
    return TSGNN_EUNSUPPORTED;
  if (ell_slots && (row_cap + nmax >= (1 << 20) || nmax > 2048)) return TSGNN_EUNSUPPORTED;     // entry = slot << 20 | row
  if ((ldx % 4) || (feats && ldx != ldf) || ((off_rowptr | off_col | off_tail_ptr | off_tail_col) & 3)) return TSGNN_EUNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(feats) |
                       reinterpret_cast<uintptr_t>(ell) | reinterpret_cast<uintptr_t>(ell_slots) | reinterpret_cast<uintptr_t>(x);
  if ((al & 15) || (reinterpret_cast<uintptr_t>(state) & 15) || (reinterpret_cast<uintptr_t>(label_out) & 7)) return TSGNN_EUNSUPPORTED;
  BatchGatherArgs a{records, n_graphs, labels, sched, sched_cap, state, ticket, graph_ptr, ids_out, label_out,
                    {arena + off_rowptr, arena + off_col, arena + off_tail_ptr, arena + off_tail_col, feats, ldf, (int)(ldx / 4), node_label, B,
                     nmax, ell_w, row_cap, tail_cap, slot_count, row_graph, row_slot, ell, tail_ptr, tail_col, ell_slots, tail_slots, x, ldx}};
  TSGNN_KNAME("batch_gather_kernel");
  batch_gather_kernel<<<(unsigned)ceil_div64(row_cap + nmax, 8), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
