// Triplet stream: a NEW triplet every replay of one hipGraph (train_triplet.py:247-287: tripletsampler_tr.sampler() -> TNet(a, p, n)
// -> margin loss -> clip -> Adam, once per optimiser step).  The dataset is small and fixed, so it lives on the device whole (the
// "arena", packed once by triplet_stream.pack_arena: per-graph records, one int32 buffer of graph-local CSR rows and CSR tails, one
// feature table); the sampler's epoch is an index array [T, B] that goes up once, its length and the cursor beside it.  ONE launch
// per step reads "entry number cursor" of that schedule and writes the capacity-padded batch (csrc/ingest.hip: rows [0, n) real, [n, row_cap) padding of a dummy graph,
// [row_cap, +nmax) ghost slots) the step's kernels read — what tsgnn_host_collate_compact + the pull + the expansion do for a
// mini-batch that crosses PCIe, without a host in the loop.
//
// A batch is at most 8 graphs, so every prefix a collate needs (first row and first tail entry of each graph) is a sum over at most
// 8 numbers: each workgroup forms them itself from the B records (LDS, uniform control flow).  Dependent loads of a row:
// cursor -> schedule entry -> records -> row pointers -> columns; the features need the first three only.
#include "sage_gather_row.h"
#include "stream_protocol.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int TS_MAX_B = 8;
constexpr int TS_REC = 8;                 // int32 words of a record: n, nnz, ntail, first row, first entry, first tail entry, id, 0

struct GatherArgs {
  const int32_t* rec; int64_t n_graphs;   // [n_graphs][TS_REC]
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  int32_t *graph_ptr, *ids_out;
  SageRowIo io;
};

// 8 rows per block, the lanes' roles as sage_gather_row.h has them.  Cursor and ticket counter: csrc/stream_protocol.h.
__global__ __launch_bounds__(256) void triplet_gather_kernel(GatherArgs a) {
  __shared__ int32_t rec_s[TS_MAX_B][TS_REC];
  __shared__ long long cur_s;
  const SageRowIo io = a.io;            // (a copy: the arguments are fetched once at entry, not in the branch that uses each)
  const int tid = threadIdx.x;
  if (tid < io.B) {
    long long cur;
    const int64_t id = stream_entry_id(a.state, a.sched, a.sched_cap, a.n_graphs, io.B, tid, cur);
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + id * TS_REC);
    const int4 r1 = *reinterpret_cast<const int4*>(a.rec + id * TS_REC + 4);
    rec_s[tid][0] = r0.x; rec_s[tid][1] = r0.y; rec_s[tid][2] = r0.z; rec_s[tid][3] = r0.w;
    rec_s[tid][4] = r1.x; rec_s[tid][5] = r1.y; rec_s[tid][6] = (int32_t)id; rec_s[tid][7] = 0;
    if (tid == 0) cur_s = cur;
  }
  __syncthreads();
  // Every workgroup has READ the cursor by now (its value went through LDS), so it may draw its ticket
  if (tid == 0) stream_ticket_flat(a.ticket, gridDim.x, a.state, cur_s);

  SageRow w;
  w.r = (int64_t)blockIdx.x * 8 + (tid >> 5);
  w.q = tid & 31;
  // the graph whose rows hold r, and the batch's totals: one pass over the B records, no data-dependent branch
  int n_tot = 0, t_tot = 0;
  w.b = io.B; w.g0 = w.t0 = w.row0 = w.ent0 = w.tail0 = w.gid = 0;
  for (int k = 0; k < io.B; ++k) {
    const int nk = rec_s[k][0], tk = rec_s[k][2];
    const bool mine = w.r >= n_tot && w.r < (int64_t)n_tot + nk;
    w.b = mine ? k : w.b;
    w.g0 = mine ? n_tot : w.g0;
    w.t0 = mine ? t_tot : w.t0;
    w.row0 = mine ? rec_s[k][3] : w.row0;
    w.ent0 = mine ? rec_s[k][4] : w.ent0;
    w.tail0 = mine ? rec_s[k][5] : w.tail0;
    w.gid = mine ? rec_s[k][6] : w.gid;
    n_tot += nk;
    t_tot += tk;
  }
  w.t_tot = t_tot;
  if (blockIdx.x == 0) {                                    // the batch's own small arrays: one writer per word
    if (tid <= io.B + 1) {
      int p = 0;
      for (int k = 0; k < io.B; ++k) p += k < tid ? rec_s[k][0] : 0;
      a.graph_ptr[tid] = tid <= io.B ? p : (int32_t)io.row_cap;     // (graph B: the dummy graph of the padding rows)
    }
    if (tid < io.B) a.ids_out[tid] = rec_s[tid][6];
  }
  if (w.r >= io.row_cap + io.nmax) return;
  w.real = w.b < io.B && w.r < io.row_cap;                  // (r < row_cap: the host validator's word, repeated)
  sage_gather_row<false>(io, w, [B = io.B](int s) {     // ghost slot s: how many graphs of the batch HAVE it
    int have = 0;
    for (int k = 0; k < B; ++k) have += rec_s[k][0] > s ? 1 : 0;
    return have;
  });
}

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_triplet_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t off_rowptr, int64_t off_col,
                             int64_t off_tail_ptr, int64_t off_tail_col, int64_t arena_words, const float* feats, int64_t ldf,
                             int64_t need_rows, int64_t need_tail, const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket,
                             int B, int nmax, int64_t row_cap, int64_t tail_cap, int ell_w, int32_t* graph_ptr, int32_t* slot_count,
                             int32_t* row_graph, int32_t* row_slot, int32_t* ell, int32_t* tail_ptr, int32_t* tail_col,
                             int32_t* ell_slots, int32_t* tail_slots, float* x, int64_t ldx, int32_t* ids_out, tsgnn_stream_t stream) {
  if (!records || !arena || !feats || !sched || !state || !ticket || !graph_ptr || !slot_count || !row_graph || !row_slot || !ell ||
      !tail_ptr || !tail_col || !x || !ids_out || (ell_slots == nullptr) != (tail_slots == nullptr))
    return TSGNN_EINVAL;
  if (B < 1 || B > TS_MAX_B || sched_cap <= 0 || n_graphs <= 0 || nmax <= 0 || row_cap <= 0 || tail_cap < 1 || ldf <= 0 || need_rows < 0 ||
      need_tail < 0 || (ell_w != 4 && ell_w != 8 && ell_w != 16))
    return TSGNN_EINVAL;
  // no schedule entry can overflow a slot: the capacities cover the arena's bounds (B times its largest n / ntail).  need_rows and
  // need_tail are the caller's word, as the arena is: this guards a slot built too small for the arena it is used with, it cannot
  // tell bounds that belong to another arena.
  if (row_cap < need_rows || tail_cap < need_tail) return TSGNN_EINVAL;
  if (off_rowptr < 0 || off_col < off_rowptr || off_tail_ptr < off_col || off_tail_col < off_tail_ptr || arena_words < off_tail_col)
    return TSGNN_EINVAL;
  if (row_cap + nmax >= ((int64_t)1 << 31) / ell_w || sched_cap >= ((int64_t)1 << 31) / B) return TSGNN_EUNSUPPORTED;
  if (ell_slots && (row_cap + nmax >= (1 << 20) || nmax > 2048)) return TSGNN_EUNSUPPORTED;     // entry = slot << 20 | row
  if ((ldf % 4) || ldx != ldf || ((off_rowptr | off_col | off_tail_ptr | off_tail_col) & 3)) return TSGNN_EUNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(feats) |
                       reinterpret_cast<uintptr_t>(ell) | reinterpret_cast<uintptr_t>(ell_slots) | reinterpret_cast<uintptr_t>(x);
  if ((al & 15) || (reinterpret_cast<uintptr_t>(state) & 15)) return TSGNN_EUNSUPPORTED;
  GatherArgs a{records, n_graphs, sched, sched_cap, state, ticket, graph_ptr, ids_out,
               {arena + off_rowptr, arena + off_col, arena + off_tail_ptr, arena + off_tail_col, feats, ldf, (int)(ldf / 4), nullptr, B, nmax,
                ell_w, row_cap, tail_cap, slot_count, row_graph, row_slot, ell, tail_ptr, tail_col, ell_slots, tail_slots, x, ldx}};
  TSGNN_KNAME("triplet_gather_kernel");
  triplet_gather_kernel<<<(unsigned)ceil_div64(row_cap + nmax, 8), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
