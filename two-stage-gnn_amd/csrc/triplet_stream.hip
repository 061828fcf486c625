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
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int TS_MAX_B = 8;
constexpr int TS_REC = 8;                 // int32 words of a record: n, nnz, ntail, first row, first entry, first tail entry, id, 0

struct GatherArgs {
  const int32_t* rec;                     // [n_graphs][TS_REC]
  const int32_t *rowptr, *col, *tptr, *tcol;   // the arena's sections: graph g's row pointers are rowptr[first row + g ..][n + 1]
  const float* feats; int64_t ldf; int ld4;
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  int B, nmax, ell_w; int64_t row_cap, tail_cap;
  int32_t *graph_ptr, *slot_count, *row_graph, *row_slot, *ell, *tail_ptr, *tail_col, *ell_slots, *tail_slots;
  float* x; int64_t ldx; int32_t* ids_out;
};

// 32 lanes per row, 8 rows per block (expand_row_lane's shape, csrc/ingest_rider.h).  Lane q of a row: q < ell_w/4 four entries of
// the row's neighbour table (and of its slot-annotated copy), q == ell_w/4 the row maps, the tail pointer, the row's share of the CSR
// tail and — on a ghost row — its slot's count, the lanes after that the feature row (float4 each, looping).
__global__ __launch_bounds__(256) void triplet_gather_kernel(GatherArgs a) {
  __shared__ int32_t rec_s[TS_MAX_B][TS_REC];
  __shared__ long long cur_s;
  const int tid = threadIdx.x;
  if (tid < a.B) {
    // (agent-scope load: the word is stored by the last workgroup of the previous launch, never through this CU's scalar cache)
    const long long cur = __hip_atomic_load(reinterpret_cast<long long*>(a.state), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int64_t T = a.state[1];                                 // the loaded schedule's length: the host's word, kept inside the buffer
    T = T < 1 ? 1 : (T > a.sched_cap ? a.sched_cap : T);
    const int64_t c = (int64_t)((unsigned long long)cur % (unsigned long long)T);
    const int id = a.sched[c * a.B + tid];
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + (int64_t)id * TS_REC);
    const int4 r1 = *reinterpret_cast<const int4*>(a.rec + (int64_t)id * TS_REC + 4);
    rec_s[tid][0] = r0.x; rec_s[tid][1] = r0.y; rec_s[tid][2] = r0.z; rec_s[tid][3] = r0.w;
    rec_s[tid][4] = r1.x; rec_s[tid][5] = r1.y; rec_s[tid][6] = id; rec_s[tid][7] = 0;
    if (tid == 0) cur_s = cur;
  }
  __syncthreads();
  // Every workgroup has READ the cursor by now (its value went through LDS), so it may draw its ticket: the workgroup that draws the
  // last one knows that all have, leaves the counter at zero for the next launch and advances the cursor.
  if (tid == 0) {
    const unsigned t = atomicAdd(a.ticket, 1u);
    if (t == gridDim.x - 1) {
      atomicExch(a.ticket, 0u);
      __hip_atomic_store(reinterpret_cast<long long*>(a.state), cur_s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  const int64_t r = (int64_t)blockIdx.x * 8 + (tid >> 5);
  const int q = tid & 31;
  // the graph whose rows hold r, and the batch's totals: one pass over the B records, no data-dependent branch
  int n_tot = 0, t_tot = 0;
  int b = a.B, g0 = 0, t0 = 0, row0 = 0, ent0 = 0, tail0 = 0, gid = 0;
  for (int k = 0; k < a.B; ++k) {
    const int nk = rec_s[k][0], tk = rec_s[k][2];
    const bool mine = r >= n_tot && r < (int64_t)n_tot + nk;
    b = mine ? k : b;
    g0 = mine ? n_tot : g0;
    t0 = mine ? t_tot : t0;
    row0 = mine ? rec_s[k][3] : row0;
    ent0 = mine ? rec_s[k][4] : ent0;
    tail0 = mine ? rec_s[k][5] : tail0;
    gid = mine ? rec_s[k][6] : gid;
    n_tot += nk;
    t_tot += tk;
  }
  if (blockIdx.x == 0) {                                    // the batch's own small arrays: one writer per word
    if (tid <= a.B + 1) {
      int p = 0;
      for (int k = 0; k < a.B; ++k) p += k < tid ? rec_s[k][0] : 0;
      a.graph_ptr[tid] = tid <= a.B ? p : (int32_t)a.row_cap;       // (graph B: the dummy graph of the padding rows)
    }
    if (tid < a.B) a.ids_out[tid] = rec_s[tid][6];
  }
  const int64_t total_rows = a.row_cap + a.nmax;
  if (r >= total_rows) return;
  const bool real = b < a.B && r < a.row_cap;               // (r < row_cap: the host validator's word, repeated)
  const int lr = (int)(r - g0);
  const int EQ = a.ell_w >> 2;
  if (q < EQ) {
    int4 v = make_int4(-1, -1, -1, -1), w = v;
    if (real) {
      const int32_t* rp = a.rowptr + (int64_t)row0 + gid + lr;
      const int e0 = rp[0], d = rp[1] - e0;
      const int32_t* c = a.col + (int64_t)ent0 + e0;
      const int k = 4 * q;
      if (k < d) { const int j = c[k]; v.x = j + g0; w.x = (j << 20) | v.x; }
      if (k + 1 < d) { const int j = c[k + 1]; v.y = j + g0; w.y = (j << 20) | v.y; }
      if (k + 2 < d) { const int j = c[k + 2]; v.z = j + g0; w.z = (j << 20) | v.z; }
      if (k + 3 < d) { const int j = c[k + 3]; v.w = j + g0; w.w = (j << 20) | v.w; }
    }
    *reinterpret_cast<int4*>(a.ell + r * a.ell_w + 4 * q) = v;
    if (a.ell_slots) *reinterpret_cast<int4*>(a.ell_slots + r * a.ell_w + 4 * q) = w;
  } else if (q == EQ) {
    if (r < a.row_cap) {
      a.row_graph[r] = real ? b : a.B;                      // (padding rows of the capacity: the dummy graph, no slot)
      a.row_slot[r] = real ? lr : -1;
    } else {
      const int s = (int)(r - a.row_cap);                   // ghost slot s: how many graphs of the batch HAVE it
      int have = 0;
      for (int k = 0; k < a.B; ++k) have += rec_s[k][0] > s ? 1 : 0;
      a.slot_count[s] = have;
    }
    int e_lo = 0, e_hi = 0;
    if (real) {
      const int32_t* tp = a.tptr + (int64_t)row0 + gid + lr;
      e_lo = tp[0]; e_hi = tp[1];
    }
    a.tail_ptr[r] = real ? t0 + e_lo : t_tot;
    if (r == total_rows - 1) a.tail_ptr[total_rows] = t_tot;
    for (int e = e_lo; e < e_hi; ++e) {                     // rows with more than ell_w neighbours: few
      const int64_t o = (int64_t)t0 + e;
      if (o >= a.tail_cap) break;
      const int j = a.tcol[(int64_t)tail0 + e];
      a.tail_col[o] = j + g0;
      if (a.tail_slots) a.tail_slots[o] = (j << 20) | (j + g0);
    }
  } else {
    const float4* src = reinterpret_cast<const float4*>(a.feats + ((int64_t)row0 + lr) * a.ldf);
    for (int c4 = q - EQ - 1; c4 < a.ld4; c4 += 32 - EQ - 1) {
      const float4 v = real ? src[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(a.x + r * a.ldx + 4 * c4) = v;
    }
  }
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
  GatherArgs a{records, arena + off_rowptr, arena + off_col, arena + off_tail_ptr, arena + off_tail_col, feats, ldf, (int)(ldf / 4),
               sched, sched_cap, state, ticket, B, nmax, ell_w, row_cap, tail_cap, graph_ptr, slot_count, row_graph, row_slot, ell, tail_ptr,
               tail_col, ell_slots, tail_slots, x, ldx, ids_out};
  TSGNN_KNAME("triplet_gather_kernel");
  triplet_gather_kernel<<<(unsigned)ceil_div64(row_cap + nmax, 8), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
