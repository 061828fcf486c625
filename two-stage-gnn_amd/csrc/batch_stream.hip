// Mini-batch stream: a NEW mini-batch of B graphs every replay of one hipGraph (train.py:104-131: DataLoader(shuffle=True) -> model ->
// cross-entropy -> clip -> Adam, once per optimiser step).  The contract is csrc/triplet_stream.hip's — the same arena, the same
// [G, 8] records, the same [HEAD | schedule] buffer with its cursor, the same capacity-padded outputs — for
// entries of up to 128 graphs: what that kernel does by walking all B records in every thread (B <= 8) is done here once per
// workgroup in LDS.
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
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int BS_MAX_B = 128;
constexpr int BS_SHARDS = 32, BS_SHARD_WORDS = 32;       // ticket counters: 32 shards + the top, each on 128 bytes of its own
constexpr int BS_REC = 8;                 // int32 words of a record: n, nnz, ntail, first row, first entry, first tail entry, id, 0

struct BatchGatherArgs {
  const int32_t* rec;                     // [n_graphs][BS_REC]
  const int32_t *rowptr, *col, *tptr, *tcol;   // the arena's sections: graph g's row pointers are rowptr[first row + g ..][n + 1]
  const float* feats; int64_t ldf; int ld4;    // feats == nullptr: one-hot rows of node_label (fin columns, ld4 float4 per row)
  const int32_t* node_label;
  const int32_t* labels;                  // [n_graphs]
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  int B, nmax, ell_w; int64_t row_cap, tail_cap;
  int32_t *graph_ptr, *slot_count, *row_graph, *row_slot, *ell, *tail_ptr, *tail_col, *ell_slots, *tail_slots;
  float* x; int64_t ldx; int32_t* ids_out; int64_t* label_out;
};

// 32 lanes per row, 8 rows per block, the lanes' roles as in triplet_gather_kernel: q < ell_w/4 four entries of the row's neighbour
// table (and of its slot-annotated copy), q == ell_w/4 the row maps, the tail pointer, the row's share of the CSR tail and — on a
// ghost row — its slot's count, the lanes after that the feature row (float4 each, looping).
__global__ __launch_bounds__(256) void batch_gather_kernel(BatchGatherArgs a) {
  __shared__ int4 off_s[BS_MAX_B];        // first row, first entry, first tail entry, id
  __shared__ int pre_n[BS_MAX_B + 1], pre_t[BS_MAX_B + 1];      // exclusive prefix sums of n / ntail over the entry's graphs
  __shared__ int wtot_s[2][2];            // wave totals of n / ntail
  __shared__ int cnt_s[2][8];             // per wave: graphs that HAVE this workgroup's k-th row as a slot
  __shared__ long long cur_s;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int64_t r_blk = (int64_t)blockIdx.x * 8;
  int n_i = 0, t_i = 0;
  if (tid < a.B) {
    // (agent-scope load: the word is stored by the last workgroup of the previous launch, never through this CU's scalar cache)
    const long long cur = __hip_atomic_load(reinterpret_cast<long long*>(a.state), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int64_t T = a.state[1];                                 // the loaded schedule's length: the host's word, kept inside the buffer
    T = T < 1 ? 1 : (T > a.sched_cap ? a.sched_cap : T);
    const int64_t c = (int64_t)((unsigned long long)cur % (unsigned long long)T);
    const int id = a.sched[c * a.B + tid];
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + (int64_t)id * BS_REC);
    const int4 r1 = *reinterpret_cast<const int4*>(a.rec + (int64_t)id * BS_REC + 4);
    n_i = r0.x; t_i = r0.z;
    off_s[tid] = make_int4(r0.w, r1.x, r1.y, id);
    if (tid == 0) cur_s = cur;
    if (blockIdx.x == 0) {                                  // the batch's own small arrays: one writer per word
      a.ids_out[tid] = id;
      a.label_out[tid] = (int64_t)a.labels[id];
    }
  }
  int sn = n_i, st = t_i;
  if (tid < BS_MAX_B) {                                     // waves 0 and 1, whole waves: threads past B carry zeros
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int un = __shfl_up(sn, d, 64), ut = __shfl_up(st, d, 64);
      if (lane >= d) { sn += un; st += ut; }
    }
    if (lane == 63) { wtot_s[wave][0] = sn; wtot_s[wave][1] = st; }
    if (r_blk + 7 >= a.row_cap) {                           // (uniform over the workgroup) rows of ghost slots: how many graphs HAVE slot s
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t s = r_blk + k - a.row_cap;
        const unsigned long long m = __ballot(s >= 0 && (int64_t)n_i > s);
        if (lane == 0) cnt_s[wave][k] = __popcll(m);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    pre_n[0] = 0; pre_t[0] = 0;
  }
  if (tid < BS_MAX_B) {
    pre_n[tid + 1] = sn + (wave ? wtot_s[0][0] : 0);
    pre_t[tid + 1] = st + (wave ? wtot_s[0][1] : 0);
  }
  __syncthreads();

  const int64_t r = r_blk + (tid >> 5);
  const int q = tid & 31;
  const int n_tot = pre_n[a.B], t_tot = pre_t[a.B];
  if (blockIdx.x == 0 && tid <= a.B + 1) {                  // (graph B: the dummy graph of the padding rows)
    const int64_t p = tid <= a.B ? (int64_t)pre_n[tid] : a.row_cap;
    a.graph_ptr[tid] = (int32_t)(p < a.row_cap ? p : a.row_cap);
  }
  const int64_t total_rows = a.row_cap + a.nmax;
  if (r >= total_rows) return;
  // the graph whose rows hold r: the last k with pre_n[k] <= r (every graph has a row, so the prefix is strictly increasing);
  // a trip count that depends on B alone
  int lo = 0, hi = a.B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)pre_n[mid] <= r) lo = mid; else hi = mid;
  }
  const bool real = r < (int64_t)n_tot && r < a.row_cap;    // (r < row_cap: the host validator's word, repeated)
  const int b = lo;
  const int g0 = pre_n[b], t0 = pre_t[b];
  const int4 o4 = off_s[b];
  const int row0 = o4.x, ent0 = o4.y, tail0 = o4.z, gid = o4.w;
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
      const int k = (int)(r - r_blk);                       // ghost slot r - row_cap: the prologue's ballots counted it
      a.slot_count[r - a.row_cap] = cnt_s[0][k] + cnt_s[1][k];
    }
    int e_lo = 0, e_hi = 0;
    if (real) {
      const int32_t* tp = a.tptr + (int64_t)row0 + gid + lr;
      e_lo = tp[0]; e_hi = tp[1];
    }
    // (an entry that fits never reaches the clamps; one that does not — refused by the host's load — leaves pointers inside tail_col)
    const int64_t tp_r = real ? (int64_t)t0 + e_lo : (int64_t)t_tot;
    const int32_t t_end = (int32_t)((int64_t)t_tot < a.tail_cap ? (int64_t)t_tot : a.tail_cap);
    a.tail_ptr[r] = tp_r < a.tail_cap ? (int32_t)tp_r : (int32_t)a.tail_cap;
    if (r == total_rows - 1) a.tail_ptr[total_rows] = t_end;
    for (int e = e_lo; e < e_hi; ++e) {                     // rows with more than ell_w neighbours: few
      const int64_t o = (int64_t)t0 + e;
      if (o >= a.tail_cap) break;
      const int j = a.tcol[(int64_t)tail0 + e];
      a.tail_col[o] = j + g0;
      if (a.tail_slots) a.tail_slots[o] = (j << 20) | (j + g0);
    }
  } else if (a.feats) {
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
  // This workgroup READ the cursor before its first barrier (the value went through LDS), so thread 0 — a neighbour-table lane of a
  // row below total_rows, which never returns early — may draw the workgroup's ticket; here, behind its stores, so that no wave waits
  // for the atomic's round trip in front of its work.  Atomics execute at the memory side, one after the other on one line, and a
  // slot of 32 DD graphs has ~1,400 workgroups: the tickets are drawn in two levels.  Workgroup b draws from shard b % 32 (a counter
  // on 128 bytes of its own); the workgroup that draws a shard's last ticket leaves the shard at zero and draws from the top counter;
  // the one that draws the top's last knows that all have read the cursor, leaves the top at zero and advances the cursor.  Nobody
  // waits for anybody.
  if (tid == 0) {
    const long long cur = cur_s;
    const unsigned S = gridDim.x < (unsigned)BS_SHARDS ? gridDim.x : (unsigned)BS_SHARDS;
    const unsigned s = blockIdx.x % S;
    const unsigned members = (gridDim.x - s + S - 1) / S;   // workgroups b < gridDim.x with b % S == s
    unsigned* shard = a.ticket + s * BS_SHARD_WORDS;
    if (atomicAdd(shard, 1u) == members - 1) {
      atomicExch(shard, 0u);
      unsigned* top = a.ticket + BS_SHARDS * BS_SHARD_WORDS;
      if (atomicAdd(top, 1u) == S - 1) {
        atomicExch(top, 0u);
        __hip_atomic_store(reinterpret_cast<long long*>(a.state), cur + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
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
  if (B < 1 || B > BS_MAX_B || sched_cap <= 0 || n_graphs <= 0 || nmax <= 0 || row_cap <= 0 || tail_cap < 1 || max_n < 1 || max_tail < 0 ||
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
  BatchGatherArgs a{records, arena + off_rowptr, arena + off_col, arena + off_tail_ptr, arena + off_tail_col, feats, ldf, (int)(ldx / 4),
                    node_label, labels, sched, sched_cap, state, ticket, B, nmax, ell_w, row_cap, tail_cap, graph_ptr, slot_count, row_graph,
                    row_slot, ell, tail_ptr, tail_col, ell_slots, tail_slots, x, ldx, ids_out, label_out};
  TSGNN_KNAME("batch_gather_kernel");
  batch_gather_kernel<<<(unsigned)ceil_div64(row_cap + nmax, 8), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
