// SAGPool mini-batch stream: a NEW mini-batch of B graphs every replay of one hipGraph (Code/sag/train.py:181-198: DataLoader(batch_size
// = 128, shuffle=True) -> F.nll_loss(model(data), data.y) -> Adam, once per optimiser step), for sag_layers.Net(use_batch=True).
// csrc/sag_stream.hip writes what sag_stack's node reads of 3 graphs (or 1); this is that launch for entries of 1 <= B <= 128 graphs,
// with the B-graph machinery of csrc/batch_stream.hip: the same arena (sag_stream.pack_arena), the same [HEAD | schedule] buffer with
// its cursor (csrc/stream_protocol.h), the same per-row body (csrc/sag_gather_row.h), and
//
//   prologue   the first B threads load the entry's records; the first two waves form the inclusive prefix sums of n and nnz with
//              wave shuffles (wave 1 adds wave 0's total through LDS)
//   per row    8 lanes per row, 32 rows per workgroup; a binary search over the prefix (at most 7 LDS reads, the same address in all
//              lanes of a row) finds the row's graph, one 16-byte LDS read fetches that graph's offsets
//   workgroup 0   ids_out [B], label_out [B] (int64: what mp.nll_loss folds into the head's backward) and the graph pointer of EVERY
//              level, gp [depth + 1][ldg]: one thread per graph applies k = min(n, ceilf(ratio * (float)n)) level after level, an LDS
//              scan per level forms the prefix, every word is clamped to its level's capacity, words past B repeat the total
//
// The capacities may lie below B times the largest graph (sag_stream.MiniBatchStream.load checks every entry on the host): for an entry
// that does not fit, rows and entries past the capacities are dropped and every pointer is clamped, so nothing is written outside the
// arrays.  One writer per word, plain vector stores, and the sharded ticket words (32 shards + the top, 128 bytes each) are the only
// atomics.
#include "sag_gather_row.h"
#include "stream_protocol.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int SB_REC = 8;                 // int32 words of a record: n, nnz, first row, first entry, index, 0, 0, 0
constexpr int SB_MAX_DEPTH = 7;

struct SagBatchGatherArgs {
  const int32_t* rec; int64_t n_graphs;
  const int32_t* labels;                  // [n_graphs]
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  int B; float ratio; int depth; int ldg;
  int32_t level_cap[SB_MAX_DEPTH + 1];
  int32_t *gp, *ids_out; int64_t* label_out;
  SagRowIo io;
};

__global__ __launch_bounds__(256) void sag_batch_gather_kernel(SagBatchGatherArgs a) {
  __shared__ int4 off_s[STREAM_MAX_B];    // first row, first entry, id, 0
  __shared__ int pre_n[STREAM_MAX_B + 1], pre_e[STREAM_MAX_B + 1];      // exclusive prefix sums of n / nnz over the entry's graphs
  __shared__ int wtot_s[2][2];            // wave totals of n / nnz
  __shared__ int lvl_tot_s[SB_MAX_DEPTH + 1][2];                 // workgroup 0: wave totals of k^l(n)
  __shared__ int gp_s[SB_MAX_DEPTH + 1][STREAM_MAX_B + 4];       // workgroup 0: the graph pointers, before they go out 16 bytes a store
  __shared__ long long cur_s;
  const SagRowIo& io = a.io;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int n_i = 0, e_i = 0;
  if (tid < a.B) {
    long long cur;
    const int64_t id = stream_entry_id(a.state, a.sched, a.sched_cap, a.n_graphs, a.B, tid, cur);
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + id * SB_REC);
    n_i = r0.x; e_i = r0.y;
    off_s[tid] = make_int4(r0.z, r0.w, (int)id, 0);
    if (tid == 0) cur_s = cur;
    if (blockIdx.x == 0) {                                  // the batch's own small arrays: one writer per word
      a.ids_out[tid] = (int32_t)id;
      a.label_out[tid] = (int64_t)a.labels[id];
    }
  }
  two_wave_prefix(n_i, e_i, tid, wtot_s, pre_n, pre_e);

  const int n_tot = pre_n[a.B], e_tot = pre_e[a.B];
  // (an entry that fits never reaches the clamps; one that does not — refused by the host's load — leaves pointers inside col)
  const int e_end = (int)((int64_t)e_tot < io.nnz_cap ? (int64_t)e_tot : io.nnz_cap);
  if (blockIdx.x == 0) {                                    // (uniform over the workgroup: the barriers below are met by every thread)
    // level l's graph pointer: thread b holds k^l(n_b) (threads past B: 0, so their words repeat the total), an LDS scan per level
    int s = n_i;
    for (int l = 0; l <= a.depth; ++l) {
      int sc = 0;
      if (tid < STREAM_MAX_B) {
        sc = wave_scan_inclusive(s, lane);
        if (lane == 63) lvl_tot_s[l][wave] = sc;
      }
      __syncthreads();
      if (tid < STREAM_MAX_B) {
        const int p = sc + (wave ? lvl_tot_s[l][0] : 0);
        gp_s[l][tid + 1] = p < a.level_cap[l] ? p : a.level_cap[l];
      }
      if (tid == 0) gp_s[l][0] = 0;
      const int kk = (int)ceilf(a.ratio * (float)s);        // float32, as PyG's topk and SagPlan compute it
      s = kk < s ? kk : s;
    }
    __syncthreads();
    const int q4 = a.ldg >> 2;
    for (int i = tid; i < (a.depth + 1) * q4; i += 256) {
      const int l = i / q4, j = 4 * (i - l * q4);
      const int* g = gp_s[l];                               // (B <= 128: word 128 is the total whatever B)
      constexpr int M = STREAM_MAX_B;
      const int j1 = j + 1 < M ? j + 1 : M, j2 = j + 2 < M ? j + 2 : M, j3 = j + 3 < M ? j + 3 : M;
      *reinterpret_cast<int4*>(a.gp + (int64_t)l * a.ldg + j) = make_int4(g[j < M ? j : M], g[j1], g[j2], g[j3]);
    }
    if (tid == 64) io.rowptr_out[io.row_cap] = e_end;
  }

  SagRow w;
  w.r = (int64_t)blockIdx.x * SAG_ROWS + (tid >> 3);
  w.sub = tid & (SAG_EG - 1);
  w.lane = lane;
  // the graph whose rows hold r: the last k with pre_n[k] <= r (every graph has a row, so the prefix is strictly increasing); a trip
  // count that depends on B alone
  int lo = 0, hi = a.B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)pre_n[mid] <= w.r) lo = mid; else hi = mid;
  }
  w.real = w.r < (int64_t)n_tot && w.r < io.row_cap;
  w.g0 = pre_n[lo]; w.eb = pre_e[lo];
  const int4 o4 = off_s[lo];
  w.row0 = o4.x; w.ent0 = o4.y; w.gid = o4.z;
  w.e_tot = e_tot; w.e_end = e_end;
  sag_gather_row(io, w);
  // This workgroup READ the cursor before its first barrier (the value went through LDS), so thread 0 may draw the workgroup's ticket;
  // here, behind its stores, so that no wave waits for the atomic's round trip in front of its work.  A DD-shaped batch of 128 graphs
  // has more than 1,400 workgroups: the sharded ticket.
  if (tid == 0) stream_ticket_sharded(a.ticket, a.state, cur_s);
}

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_sag_batch_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t off_rowptr, int64_t off_col,
                               int64_t arena_words, const float* feats, int64_t ldf, const int32_t* labels, int64_t max_n,
                               int64_t max_nnz, const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket, int B,
                               int64_t row_cap, int64_t nnz_cap, const int64_t* level_caps, float ratio, int depth, int32_t* rowptr,
                               int32_t* col, float* x, int64_t ldx, float* dinv, float* self_w, int32_t* graph_ptr, int64_t ldg,
                               int32_t* ids_out, int64_t* label_out, tsgnn_stream_t stream) {
  if (!records || !arena || !feats || !labels || !sched || !state || !ticket || !level_caps || !rowptr || !col || !x || !dinv || !self_w ||
      !graph_ptr || !ids_out || !label_out)
    return TSGNN_EINVAL;
  if (B < 1 || B > STREAM_MAX_B || sched_cap <= 0 || n_graphs <= 0 || row_cap <= 0 || nnz_cap < 1 || ldf <= 0 || max_n < 1 || max_nnz < 0 ||
      depth < 1 || depth > SB_MAX_DEPTH || !(ratio > 0.f) || !(ratio <= 1.f))
    return TSGNN_EINVAL;
  if (ldg < B + 1 || (ldg % 4)) return TSGNN_EINVAL;
  if (off_rowptr < 0 || off_col < off_rowptr || arena_words < off_col) return TSGNN_EINVAL;
  if (max_n >= ((int64_t)1 << 31) / B || max_nnz >= ((int64_t)1 << 31) / B || row_cap >= ((int64_t)1 << 31) - SAG_ROWS ||
      nnz_cap >= ((int64_t)1 << 31) || sched_cap >= ((int64_t)1 << 31) / B || ldg >= ((int64_t)1 << 31) / (SB_MAX_DEPTH + 1))
    return TSGNN_EUNSUPPORTED;
  // every graph of the arena fits the slot on its own at every level (max_n and max_nnz are the caller's word, as the arena is).
  // Whether an ENTRY fits is the uploader's check (sag_stream.MiniBatchStream.load): the kernel clamps, so an entry that does not fit
  // cannot write outside the arrays.
  if (row_cap < max_n || nnz_cap < max_nnz || level_caps[0] != row_cap) return TSGNN_EINVAL;
  SagBatchGatherArgs a{};
  {
    int s = (int)max_n;
    for (int l = 0; l <= depth; ++l) {
      if (level_caps[l] < s) return TSGNN_EINVAL;
      if (level_caps[l] >= ((int64_t)1 << 31)) return TSGNN_EUNSUPPORTED;
      a.level_cap[l] = (int32_t)level_caps[l];
      const int kk = (int)ceilf(ratio * (float)s);
      s = kk < s ? kk : s;
    }
  }
  if ((ldf % 4) || ldx != ldf || ((off_rowptr | off_col) & 3)) return TSGNN_EUNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(feats) |
                       reinterpret_cast<uintptr_t>(rowptr) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dinv) |
                       reinterpret_cast<uintptr_t>(self_w) | reinterpret_cast<uintptr_t>(graph_ptr) | reinterpret_cast<uintptr_t>(state);
  if ((al & 15) || (reinterpret_cast<uintptr_t>(label_out) & 7)) return TSGNN_EUNSUPPORTED;
  a.rec = records; a.n_graphs = n_graphs; a.labels = labels;
  a.sched = sched; a.sched_cap = sched_cap; a.state = state; a.ticket = ticket;
  a.B = B; a.ratio = ratio; a.depth = depth; a.ldg = (int)ldg;
  a.gp = graph_ptr; a.ids_out = ids_out; a.label_out = label_out;
  a.io = SagRowIo{arena + off_rowptr, arena + off_col, feats, ldf, (int)(ldf / 4), row_cap, nnz_cap, rowptr, col, x, ldx, dinv, self_w};
  TSGNN_KNAME("sag_batch_gather_kernel");
  sag_batch_gather_kernel<<<(unsigned)ceil_div64(row_cap, SAG_ROWS), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
