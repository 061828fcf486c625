// SAGPool triplet stream: a NEW triplet every replay of one hipGraph (Code/sag/train_triplet.py:198-214: tripletsampler_tr.sampler() ->
// TNet(a, p, n) -> margin loss -> Adam, once per optimiser step).  csrc/triplet_stream.hip does this for the GraphSage family; this
// is the launch for sag_layers.Net.  The dataset lives on the device whole (the arena of sag_stream.pack_arena: per-graph records, one
// int32 buffer of graph-local CSR rows, one feature table), the sampler's epoch is an index array [T, 3] behind {cursor, T}, and ONE
// launch per step reads "entry number cursor" and writes what sag_stack's node reads of a batch, padded to capacities that do not
// depend on the triplet:
//   rowptr [row_cap + 1]     rows at or past n_tot are empty: every entry from n_tot on is the batch's nnz
//   col [: nnz]              node ids offset by the graphs before
//   x [row_cap][ldx]         feature rows, zero on padding rows
//   dinv / self_w [row_cap]  tsgnn_gcn_coef_f32's values on the batch rows (gcn_norm_coef, common.h), 0 / 0 on padding rows
//   gp [depth + 1][4]        the graph pointer of EVERY level: k_b = min(n_b, ceil(float32(ratio) * float32(n_b))) level after level,
//                            what sag_stack.SagPlan computes on the host with np.float32
//   ids_out [3]
// Cursor and ticket counter: the protocol of csrc/stream_protocol.h, on the same [HEAD | schedule] buffer.
// The number of graphs a schedule entry names is a template parameter of the body: 3 is the triplet launch above, 1 the ANCHOR launch of
// the 2stg+ post-training step (Code/sag/train_triplet_pre_train.py:219-263: one optimiser step per graph at B = 1) — a schedule
// [T, 1], capacities of ONE largest graph, gp rows (0, k_l, k_l, k_l) (still one 16-byte store: words 2 and 3 repeat the total),
// ids_out [1].
// The rows themselves: csrc/sag_gather_row.h (one writer per word, plain vector stores; a level's graph pointer is a 16-byte store
// too); the ticket counter is the only atomic.
#include "sag_gather_row.h"
#include "stream_protocol.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int SS_B = 3;                   // a triplet
constexpr int SS_ANCHOR = 1;              // the anchor alone
constexpr int SS_REC = 8;                 // int32 words of a record: n, nnz, first row, first entry, index, 0, 0, 0
constexpr int SS_MAX_DEPTH = 7;

struct SagGatherArgs {
  const int32_t* rec; int64_t n_graphs;
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  float ratio; int depth;
  int32_t *gp, *ids_out;
  SagRowIo io;
};

template <int NB>
__device__ __forceinline__ void sag_gather_body(const SagGatherArgs& a) {
  __shared__ int32_t rec_s[NB][SS_REC];
  __shared__ long long cur_s;
  const SagRowIo& io = a.io;
  const int tid = threadIdx.x;
  if (tid < NB) {
    long long cur;
    const int64_t id = stream_entry_id(a.state, a.sched, a.sched_cap, a.n_graphs, NB, tid, cur);
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + id * SS_REC);
    rec_s[tid][0] = r0.x; rec_s[tid][1] = r0.y; rec_s[tid][2] = r0.z; rec_s[tid][3] = r0.w;
    rec_s[tid][4] = (int32_t)id;
    if (tid == 0) cur_s = cur;
  }
  __syncthreads();
  // Every workgroup has READ the cursor by now (its value went through LDS), so it may draw its ticket
  if (tid == 0) stream_ticket_flat(a.ticket, gridDim.x, a.state, cur_s);

  SagRow w;
  w.r = (int64_t)blockIdx.x * SAG_ROWS + (tid >> 3);
  w.sub = tid & (SAG_EG - 1);
  w.lane = tid & 63;
  // the graph whose rows hold r, and the batch's totals: one pass over the three records, no data-dependent branch
  int n_tot = 0, e_tot = 0;
  int b = NB;
  w.g0 = w.eb = w.row0 = w.ent0 = w.gid = 0;
  for (int k = 0; k < NB; ++k) {
    const int nk = rec_s[k][0], ek = rec_s[k][1];
    const bool mine = w.r >= n_tot && w.r < (int64_t)n_tot + nk;
    b = mine ? k : b;
    w.g0 = mine ? n_tot : w.g0;
    w.eb = mine ? e_tot : w.eb;
    w.row0 = mine ? rec_s[k][2] : w.row0;
    w.ent0 = mine ? rec_s[k][3] : w.ent0;
    w.gid = mine ? rec_s[k][4] : w.gid;
    n_tot += nk;
    e_tot += ek;
  }
  if (blockIdx.x == 0) {                                    // the batch's own small arrays: one writer per word
    if (tid <= a.depth) {                                   // level tid: the k chain applied tid times, then the prefix
      int s[NB];
      for (int k = 0; k < NB; ++k) s[k] = rec_s[k][0];
      for (int l = 0; l < tid; ++l)
        for (int k = 0; k < NB; ++k) {
          const int kk = (int)ceilf(a.ratio * (float)s[k]);       // float32, as PyG's topk and SagPlan compute it
          s[k] = kk < s[k] ? kk : s[k];
        }
      int p[4] = {0, 0, 0, 0};                              // the prefix; past NB graphs the words repeat the total
      for (int k = 0; k < 3; ++k) p[k + 1] = p[k] + (k < NB ? s[k] : 0);
      *reinterpret_cast<int4*>(a.gp + 4 * tid) = make_int4(p[0], p[1], p[2], p[3]);
    }
    if (tid >= 32 && tid < 32 + NB) a.ids_out[tid - 32] = rec_s[tid - 32][4];
    if (tid == 64) io.rowptr_out[io.row_cap] = e_tot;
  }
  w.real = b < NB && w.r < io.row_cap;
  w.e_tot = e_tot;
  w.e_end = (int)((int64_t)e_tot < io.nnz_cap ? (int64_t)e_tot : io.nnz_cap);     // (= e_tot: the entry point's need_nnz check)
  sag_gather_row(io, w);
}

__global__ __launch_bounds__(256) void sag_triplet_gather_kernel(SagGatherArgs a) { sag_gather_body<SS_B>(a); }
__global__ __launch_bounds__(256) void sag_anchor_gather_kernel(SagGatherArgs a) { sag_gather_body<SS_ANCHOR>(a); }

template <int NB>
int sag_gather_launch(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t off_rowptr, int64_t off_col,
                      int64_t arena_words, const float* feats, int64_t ldf, int64_t need_rows, int64_t need_nnz,
                      const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket, int64_t row_cap,
                      int64_t nnz_cap, float ratio, int depth, int32_t* rowptr, int32_t* col, float* x, int64_t ldx,
                      float* dinv, float* self_w, int32_t* graph_ptr, int32_t* ids_out, tsgnn_stream_t stream) {
  if (!records || !arena || !feats || !sched || !state || !ticket || !rowptr || !col || !x || !dinv || !self_w || !graph_ptr || !ids_out)
    return TSGNN_EINVAL;
  if (sched_cap <= 0 || n_graphs <= 0 || row_cap <= 0 || nnz_cap < 1 || ldf <= 0 || need_rows < 0 || need_nnz < 0 || depth < 1 ||
      depth > SS_MAX_DEPTH || !(ratio > 0.f) || !(ratio <= 1.f))
    return TSGNN_EINVAL;
  // no schedule entry can overflow a slot: the capacities cover the arena's bounds (NB times its largest n / nnz).  need_rows and
  // need_nnz are the caller's word, as the arena is (see tsgnn_triplet_gather_f32)
  if (row_cap < need_rows || nnz_cap < need_nnz) return TSGNN_EINVAL;
  if (off_rowptr < 0 || off_col < off_rowptr || arena_words < off_col) return TSGNN_EINVAL;
  if (row_cap >= ((int64_t)1 << 31) - SAG_ROWS || nnz_cap >= ((int64_t)1 << 31) || sched_cap >= ((int64_t)1 << 31) / NB)
    return TSGNN_EUNSUPPORTED;
  if ((ldf % 4) || ldx != ldf || ((off_rowptr | off_col) & 3)) return TSGNN_EUNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(feats) |
                       reinterpret_cast<uintptr_t>(rowptr) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dinv) |
                       reinterpret_cast<uintptr_t>(self_w) | reinterpret_cast<uintptr_t>(graph_ptr) | reinterpret_cast<uintptr_t>(state);
  if (al & 15) return TSGNN_EUNSUPPORTED;
  SagGatherArgs a{records, n_graphs, sched, sched_cap, state, ticket, ratio, depth, graph_ptr, ids_out,
                  {arena + off_rowptr, arena + off_col, feats, ldf, (int)(ldf / 4), row_cap, nnz_cap, rowptr, col, x, ldx, dinv, self_w}};
  if (NB == SS_B) {
    TSGNN_KNAME("sag_triplet_gather_kernel");
    sag_triplet_gather_kernel<<<(unsigned)ceil_div64(row_cap, SAG_ROWS), 256, 0, stream>>>(a);
  } else {
    TSGNN_KNAME("sag_anchor_gather_kernel");
    sag_anchor_gather_kernel<<<(unsigned)ceil_div64(row_cap, SAG_ROWS), 256, 0, stream>>>(a);
  }
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_sag_triplet_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t off_rowptr, int64_t off_col,
                                 int64_t arena_words, const float* feats, int64_t ldf, int64_t need_rows, int64_t need_nnz,
                                 const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket, int64_t row_cap,
                                 int64_t nnz_cap, float ratio, int depth, int32_t* rowptr, int32_t* col, float* x, int64_t ldx,
                                 float* dinv, float* self_w, int32_t* graph_ptr, int32_t* ids_out, tsgnn_stream_t stream) {
  return sag_gather_launch<SS_B>(records, n_graphs, arena, off_rowptr, off_col, arena_words, feats, ldf, need_rows, need_nnz, sched, sched_cap,
                                 state, ticket, row_cap, nnz_cap, ratio, depth, rowptr, col, x, ldx, dinv, self_w, graph_ptr, ids_out, stream);
}

int tsgnn_sag_anchor_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t off_rowptr, int64_t off_col,
                                int64_t arena_words, const float* feats, int64_t ldf, int64_t need_rows, int64_t need_nnz,
                                const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket, int64_t row_cap,
                                int64_t nnz_cap, float ratio, int depth, int32_t* rowptr, int32_t* col, float* x, int64_t ldx,
                                float* dinv, float* self_w, int32_t* graph_ptr, int32_t* ids_out, tsgnn_stream_t stream) {
  return sag_gather_launch<SS_ANCHOR>(records, n_graphs, arena, off_rowptr, off_col, arena_words, feats, ldf, need_rows, need_nnz, sched,
                                      sched_cap, state, ticket, row_cap, nnz_cap, ratio, depth, rowptr, col, x, ldx, dinv, self_w, graph_ptr,
                                      ids_out, stream);
}

}  // extern "C"
