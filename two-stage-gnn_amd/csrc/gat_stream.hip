// GAT triplet stream: a NEW triplet every replay of one hipGraph (Code/sage+gat+diffpool/train_triplet.py:247-287 with --method=GAT:
// tripletsampler_tr.sampler() -> TNet(a, p, n) -> margin loss -> clip -> Adam, once per optimiser step).  csrc/triplet_stream.hip does
// this for the GraphSage family and csrc/sag_stream.hip for SAGPool; this is the launch for gat_triplet.tripletnet.  The dataset lives
// on the device whole (the arena of gat_stream.pack_arena: every graph's piece buffer, the one gat_assemble.hip reads, behind a table
// of records), the sampler's epoch is an index array [T, 3] behind {cursor, T}, and ONE launch per step reads "entry number cursor"
// and writes every array the fused GAT launches read of a batch — gat_assemble_kernel with the three pieces found on the device
// instead of in a host description (gat_assemble_body.h holds what the two share) — at capacities that do not depend on the triplet.
//
// Behind the triplet's own R rows / E entries / I listed edge-less columns everything up to capacity is inert:
//   rowptr, rowptr_t (R .. row_cap]   = E: padding rows are empty both ways
//   x [R .. row_cap)                  +0;  row_mult 0;  the indicator rows iso_cols_v 0
//   row_graph [R .. row_cap)          = 2, the last graph (in bounds for iso_ptr[row_graph[r] + 1] of the forward and for the readout's
//                                     winners [3, C] of the backward; a padding row has no entry either way, so nothing of a real row,
//                                     of dW' or of dx depends on what it computes), row_slot 0
//   graph_ptr[3] = R, iso_ptr[3] = I  the readout and the per-graph workgroups end at the last real row
//   col, col_t, src_e_t, inv past E and the list past I are not written: every reader reaches them through the pointers above.
// Grid: x = the chunk count of the largest piece (summed over its arrays), y = the three pieces + one row of workgroups that strides
// over the padding.  Cursor and ticket counter: the protocol of csrc/stream_protocol.h, on the same [HEAD | schedule] buffer.
// One writer per word, plain vector stores (16 bytes wherever the destination sits on 16 bytes: ga_copy_add, the padding feature
// rows), the ticket counter is the only atomic.
//
// The number of pieces a schedule entry names is a template parameter of the body: 3 is the triplet launch above, 1 the ANCHOR launch of
// the 2stg+ post-training step (train_triplet_pre_train.py:233-262: one Adam step per anchor graph at B = 1; gat_stream.PostTrainStream).
// With one piece the schedule entries are one word, the grid is (chunks of the largest piece, 1 + 1), padding rows get row_graph 0,
// graph_ptr[1] = R, iso_ptr[1] = I and ids_out[0] is the anchor's index.
#include "gat_assemble_body.h"
#include "stream_protocol.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int GS_B = 3;                   // a triplet
constexpr int GS_ANCHOR = 1;              // the anchor of a post-training step
constexpr int GS_REC = 8;                 // int32 words of a record: piece offset (words), n, nr, nnz, k, Nmax - n, index, 0

struct GsArgs {
  const int32_t* rec; int64_t n_graphs; const int32_t* arena;
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  int64_t row_cap, nnz_cap, iso_cap; int32_t* ids_out;
  GA_OUTPUT_FIELDS
};

template <int NB>
__device__ __forceinline__ void gs_gather_body(const GsArgs& a) {
  __shared__ int32_t rec_s[NB][GS_REC];
  __shared__ long long cur_s;
  const int tid = threadIdx.x;
  if (tid < NB) {
    long long cur;
    const int64_t id = stream_entry_id(a.state, a.sched, a.sched_cap, a.n_graphs, NB, tid, cur);
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + id * GS_REC);
    const int4 r1 = *reinterpret_cast<const int4*>(a.rec + id * GS_REC + 4);
    rec_s[tid][0] = r0.x; rec_s[tid][1] = r0.y; rec_s[tid][2] = r0.z; rec_s[tid][3] = r0.w;
    rec_s[tid][4] = r1.x; rec_s[tid][5] = r1.y; rec_s[tid][6] = (int32_t)id; rec_s[tid][7] = 0;
    if (tid == 0) cur_s = cur;
  }
  __syncthreads();
  // Every workgroup has READ the cursor by now (its value went through LDS), so it may draw its ticket
  if (tid == 0) stream_ticket_flat(a.ticket, gridDim.x * gridDim.y, a.state, cur_s);
  // where each piece goes, and the batch's totals
  int row0[NB + 1], e0[NB + 1], i0[NB + 1];
  row0[0] = e0[0] = i0[0] = 0;
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    row0[k + 1] = row0[k] + rec_s[k][2];
    e0[k + 1] = e0[k] + rec_s[k][3];
    i0[k + 1] = i0[k] + rec_s[k][4];
  }
  const int64_t R = row0[NB], E = e0[NB], I = i0[NB];
  // (the entry point checked the capacities against the arena's bounds; records that break them write nothing)
  if (R > a.row_cap || E > a.nnz_cap || I > a.iso_cap) return;

  if (blockIdx.y < NB) {
    const int y = blockIdx.y;
    GaPiece q;
    q.src = a.arena + rec_s[y][0];
    q.n = rec_s[y][1]; q.nr = rec_s[y][2]; q.nnz = rec_s[y][3]; q.k = rec_s[y][4]; q.mult = rec_s[y][5];
    q.row0 = q.e0 = q.i0 = 0;
#pragma unroll
    for (int k = 1; k < NB; ++k)                // (selects, not an indexed read: the prefix arrays stay in registers)
      if (y == k) { q.row0 = row0[k]; q.e0 = e0[k]; q.i0 = i0[k]; }
    q.gidx = y; q.last = y == NB - 1;
    int64_t b = blockIdx.x;
    const int kind = ga_kind_of(q, a.ldf, b);
    if (kind == GA_KINDS) return;               // (the grid is sized for the largest piece of the dataset)
    ga_piece_chunk(a, q, kind, b);
    if (kind == GA_LIST && b == 0 && tid == 64) a.ids_out[y] = rec_s[y][6];
    return;
  }

  // the padding: this row of workgroups strides over [R, capacity) of every per-row array
  const int64_t i = (int64_t)blockIdx.x * 256 + tid, S = (int64_t)gridDim.x * 256;
  const int Ei = (int)E;
  for (int64_t r = R + 1 + i; r <= a.row_cap; r += S) {
    a.rowptr[r] = Ei;
    a.rowptr_t[r] = Ei;
  }
  for (int64_t r = R + i; r < a.row_cap; r += S) {
    a.row_mult[r] = 0.f;
    a.row_graph[r] = NB - 1;
    a.row_slot[r] = 0;
  }
  for (int v = 0; v < a.nH; ++v) {
    const int64_t w1 = a.row_cap * a.H[v];
    for (int64_t w = R * a.H[v] + i; w < w1; w += S) a.iso_cols[v][w] = 0.f;
  }
  {
    const int64_t ld4 = a.ldf / 4;                          // (rows of ldf = 4 m floats on a 16-byte base)
    float4* x4 = reinterpret_cast<float4*>(a.x);
    for (int64_t w = R * ld4 + i; w < a.row_cap * ld4; w += S) x4[w] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__global__ __launch_bounds__(256) void gat_triplet_gather_kernel(GsArgs a) { gs_gather_body<GS_B>(a); }
__global__ __launch_bounds__(256) void gat_anchor_gather_kernel(GsArgs a) { gs_gather_body<GS_ANCHOR>(a); }

// what the two entry points share: the checks, the description and the launch for NB pieces per schedule entry
template <int NB>
int gs_launch(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t arena_words, int64_t max_nr, int64_t max_nnz,
              int64_t max_k, const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket, const int64_t* desc,
              int32_t* ids_out, hipStream_t stream) {
  if (!records || !arena || !sched || !state || !ticket || !desc || !ids_out) return TSGNN_EINVAL;
  if (n_graphs <= 0 || sched_cap <= 0 || arena_words <= 0 || max_nr < 1 || max_nnz < 0 || max_k < 0 || max_k > max_nr) return TSGNN_EINVAL;
  GsArgs a{};
  int64_t R, E, I, B;
  if (!ga_unpack_header(desc, a, R, E, I, B) || B != NB) return TSGNN_EINVAL;
  // no schedule entry can overflow an array: the capacities cover NB times the arena's largest piece, also when one object fills
  // all of a triplet's three places.  max_nr / max_nnz / max_k are the caller's word, as the arena is (see tsgnn_triplet_gather_f32)
  if (R < NB * max_nr || E < NB * max_nnz || I < NB * max_k) return TSGNN_EINVAL;
  if (arena_words >= ((int64_t)1 << 31) || sched_cap >= ((int64_t)1 << 31) / NB || R * a.ldf >= ((int64_t)1 << 31)) return TSGNN_EUNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(state);
  if (al & 15) return TSGNN_EUNSUPPORTED;
  a.rec = records; a.n_graphs = n_graphs; a.arena = arena; a.sched = sched; a.sched_cap = sched_cap; a.state = state; a.ticket = ticket;
  a.row_cap = R; a.nnz_cap = E; a.iso_cap = I; a.ids_out = ids_out;
  GaPiece top{};                                           // the largest piece per kind, closing entries included
  top.nr = (int)max_nr; top.nnz = (int)max_nnz; top.k = (int)max_k; top.last = 1;
  int64_t most = 0;
  for (int kind = 0; kind < GA_KINDS; ++kind) most += ga_chunks(top, kind, a.ldf);
  if (most >= 65536) return TSGNN_EUNSUPPORTED;
  if (NB == GS_B) {
    TSGNN_KNAME("gat_triplet_gather_kernel");
    gat_triplet_gather_kernel<<<dim3((unsigned)most, NB + 1), 256, 0, stream>>>(a);
  } else {
    TSGNN_KNAME("gat_anchor_gather_kernel");
    gat_anchor_gather_kernel<<<dim3((unsigned)most, NB + 1), 256, 0, stream>>>(a);
  }
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_gat_triplet_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t arena_words, int64_t max_nr,
                                 int64_t max_nnz, int64_t max_k, const int32_t* sched, int64_t sched_cap, int64_t* state,
                                 unsigned* ticket, const int64_t* desc, int32_t* ids_out, tsgnn_stream_t stream) {
  return gs_launch<GS_B>(records, n_graphs, arena, arena_words, max_nr, max_nnz, max_k, sched, sched_cap, state, ticket, desc, ids_out, stream);
}

/* see include/tsgnn.h */
int tsgnn_gat_anchor_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t arena_words, int64_t max_nr,
                                int64_t max_nnz, int64_t max_k, const int32_t* sched, int64_t sched_cap, int64_t* state,
                                unsigned* ticket, const int64_t* desc, int32_t* ids_out, tsgnn_stream_t stream) {
  return gs_launch<GS_ANCHOR>(records, n_graphs, arena, arena_words, max_nr, max_nnz, max_k, sched, sched_cap, state, ticket, desc, ids_out,
                              stream);
}

}  // extern "C"
