// EigenGCN triplet stream: a NEW triplet every replay of one hipGraph (Code/eigengcn/train_triplet.py:289-317: tripletsampler_tr.sampler()
// -> TNet(a, p, n) -> margin loss -> clip -> Adam, once per optimiser step).  csrc/triplet_stream.hip does this for the GraphSage family,
// csrc/sag_stream.hip for SAGPool and csrc/gat_stream.hip for GAT; this is the launch for eigen_triplet.tripletnet.  The dataset lives
// on the device whole (the arena of eigen_stream.pack_arena: every graph's piece buffer, the one eigen_assemble.hip reads, behind a
// table of records), the sampler's epoch is an index array [T, 3] behind {cursor, T}, and ONE launch per step reads "entry number
// cursor" and writes every array of the three-graph EigenBatch — eigen_assemble_kernel with the three pieces found on the device
// instead of in a host description (eigen_assemble_body.h holds what the two share) — at capacities that do not depend on the triplet.
//
// With R_i rows and E_i entries of the triplet's own at level graph i, row_cap_i / nnz_cap_i the capacities, everything behind the
// triplet's own is inert:
//   rowptr_i (R_i .. row_cap_i + Nmax]   = E_i: padding rows and the Nmax ghost-slot rows (which sit behind the row CAPACITY) are empty
//   graph_ptr_i[3]                       = R_i: per-graph workgroups and readouts end at the last real row
//   row_graph_i [R_i .. row_cap_i)       = 2, the last graph (in bounds wherever a row-local kernel looks its graph up), row_slot_i 0
//   cluster_of_i [R_i .. row_cap_i)      = -1: a padding row belongs to no cluster
//   coef_i, final_coef padding rows      +0: eigen_pool_bwd<final> reads coef[r] of every row below n_rows0
//   x [R_0 .. row_cap_0 + Nmax)          +0: padding rows and ghost rows
//   slot_count_i[s]                      = the number of the three pieces with n_i > s
//   bptr_i from the closing entry on     = R_i (index R_{i+1} + 3 .. row_cap_{i+1} + 3): empty buckets
//   col_i, val_i past E_i and members_i past R_i are NOT written: every reader reaches them through rowptr_i / bptr_i.
// Grid: x = the chunk count of the dataset's largest piece (summed over its arrays), y = the three pieces + one row of workgroups
// that strides over the closing entries, the padding and the slot counts.  Cursor and ticket counter: the protocol of
// csrc/stream_protocol.h, on the same [HEAD | schedule] buffer.  One writer per word, plain vector stores (16 bytes wherever the
// destination sits on 16 bytes: ea_copy, es_fill), the ticket counter is the only atomic.
//
// The number of pieces a schedule entry names is a template parameter of the body: 3 is the triplet launch above, 1 the ANCHOR launch of
// the 2stg+ post-training step (Code/eigengcn/train_triplet_pre_train.py:192-247: one optimiser step on the sampler's anchor at
// B = 1) — a schedule [T, 1], a header with B = 1, capacities of ONE largest piece per level, grid (most, 1 + 1), padding row_graph 0,
// graph_ptr_i[1] = the anchor's rows, bucket pointers sized for one graph, ids_out [1]; everything behind the anchor's own R_i / E_i
// inert as above.
#include "eigen_assemble_body.h"
#include "stream_protocol.h"

namespace {

constexpr int ES_B = 3;                   // a triplet
constexpr int ES_ANCHOR = 1;              // the anchor alone
constexpr int ES_REC = 12;                // int32 words of a record: piece offset (words), index, n[0..3], nnz[0..3], 0, 0

struct EsArgs {
  const int32_t* rec; int64_t n_graphs; const int32_t* arena; int64_t arena_words;
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  int32_t* ids_out;
  EaHead h;                               // R[i], E[i]: the CAPACITIES the arrays are allocated for
};

// dst[lo, hi) = value by the threads i, i + S, ...; dst sits on 16 bytes
__device__ __forceinline__ void es_fill(int* __restrict__ dst, int64_t lo, int64_t hi, int value, int64_t i, int64_t S) {
  if (hi <= lo) return;
  const int64_t v0 = min((lo + 3) & ~(int64_t)3, hi);
  const int64_t v1 = max(hi & ~(int64_t)3, v0);
  if (i < v0 - lo) dst[lo + i] = value;
  if (i < hi - v1) dst[v1 + i] = value;
  const ea_i4 o = {value, value, value, value};
  for (int64_t w = (v0 >> 2) + i; w < (v1 >> 2); w += S) reinterpret_cast<ea_i4*>(dst)[w] = o;
}

template <int NB>
__device__ __forceinline__ void es_gather_body(const EsArgs& a) {
  __shared__ int32_t rec_s[NB][ES_REC];
  __shared__ long long cur_s;
  __shared__ EaPiece q_s;                     // this workgroup's piece (LDS: ea_piece_block indexes its levels at run time)
  const int tid = threadIdx.x;
  if (tid < NB) {
    long long cur;
    const int64_t id = stream_entry_id(a.state, a.sched, a.sched_cap, a.n_graphs, NB, tid, cur);
    const int4* r = reinterpret_cast<const int4*>(a.rec + id * ES_REC);
    const int4 r0 = r[0], r1 = r[1], r2 = r[2];
    int32_t* o = rec_s[tid];
    o[0] = r0.x; o[1] = (int32_t)id; o[2] = r0.z; o[3] = r0.w;
    o[4] = r1.x; o[5] = r1.y; o[6] = r1.z; o[7] = r1.w; o[8] = r2.x; o[9] = r2.y; o[10] = 0; o[11] = 0;
    if (tid == 0) cur_s = cur;
  }
  __syncthreads();
  // Every workgroup has READ the cursor by now (its value went through LDS), so it may draw its ticket
  if (tid == 0) stream_ticket_flat(a.ticket, gridDim.x * gridDim.y, a.state, cur_s);
  const EaHead& h = a.h;
  const int nlev = h.nlev, L = nlev - 1;
  // where each piece goes, and the triplet's totals.  (The entry point checked the capacities against the arena's bounds; records
  // that break them, or that leave the arena, write nothing.)
  int R[EA_LMAX], E[EA_LMAX];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < EA_LMAX; ++i) {
    R[i] = E[i] = 0;
    if (i < nlev) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const int n = rec_s[k][2 + i], z = rec_s[k][2 + EA_LMAX + i];
        ok = ok && n >= 0 && n <= h.nmax && z >= 0 && R[i] <= h.R[i] - n && E[i] <= h.E[i] - z;
        R[i] += n; E[i] += z;
      }
    }
  }
  if (!ok) return;

  if (blockIdx.y < NB) {
    const int y = blockIdx.y;
    EaPiece& q = q_s;
    if (tid == 0) {
      q.gidx = y; q.last = 0;                   // (the closing entries and the ghost rows are the padding workgroups')
      for (int i = 0; i < EA_LMAX; ++i) {
        q.n[i] = i < nlev ? rec_s[y][2 + i] : 0;
        q.nnz[i] = i < nlev ? rec_s[y][2 + EA_LMAX + i] : 0;
        q.row0[i] = q.e0[i] = 0;
        for (int k = 0; k < y; ++k) {
          q.row0[i] += i < nlev ? rec_s[k][2 + i] : 0;
          q.e0[i] += i < nlev ? rec_s[k][2 + EA_LMAX + i] : 0;
        }
      }
      q.src = a.arena + rec_s[y][0];
    }
    __syncthreads();
    const int64_t off = rec_s[y][0];
    if (off < 0 || (off & 3) || off + ea_section(q.n, q.nnz, nlev, h.J, h.Jf, h.ldf, 7 * nlev - 2) > a.arena_words) return;
    ea_piece_block(h, q);
    return;
  }

  // the closing entries, the padding and the slot counts: this row of workgroups strides over them
  const int64_t i = (int64_t)blockIdx.x * 256 + tid, S = (int64_t)gridDim.x * 256;
  if (i < NB) a.ids_out[i] = rec_s[i][1];
#pragma unroll
  for (int v = 0; v < EA_LMAX; ++v) {
    if (v >= nlev) continue;
    es_fill(h.rowptr[v], R[v], (int64_t)h.R[v] + h.nmax + 1, E[v], i, S);
    es_fill(h.row_graph[v], R[v], h.R[v], NB - 1, i, S);
    es_fill(h.row_slot[v], R[v], h.R[v], 0, i, S);
    if (i == 0) h.graph_ptr[v][NB] = R[v];
    for (int64_t s = i; s < h.nmax; s += S) {
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < NB; ++k) cnt += rec_s[k][2 + v] > s ? 1 : 0;
      h.slot_count[v][s] = cnt;
    }
  }
  int RL = 0;                                   // R[L] without a dynamic index into the registers
#pragma unroll
  for (int v = 0; v < EA_LMAX; ++v) RL = v == L ? R[v] : RL;
#pragma unroll
  for (int v = 0; v < EA_LMAX - 1; ++v) {
    if (v >= L) continue;
    es_fill(h.cluster_of[v], R[v], h.R[v], -1, i, S);
    es_fill(reinterpret_cast<int*>(h.coef[v]), (int64_t)R[v] * h.J, (int64_t)h.R[v] * h.J, 0, i, S);
    es_fill(h.bptr[v], (int64_t)R[v + 1] + NB, (int64_t)h.R[v + 1] + NB + 1, R[v], i, S);
  }
  if (h.Jf > 0) es_fill(reinterpret_cast<int*>(h.final_coef), (int64_t)RL * h.Jf, (int64_t)h.R[L] * h.Jf, 0, i, S);
  es_fill(reinterpret_cast<int*>(h.x), (int64_t)R[0] * h.ldf, ((int64_t)h.R[0] + h.nmax) * h.ldf, 0, i, S);
}

__global__ __launch_bounds__(256) void eigen_triplet_gather_kernel(EsArgs a) { es_gather_body<ES_B>(a); }
__global__ __launch_bounds__(256) void eigen_anchor_gather_kernel(EsArgs a) { es_gather_body<ES_ANCHOR>(a); }

template <int NB>
int es_gather_launch(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t arena_words, const int64_t* top_n,
                     const int64_t* top_nnz, const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket, const int64_t* desc,
                     int32_t* ids_out, tsgnn_stream_t stream) {
  if (!records || !arena || !top_n || !top_nnz || !sched || !state || !ticket || !desc || !ids_out) return TSGNN_EINVAL;
  if (n_graphs <= 0 || sched_cap <= 0 || arena_words <= 0) return TSGNN_EINVAL;
  EsArgs a{};
  if (!ea_unpack_header(desc, a.h) || a.h.B != NB) return TSGNN_EINVAL;
  const EaHead& h = a.h;
  // no schedule entry can overflow an array: the capacities cover NB times the arena's largest piece at every level, also when
  // one object fills every place.  top_n / top_nnz are the caller's word, as the arena is (see tsgnn_triplet_gather_f32)
  EaPiece top{};
  for (int i = 0; i < h.nlev; ++i) {
    if (top_n[i] < 1 || top_n[i] > h.nmax || top_nnz[i] < 0) return TSGNN_EINVAL;
    if (h.R[i] < NB * top_n[i] || h.E[i] < NB * top_nnz[i]) return TSGNN_EINVAL;
    top.n[i] = (int)top_n[i]; top.nnz[i] = (int)top_nnz[i];
  }
  const int64_t lim = (int64_t)1 << 31;
  if (arena_words >= lim || sched_cap >= lim / NB || n_graphs >= lim / ES_REC) return TSGNN_EUNSUPPORTED;
  if (((int64_t)h.R[0] + h.nmax) * h.ldf >= lim) return TSGNN_EUNSUPPORTED;
  for (int i = 0; i < h.nlev; ++i)
    if ((int64_t)h.R[i] * (i < h.nlev - 1 ? h.J : (h.Jf > 0 ? h.Jf : 1)) >= lim) return TSGNN_EUNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(state);
  if (al & 15) return TSGNN_EUNSUPPORTED;
  a.rec = records; a.n_graphs = n_graphs; a.arena = arena; a.arena_words = arena_words; a.sched = sched; a.sched_cap = sched_cap;
  a.state = state; a.ticket = ticket; a.ids_out = ids_out;
  int64_t most = 0;                                        // the largest piece per kind (no piece of a triplet closes the batch)
  for (int kind = 0; kind < ea_kinds(h.nlev); ++kind) most += ea_chunks(ea_len(h, top, kind));
  if (most >= 65536) return TSGNN_EUNSUPPORTED;
  if (NB == ES_B) {
    TSGNN_KNAME("eigen_triplet_gather_kernel");
    eigen_triplet_gather_kernel<<<dim3((unsigned)most, NB + 1), 256, 0, stream>>>(a);
  } else {
    TSGNN_KNAME("eigen_anchor_gather_kernel");
    eigen_anchor_gather_kernel<<<dim3((unsigned)most, NB + 1), 256, 0, stream>>>(a);
  }
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_eigen_triplet_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t arena_words,
                                   const int64_t* top_n, const int64_t* top_nnz, const int32_t* sched, int64_t sched_cap, int64_t* state,
                                   unsigned* ticket, const int64_t* desc, int32_t* ids_out, tsgnn_stream_t stream) {
  return es_gather_launch<ES_B>(records, n_graphs, arena, arena_words, top_n, top_nnz, sched, sched_cap, state, ticket, desc, ids_out, stream);
}

int tsgnn_eigen_anchor_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t arena_words,
                                  const int64_t* top_n, const int64_t* top_nnz, const int32_t* sched, int64_t sched_cap, int64_t* state,
                                  unsigned* ticket, const int64_t* desc, int32_t* ids_out, tsgnn_stream_t stream) {
  return es_gather_launch<ES_ANCHOR>(records, n_graphs, arena, arena_words, top_n, top_nnz, sched, sched_cap, state, ticket, desc, ids_out,
                                     stream);
}

}  // extern "C"
