// GAT mini-batch stream: a NEW batch of B graphs every replay of one hipGraph (Code/sage+gat+diffpool/train.py:104-131 with --method=GAT:
// DGATEncoderGraph(final_dim='number_classes') -> model.loss(ypred, label) -> clip -> Adam, once per optimiser step; host side:
// gat_stream.MiniBatchStream).  csrc/gat_stream.hip writes the packed GAT batch of 3 pieces (or 1) per schedule entry; this is that
// launch for entries of 1 <= B <= 128 pieces: the same arena (gat_stream.pack_arena), the same chunk copy (gat_assemble_body.h:
// ga_kind_of / ga_piece_chunk, unchanged), the same [HEAD | schedule] buffer with its cursor (stream_protocol.h), and
//
//   prologue   the first B threads load the entry's 32-byte records; the first two waves form the exclusive prefix sums of nr, nnz and
//              k over the entry's graphs with wave shuffles (two_wave_prefix, called twice: it carries two quantities and there are
//              three; wave 1 adds wave 0's total through LDS — B = 64 / 65 sit on that boundary)
//   body       piece y's chunk b with q.row0 / e0 / i0 from the prefix, q.gidx = y, q.last = (y == B - 1); the workgroup that takes the
//              first chunk of a piece's list also writes ids_out[y] and label_out[y] (int64: what mp.cross_entropy takes)
//   padding    one further set of workgroups strides over [R, capacity) of the per-row arrays, as gs_gather_body does
//
// Behind the entry's own R rows / E entries / I listed edge-less columns everything up to capacity is inert, by csrc/gat_stream.hip's
// contract: rowptr, rowptr_t (R .. row_cap] = E; x, row_mult, iso_cols_v rows +0; row_graph B - 1 (in bounds for the readers'
// iso_ptr[row_graph[r] + 1]); row_slot 0; graph_ptr[B] = R, iso_ptr[B] = I; col, col_t, src_e_t, inv past E and the list past I are not
// written.
//
// Grid: 1-D, (chunks of the dataset's largest piece, summed over its arrays) x (B + 1); workgroup w takes piece w / chunks and chunk
// w % chunks, so stream_ticket_sharded applies as it stands (a DD-shaped batch of 128 graphs has thousands of workgroups).  Every
// workgroup reads the cursor before its first barrier and draws its ticket behind its stores.  The capacities may lie below B times the
// largest piece (gat_stream.MiniBatchStream.load checks every entry on the host): an entry that does not fit, or that names a record
// whose piece leaves the arena or does not start on 16 bytes, writes NOTHING and still advances the cursor.  One writer per word, plain
// vector stores (16 bytes wherever the destination sits on 16 bytes), the ticket words are the only atomics; nobody waits for anybody.
#include "gat_assemble_body.h"
#include "stream_protocol.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int GB_REC = 8;                 // int32 words of a record: piece offset (words), n, nr, nnz, k, Nmax - n, index, 0

struct GbArgs {
  const int32_t* rec; int64_t n_graphs; const int32_t* arena; int64_t arena_words;
  const int32_t* labels;                  // [n_graphs]
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}; ticket: 32 shards + the top
  int B; int max_nr, max_nnz, max_k; unsigned chunks;                             // chunks: workgroups per piece
  int64_t row_cap, nnz_cap, iso_cap; int32_t* ids_out; int64_t* label_out;
  GA_OUTPUT_FIELDS
};

// the stores of workgroup (y, b) once the entry is known to fit
__device__ __forceinline__ void gb_write(const GbArgs& a, const int4 r0, const int4 r1, int y, int64_t b, int row0, int e0, int i0,
                                         int64_t R, int64_t E) {
  const int tid = threadIdx.x;
  if (y < a.B) {
    GaPiece q;
    q.src = a.arena + r0.x;
    q.n = r0.y; q.nr = r0.z; q.nnz = r0.w; q.k = r1.x; q.mult = r1.y;
    q.row0 = row0; q.e0 = e0; q.i0 = i0;
    q.gidx = y; q.last = y == a.B - 1;
    const int kind = ga_kind_of(q, a.ldf, b);
    if (kind == GA_KINDS) return;               // (the grid is sized for the largest piece of the dataset)
    ga_piece_chunk(a, q, kind, b);
    if (kind == GA_LIST && b == 0) {            // the batch's own small arrays: one writer per word
      if (tid == 64) a.ids_out[y] = r1.z;
      if (tid == 65) a.label_out[y] = (int64_t)a.labels[r1.z];
    }
    return;
  }
  // the padding: this set of workgroups strides over [R, capacity) of every per-row array
  const int64_t i = b * 256 + tid, S = (int64_t)a.chunks * 256;
  const int Ei = (int)E;
  for (int64_t r = R + 1 + i; r <= a.row_cap; r += S) {
    a.rowptr[r] = Ei;
    a.rowptr_t[r] = Ei;
  }
  for (int64_t r = R + i; r < a.row_cap; r += S) {
    a.row_mult[r] = 0.f;
    a.row_graph[r] = a.B - 1;
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

__global__ __launch_bounds__(256) void gat_batch_gather_kernel(GbArgs a) {
  __shared__ int4 rec_s[STREAM_MAX_B][2];                   // offset, n, nr, nnz | k, Nmax - n, index, 0
  __shared__ int pre_r[STREAM_MAX_B + 1], pre_e[STREAM_MAX_B + 1], pre_i[STREAM_MAX_B + 1], pre_0[STREAM_MAX_B + 1];
  __shared__ int wtot_a[2][2], wtot_b[2][2];
  __shared__ long long cur_s;
  const int tid = threadIdx.x;
  int nr_i = 0, nnz_i = 0, k_i = 0, bad = 0;
  if (tid < a.B) {
    long long cur;
    const int64_t id = stream_entry_id(a.state, a.sched, a.sched_cap, a.n_graphs, a.B, tid, cur);
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + id * GB_REC);
    const int4 r1 = *reinterpret_cast<const int4*>(a.rec + id * GB_REC + 4);
    rec_s[tid][0] = r0;
    rec_s[tid][1] = make_int4(r1.x, r1.y, (int)id, 0);
    if (tid == 0) cur_s = cur;
    // a record no chunk copy must follow: sizes outside the arena's largest piece, a piece off 16 bytes or past the arena's end
    bad = r0.x < 0 || (r0.x & 3) || r0.y < 0 || r0.y > r0.z || r0.z > a.max_nr || r0.w < 0 || r0.w > a.max_nnz || r1.x < 0 ||
          r1.x > a.max_k || r1.x > r0.z;
    if (!bad) {
      int64_t off[10];
      ga_layout(r0.z, r0.w, r1.x, a.ldf, off);
      bad = (int64_t)r0.x + off[9] > a.arena_words;
      nr_i = r0.z; nnz_i = r0.w; k_i = r1.x;
    }
  }
  two_wave_prefix(nr_i, nnz_i, tid, wtot_a, pre_r, pre_e);  // (every workgroup has READ the cursor in front of these barriers)
  two_wave_prefix(k_i, 0, tid, wtot_b, pre_i, pre_0);       // (pre_0 is a sink: the helper carries two quantities, there is no fourth)
  bad = __syncthreads_or(bad);

  const int64_t R = pre_r[a.B], E = pre_e[a.B], I = pre_i[a.B];
  // (gat_stream.MiniBatchStream.load refuses an entry that does not fit; one that reaches the launch all the same writes nothing)
  if (!bad && R <= a.row_cap && E <= a.nnz_cap && I <= a.iso_cap) {
    const int y = (int)(blockIdx.x / a.chunks);
    const int64_t b = blockIdx.x - (unsigned)y * a.chunks;
    const int ys = y < a.B ? y : 0;
    gb_write(a, rec_s[ys][0], rec_s[ys][1], y, b, pre_r[ys], pre_e[ys], pre_i[ys], R, E);
  }
  // behind the stores, so that no wave waits for the atomic's round trip in front of its work
  if (tid == 0) stream_ticket_sharded(a.ticket, a.state, cur_s);
}

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_gat_batch_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t arena_words, int64_t max_nr,
                               int64_t max_nnz, int64_t max_k, const int32_t* labels, const int32_t* sched, int64_t sched_cap,
                               int64_t* state, unsigned* ticket, int B, const int64_t* desc, int32_t* ids_out, int64_t* label_out,
                               tsgnn_stream_t stream) {
  if (!records || !arena || !labels || !sched || !state || !ticket || !desc || !ids_out || !label_out) return TSGNN_EINVAL;
  if (B < 1 || B > STREAM_MAX_B) return TSGNN_EINVAL;
  if (n_graphs <= 0 || sched_cap <= 0 || arena_words <= 0 || max_nr < 1 || max_nnz < 0 || max_k < 0 || max_k > max_nr) return TSGNN_EINVAL;
  GbArgs a{};
  int64_t R, E, I, Bd;
  if (!ga_unpack_header(desc, a, R, E, I, Bd) || Bd != B) return TSGNN_EINVAL;
  // every piece of the arena fits the batch on its own (max_nr / max_nnz / max_k are the caller's word, as the arena is).  Whether an
  // ENTRY fits is the uploader's check (gat_stream.MiniBatchStream.load): the kernel writes nothing for one that does not.
  if (R < max_nr || E < max_nnz || I < max_k) return TSGNN_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  if (arena_words >= lim || sched_cap >= lim / B || R * a.ldf >= lim || max_nr >= lim / B || max_nnz >= lim / B) return TSGNN_EUNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(state);
  if ((al & 15) || (reinterpret_cast<uintptr_t>(label_out) & 7)) return TSGNN_EUNSUPPORTED;
  GaPiece top{};                                           // the largest piece per kind, closing entries included
  top.nr = (int)max_nr; top.nnz = (int)max_nnz; top.k = (int)max_k; top.last = 1;
  int64_t most = 0;
  for (int kind = 0; kind < GA_KINDS; ++kind) most += ga_chunks(top, kind, a.ldf);
  if (most * (B + 1) >= lim) return TSGNN_EUNSUPPORTED;
  a.rec = records; a.n_graphs = n_graphs; a.arena = arena; a.arena_words = arena_words; a.labels = labels;
  a.sched = sched; a.sched_cap = sched_cap; a.state = state; a.ticket = ticket;
  a.B = B; a.max_nr = (int)max_nr; a.max_nnz = (int)max_nnz; a.max_k = (int)max_k; a.chunks = (unsigned)most;
  a.row_cap = R; a.nnz_cap = E; a.iso_cap = I; a.ids_out = ids_out; a.label_out = label_out;
  TSGNN_KNAME("gat_batch_gather_kernel");
  gat_batch_gather_kernel<<<(unsigned)(most * (B + 1)), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
