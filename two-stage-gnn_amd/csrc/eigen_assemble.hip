// Resident one-graph pieces of the EigenGCN encoder -> the complete EigenBatch of a chunk of graphs (eigen_triplet.py): every level's
// packed CSR with its row bookkeeping, every pooling level's clusters / coefficients / bucket lists, the final coefficients and the
// feature rows, equal word for word to eigen_pool.concat_batches of the same one-graph batches.
//
// A piece is one int32 device buffer with piece-local indices, its sections starting on 16 bytes (tsgnn_eigen_assemble_layout):
//   per level graph i = 0..L:  rowptr [n_i + 1] | col [nnz_i] | val [nnz_i] (float bits)
//   per pooling level i < L:   cluster_of [n_i] | coef [n_i, J] (float bits) | bptr [n_{i+1} + 2] | members [n_i]
//   final [n_L, Jf] (float bits) | feature rows [n_0, ldf] (float bits)
//
// A workgroup takes one (piece, array, chunk of the array): it copies its chunk to the piece's place in the batch's array and adds
// the piece's row, entry or cluster offset in registers.  Every output word has one writer; nothing is atomic.  The destination
// decides the vector width: up to three single words until it sits on 16 bytes, 16-byte stores from there, up to three words behind.
// One more row of workgroups (blockIdx.y = K) counts the graphs that have each node slot (GraphBatch.slot_count).
// (The layout, the copies and the piece workgroup live in eigen_assemble_body.h: the triplet stream's gather, eigen_stream.hip, runs them too.)
//
// The pieces' records travel by value in the kernel arguments, up to EA_KMAX per launch; further launches write disjoint slices of
// the same arrays and continue the slot counts in stream order.  (One launch per chunk reading the records from a staged copy of the
// description in device memory was measured too and was not faster: profiles/r10/eigen_two_stage_launch_shapes.txt.)
#include "eigen_assemble_body.h"

namespace {

// slot_count[i][s] (+)= the pieces of this launch with n_i > s: one thread per (level, slot)
__device__ __forceinline__ void ea_slot_block(const EaArgs& a) {
  const EaHead& h = a.h;
  const int per = (h.nmax + 255) / 256;
  const int i = (int)(blockIdx.x / per);
  if (i >= h.nlev) return;
  const int s = (int)(blockIdx.x % per) * 256 + (int)threadIdx.x;
  if (s >= h.nmax) return;
  int cnt = h.first ? 0 : h.slot_count[i][s];
  for (int t = 0; t < h.K; ++t) cnt += a.p[t].n[i] > s ? 1 : 0;
  h.slot_count[i][s] = cnt;
}

__global__ __launch_bounds__(256) void eigen_assemble_kernel(EaArgs a) {
  if ((int)blockIdx.y == a.h.K)
    ea_slot_block(a);
  else
    ea_piece_block(a.h, a.p[blockIdx.y]);
}

// desc -> the kernel's arguments; false: a description the kernel must not see
inline bool ea_unpack(const int64_t* d, EaArgs& a, int64_t& most) {
  EaHead& h = a.h;
  if (!ea_unpack_header(d, h)) return false;
  const int64_t K = d[0], B = d[1], nlev = d[2], nmax = d[6];
  const int64_t lim = 2147483647;
  most = 0;
  for (int64_t t = 0; t < K; ++t) {
    const int64_t* w = d + EA_HEADER + t * EA_PIECE;
    const int64_t gidx = w[1], last = w[2];
    if (!ea_ptr16(w[0]) || gidx < 0 || gidx >= B || (last != 0 && last != 1) || (last && gidx != B - 1)) return false;
    for (int i = 0; i < nlev; ++i) {
      const int64_t n = w[3 + 4 * i], nnz = w[4 + 4 * i], row0 = w[5 + 4 * i], e0 = w[6 + 4 * i];
      if (n < 0 || n > nmax || nnz < 0 || row0 < 0 || e0 < 0) return false;
      // the piece stays inside the batch's arrays (whose sizes are themselves below 2^31)
      if (row0 + n > h.R[i] || e0 + nnz > h.E[i]) return false;
      if (last && (row0 + n != h.R[i] || e0 + nnz != h.E[i])) return false;
    }
    EaPiece& q = a.p[t];
    q.src = reinterpret_cast<const int*>(w[0]); q.gidx = (int)gidx; q.last = (int)last;
    for (int i = 0; i < EA_LMAX; ++i) {
      const bool used = i < nlev;
      q.n[i] = used ? (int)w[3 + 4 * i] : 0; q.nnz[i] = used ? (int)w[4 + 4 * i] : 0;
      q.row0[i] = used ? (int)w[5 + 4 * i] : 0; q.e0[i] = used ? (int)w[6 + 4 * i] : 0;
    }
    int64_t c = 0;
    for (int kind = 0; kind < ea_kinds((int)nlev); ++kind) c += ea_chunks(ea_len(h, q, kind));
    most = c > most ? c : most;
  }
  for (int64_t t = K; t < EA_KMAX; ++t) a.p[t] = a.p[0];
  const int64_t slots = nlev * ((nmax + 255) / 256);
  most = slots > most ? slots : most;
  return most < lim;
}

}  // namespace

extern "C" {

int tsgnn_eigen_assemble_header_words(void) { return EA_HEADER; }
int tsgnn_eigen_assemble_piece_words(void) { return EA_PIECE; }
int tsgnn_eigen_assemble_max_pieces(void) { return EA_KMAX; }
int tsgnn_eigen_assemble_max_levels(void) { return EA_LMAX - 1; }

int tsgnn_eigen_assemble_layout(int nlev, int J, int Jf, int64_t ldf, const int64_t* n, const int64_t* nnz, int64_t* off) {
  if (!n || !nnz || !off || nlev < 1 || J < 1 || J > 5 || Jf < 0 || Jf > 4 || ldf < 0 || (ldf & 3) || ldf >= 2147483647)
    return TSGNN_EINVAL;
  for (int i = 0; i < nlev; ++i)
    if (n[i] < 0 || nnz[i] < 0 || n[i] >= 2147483647 || nnz[i] >= 2147483647) return TSGNN_EINVAL;
  const int ns = 7 * nlev - 1;
  for (int s = 0; s < ns; ++s) off[s] = ea_section(n, nnz, nlev, J, Jf, (int)ldf, s);
  return TSGNN_OK;
}

int tsgnn_eigen_assemble_f32(const int64_t* desc, tsgnn_stream_t stream) {
  static_assert(sizeof(EaArgs) <= 4096, "the records travel in the kernel arguments");
  EaArgs a;
  int64_t most = 0;
  if (!ea_unpack(desc, a, most)) return TSGNN_EINVAL;
  const dim3 grid((unsigned)most, (unsigned)a.h.K + 1);
  TSGNN_KNAME("eigen_assemble_kernel");
  eigen_assemble_kernel<<<grid, 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
