// Resident one-graph pieces of the GAT encoder's packed batch -> the arrays of the concatenated batch, in ONE launch for up to 8
// pieces (gat_triplet.py).  A piece is one int32 device buffer that holds, in sections that start on 16 bytes
// (tsgnn_gat_assemble_layout): rowptr [nr + 1] | rowptr_t [nr + 1] | col [nnz] | col_t [nnz] | src_e_t [nnz] | inv [nnz] |
// edge-less rows [k] | their weights [k] (float bits) | feature rows [nr, ldf] (float bits), all with piece-local indices.
// nr = n real rows + one ghost representative when n < Nmax (GraphBatch.from_dense_ghost1's layout).
//
// A workgroup takes one (piece, array, chunk of the array): it copies its chunk to the piece's place in the batch's array and adds
// the piece's row or entry offset in registers.  Every output element has one writer; nothing is atomic.  The destination decides
// the vector width: up to three scalar words until it sits on 16 bytes, 16-byte stores from there, up to three scalar words behind.
// The layout, the copy and the workgroup's body live in gat_assemble_body.h, shared with the stream's gather (gat_stream.hip).
#include "gat_assemble_body.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int GA_KMAX = 8;          // pieces per launch
constexpr int GA_PIECE = 11;

struct GaArgs {
  GaPiece p[GA_KMAX];
  int K;
  GA_OUTPUT_FIELDS
};

__global__ __launch_bounds__(256) void gat_assemble_kernel(GaArgs a) {
  const GaPiece& q = a.p[blockIdx.y];
  int64_t b = blockIdx.x;
  const int kind = ga_kind_of(q, a.ldf, b);
  if (kind == GA_KINDS) return;                 // (the grid is sized for the piece with the most chunks)
  ga_piece_chunk(a, q, kind, b);
}

// desc -> args; false: a description the kernel must not see
inline bool ga_unpack(const int64_t* d, GaArgs& a) {
  int64_t R, E, I, B;
  if (!ga_unpack_header(d, a, R, E, I, B)) return false;
  const int64_t K = d[0];
  if (K < 1 || K > GA_KMAX) return false;
  a.K = (int)K;
  for (int t = 0; t < a.K; ++t) {
    const int64_t* w = d + GA_HEADER + t * GA_PIECE;
    const int64_t n = w[1], nr = w[2], nnz = w[3], k = w[4], mult = w[5], row0 = w[6], e0 = w[7], i0 = w[8], gidx = w[9], last = w[10];
    if (!w[0] || (w[0] & 15)) return false;
    if (n < 0 || nr < n || nr > n + 1 || nnz < 0 || k < 0 || k > nr || mult < 0 || row0 < 0 || e0 < 0 || i0 < 0 || gidx < 0 || (last != 0 && last != 1))
      return false;
    if (nr == n + 1 && mult < 1) return false;
    // the piece stays inside the batch's arrays (whose sizes are themselves below 2^31)
    if (row0 + nr > R || e0 + nnz > E || i0 + k > I || gidx >= B) return false;
    if (last && (row0 + nr != R || e0 + nnz != E || i0 + k != I || gidx != B - 1)) return false;
    GaPiece& q = a.p[t];
    q.src = reinterpret_cast<const int*>(w[0]);
    q.n = (int)n; q.nr = (int)nr; q.nnz = (int)nnz; q.k = (int)k; q.mult = (int)mult;
    q.row0 = (int)row0; q.e0 = (int)e0; q.i0 = (int)i0; q.gidx = (int)gidx; q.last = (int)last;
  }
  for (int t = a.K; t < GA_KMAX; ++t) a.p[t] = a.p[0];
  return true;
}

}  // namespace

extern "C" {

int tsgnn_gat_assemble_header_words(void) { return GA_HEADER; }
int tsgnn_gat_assemble_piece_words(void) { return GA_PIECE; }
int tsgnn_gat_assemble_max_pieces(void) { return GA_KMAX; }

int tsgnn_gat_assemble_layout(int64_t nr, int64_t nnz, int64_t k, int64_t ldf, int64_t* off) {
  if (!off || nr < 0 || nnz < 0 || k < 0 || ldf < 0 || (ldf & 3)) return TSGNN_EINVAL;
  if (nr >= 2147483647 || nnz >= 2147483647 || k > nr) return TSGNN_EINVAL;
  ga_layout(nr, nnz, k, ldf, off);
  return TSGNN_OK;
}

int tsgnn_gat_assemble_f32(const int64_t* desc, tsgnn_stream_t stream) {
  GaArgs a;
  if (!ga_unpack(desc, a)) return TSGNN_EINVAL;
  int64_t most = 0;
  for (int t = 0; t < a.K; ++t) {
    int64_t c = 0;
    for (int kind = 0; kind < GA_KINDS; ++kind) c += ga_chunks(a.p[t], kind, a.ldf);
    most = c > most ? c : most;
  }
  if (most >= 2147483647) return TSGNN_EINVAL;
  TSGNN_KNAME("gat_assemble_kernel");
  gat_assemble_kernel<<<dim3((unsigned)most, (unsigned)a.K), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
