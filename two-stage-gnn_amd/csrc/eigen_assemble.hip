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
//
// The pieces' records travel by value in the kernel arguments, up to EA_KMAX per launch; further launches write disjoint slices of
// the same arrays and continue the slot counts in stream order.  (One launch per chunk reading the records from a staged copy of the
// description in device memory was measured too and was not faster: profiles/r10/eigen_two_stage_launch_shapes.txt.)
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int EA_KMAX = 32;         // pieces per launch
constexpr int EA_LMAX = 4;          // level graphs (L + 1)
constexpr int EA_CHUNK = 2048;      // words per workgroup: 256 threads x two 16-byte stores
constexpr int EA_HEADER = 60, EA_PIECE = 19;

struct EaPiece {
  const int* src;
  int gidx, last;                   // its graph number; closes the batch
  int n[EA_LMAX], nnz[EA_LMAX];     // rows and entries of every level graph
  int row0[EA_LMAX], e0[EA_LMAX];   // where the piece goes: first row / entry of every level (first cluster of level i = row0[i + 1])
};
struct EaHead {
  int K, B, nlev, J, Jf, ldf, nmax, first;
  int R[EA_LMAX], E[EA_LMAX];       // rows and entries of the WHOLE batch
  int *rowptr[EA_LMAX], *col[EA_LMAX], *graph_ptr[EA_LMAX], *row_graph[EA_LMAX], *row_slot[EA_LMAX], *slot_count[EA_LMAX];
  float* val[EA_LMAX];
  int *cluster_of[EA_LMAX - 1], *bptr[EA_LMAX - 1], *members[EA_LMAX - 1];
  float* coef[EA_LMAX - 1];
  float *final_coef, *x;
};
struct EaArgs {
  EaHead h;
  EaPiece p[EA_KMAX];
};

__host__ __device__ inline int64_t ea_a4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// words of section s of a piece buffer whose level graphs have n[i] rows and nnz[i] entries (any number of levels: the layout
// function serves every piece buffer, the kernel only those of up to EA_LMAX level graphs)
template <class T>
__host__ __device__ inline int64_t ea_section_len(const T* n, const T* nnz, int nlev, int J, int Jf, int ldf, int s) {
  const int L = nlev - 1;
  if (s < 3 * nlev) return s % 3 == 0 ? (int64_t)n[s / 3] + 1 : (int64_t)nnz[s / 3];
  s -= 3 * nlev;
  if (s < 4 * L) {
    const int i = s / 4, t = s % 4;
    return t == 1 ? (int64_t)n[i] * J : t == 2 ? (int64_t)n[i + 1] + 2 : (int64_t)n[i];
  }
  s -= 4 * L;
  return s == 0 ? (int64_t)n[L] * Jf : (int64_t)n[0] * ldf;
}
// first word of section s (s = the number of sections: the buffer's length)
template <class T>
__host__ __device__ inline int64_t ea_section(const T* n, const T* nnz, int nlev, int J, int Jf, int ldf, int s) {
  int64_t o = 0;
  for (int t = 0; t < s; ++t) o = ea_a4(o + ea_section_len(n, nnz, nlev, J, Jf, ldf, t));
  return o;
}

// the arrays a piece writes, in the order its workgroups take them: five per level graph (rowptr, col, val, the row maps, the
// closing rowptr entries), four per pooling level (cluster_of, coef, bptr, members), then final, x and x's ghost rows
__host__ __device__ inline int ea_kinds(int nlev) { return 5 * nlev + 4 * (nlev - 1) + 3; }

__host__ __device__ inline int64_t ea_len(const EaHead& h, const EaPiece& p, int kind) {
  const int L = h.nlev - 1;
  if (kind < 5 * h.nlev) {
    const int i = kind / 5, t = kind % 5;
    switch (t) {
      case 0: return p.n[i];
      case 1: case 2: return p.nnz[i];
      case 3: return p.n[i] > 0 ? p.n[i] : 1;                 // (its first thread also writes graph_ptr)
      default: return p.last ? (int64_t)h.nmax + 1 : 0;
    }
  }
  kind -= 5 * h.nlev;
  if (kind < 4 * L) {
    const int i = kind / 4, t = kind % 4;
    return t == 1 ? (int64_t)p.n[i] * h.J : t == 2 ? (int64_t)p.n[i + 1] + 1 + (p.last ? 1 : 0) : (int64_t)p.n[i];
  }
  kind -= 4 * L;
  return kind == 0 ? (int64_t)p.n[L] * h.Jf : kind == 1 ? (int64_t)p.n[0] * h.ldf : (p.last ? (int64_t)h.nmax * h.ldf : 0);
}
__host__ __device__ inline int64_t ea_chunks(int64_t len) { return (len + EA_CHUNK - 1) / EA_CHUNK; }

typedef int ea_i4u __attribute__((ext_vector_type(4), aligned(4)));      // four words from an address that is only word-aligned
typedef int ea_i4 __attribute__((ext_vector_type(4)));

template <int MODE>
__device__ __forceinline__ int ea_shift(int v, int add) { return MODE == 0 ? v + add : (v >= 0 ? v + add : v); }

// dst[0, len) = shift(src[0, len)) for chunk c of this workgroup; dst_word: index of dst[0] from a 16-byte aligned base.
// MODE 0: + add; MODE 1: + add where the word is not negative (cluster_of keeps its -1)
template <int MODE>
__device__ __forceinline__ void ea_copy(int* __restrict__ dst, const int* __restrict__ src, int64_t len, int add, int64_t dst_word, int64_t c) {
  const int64_t head = min((int64_t)((4 - (dst_word & 3)) & 3), len);
  const int64_t nvec = (len - head) >> 2;
  const int64_t tail0 = head + 4 * nvec;
  const int t = (int)threadIdx.x;
  if (c == 0) {
    if (t < head) dst[t] = ea_shift<MODE>(src[t], add);
    if (t >= 64 && tail0 + (t - 64) < len) dst[tail0 + (t - 64)] = ea_shift<MODE>(src[tail0 + (t - 64)], add);
  }
  const int64_t v1 = min(nvec, (c + 1) * (EA_CHUNK / 4));
  for (int64_t v = c * (EA_CHUNK / 4) + t; v < v1; v += 256) {
    const ea_i4u a = *reinterpret_cast<const ea_i4u*>(src + head + 4 * v);
    ea_i4 o = {ea_shift<MODE>(a.x, add), ea_shift<MODE>(a.y, add), ea_shift<MODE>(a.z, add), ea_shift<MODE>(a.w, add)};
    *reinterpret_cast<ea_i4*>(dst + head + 4 * v) = o;
  }
}

// dst[0, len) = value, the same way
__device__ __forceinline__ void ea_fill(int* __restrict__ dst, int64_t len, int value, int64_t dst_word, int64_t c) {
  const int64_t head = min((int64_t)((4 - (dst_word & 3)) & 3), len);
  const int64_t nvec = (len - head) >> 2;
  const int64_t tail0 = head + 4 * nvec;
  const int t = (int)threadIdx.x;
  if (c == 0) {
    if (t < head) dst[t] = value;
    if (t >= 64 && tail0 + (t - 64) < len) dst[tail0 + (t - 64)] = value;
  }
  const int64_t v1 = min(nvec, (c + 1) * (EA_CHUNK / 4));
  const ea_i4 o = {value, value, value, value};
  for (int64_t v = c * (EA_CHUNK / 4) + t; v < v1; v += 256) *reinterpret_cast<ea_i4*>(dst + head + 4 * v) = o;
}

// the work of one workgroup for piece p
__device__ __forceinline__ void ea_piece_block(const EaHead& h, const EaPiece& p) {
  int64_t b = blockIdx.x;
  const int nk = ea_kinds(h.nlev);
  int kind = 0;
  for (; kind < nk; ++kind) {
    const int64_t nc = ea_chunks(ea_len(h, p, kind));
    if (b < nc) break;
    b -= nc;
  }
  if (kind == nk) return;                       // (the grid is sized for the piece with the most chunks)
  const int nlev = h.nlev, L = nlev - 1, J = h.J, Jf = h.Jf, ldf = h.ldf;
  const int* s = p.src;
  const int64_t len = ea_len(h, p, kind);
  if (kind < 5 * nlev) {
    const int i = kind / 5, t = kind % 5;
    const int row0 = p.row0[i], e0 = p.e0[i];
    switch (t) {
      case 0: ea_copy<0>(h.rowptr[i] + row0, s + ea_section(p.n, p.nnz, nlev, J, Jf, ldf, 3 * i), len, e0, row0, b); break;
      case 1: ea_copy<0>(h.col[i] + e0, s + ea_section(p.n, p.nnz, nlev, J, Jf, ldf, 3 * i + 1), len, row0, e0, b); break;
      case 2: ea_copy<0>(reinterpret_cast<int*>(h.val[i]) + e0, s + ea_section(p.n, p.nnz, nlev, J, Jf, ldf, 3 * i + 2), len, 0, e0, b); break;
      case 3: {
        const int n = p.n[i], g = p.gidx;
        if (b == 0 && threadIdx.x == 0) {
          h.graph_ptr[i][g] = row0;
          if (p.last) h.graph_ptr[i][g + 1] = row0 + n;
        }
        for (int64_t r = b * EA_CHUNK + threadIdx.x; r < min((int64_t)n, (b + 1) * EA_CHUNK); r += 256) {
          h.row_graph[i][row0 + r] = g;
          h.row_slot[i][row0 + r] = (int)r;
        }
        break;
      }
      default: ea_fill(h.rowptr[i] + h.R[i], len, h.E[i], h.R[i], b);        // the closing entry and the Nmax empty ghost-slot rows
    }
    return;
  }
  kind -= 5 * nlev;
  if (kind < 4 * L) {
    const int i = kind / 4, t = kind % 4;
    const int r0 = p.row0[i], c0 = p.row0[i + 1];
    const int sec = 3 * nlev + 4 * i + t;
    const int* from = s + ea_section(p.n, p.nnz, nlev, J, Jf, ldf, sec);
    switch (t) {
      case 0: ea_copy<1>(h.cluster_of[i] + r0, from, len, c0, r0, b); break;
      case 1: ea_copy<0>(reinterpret_cast<int*>(h.coef[i]) + (int64_t)r0 * J, from, len, 0, (int64_t)r0 * J, b); break;
      case 2: ea_copy<0>(h.bptr[i] + c0 + p.gidx, from, len, r0, (int64_t)c0 + p.gidx, b); break;   // k + 1 buckets per graph
      default: ea_copy<0>(h.members[i] + r0, from, len, r0, r0, b);
    }
    return;
  }
  kind -= 4 * L;
  const int sec = 3 * nlev + 4 * L + kind;
  if (kind == 0) {
    const int64_t at = (int64_t)p.row0[L] * Jf;
    ea_copy<0>(reinterpret_cast<int*>(h.final_coef) + at, s + ea_section(p.n, p.nnz, nlev, J, Jf, ldf, sec), len, 0, at, b);
  } else if (kind == 1) {                       // (rows of ldf = 4 m floats: the destination of a piece starts on 16 bytes)
    ea_copy<0>(reinterpret_cast<int*>(h.x) + (int64_t)p.row0[0] * ldf, s + ea_section(p.n, p.nnz, nlev, J, Jf, ldf, sec), len, 0, 0, b);
  } else {
    ea_fill(reinterpret_cast<int*>(h.x) + (int64_t)h.R[0] * ldf, len, 0, 0, b);                          // the Nmax ghost rows: zero
  }
}

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

inline bool ea_ptr16(int64_t v) { return v != 0 && (v & 15) == 0; }

// desc -> the kernel's arguments; false: a description the kernel must not see
inline bool ea_unpack(const int64_t* d, EaArgs& a, int64_t& most) {
  if (!d || (reinterpret_cast<uintptr_t>(d) & 7)) return false;
  const int64_t K = d[0], B = d[1], nlev = d[2], J = d[3], Jf = d[4], ldf = d[5], nmax = d[6], first = d[7];
  const int64_t lim = 2147483647;
  if (nlev < 1 || nlev > EA_LMAX || J < 1 || J > 5 || Jf < 0 || Jf > 4 || ldf < 4 || (ldf & 3) || ldf >= lim) return false;
  if (B < 1 || B >= lim || K < 1 || K > B || K > EA_KMAX || nmax < 1 || nmax >= lim || (first != 0 && first != 1)) return false;
  EaHead& h = a.h;
  h.K = (int)K; h.B = (int)B; h.nlev = (int)nlev; h.J = (int)J; h.Jf = (int)Jf; h.ldf = (int)ldf; h.nmax = (int)nmax; h.first = (int)first;
  const int L = (int)nlev - 1;
  if (!ea_ptr16(d[9]) || (Jf > 0 && !ea_ptr16(d[10]))) return false;
  h.x = reinterpret_cast<float*>(d[9]);
  h.final_coef = reinterpret_cast<float*>(Jf > 0 ? d[10] : 0);
  for (int i = 0; i < EA_LMAX; ++i) {
    const bool used = i < nlev;
    const int64_t R = d[12 + 2 * i], E = d[13 + 2 * i];
    if (used && (R < 0 || E < 0 || R + nmax + 1 >= lim || E >= lim)) return false;
    h.R[i] = used ? (int)R : 0;
    h.E[i] = used ? (int)E : 0;
    const int64_t* o = d + 20 + 7 * i;
    for (int t = 0; t < 7; ++t)
      if (used && !ea_ptr16(o[t])) return false;                       // every output: present, on 16 bytes
    h.rowptr[i] = reinterpret_cast<int*>(used ? o[0] : 0); h.col[i] = reinterpret_cast<int*>(used ? o[1] : 0);
    h.val[i] = reinterpret_cast<float*>(used ? o[2] : 0); h.graph_ptr[i] = reinterpret_cast<int*>(used ? o[3] : 0);
    h.row_graph[i] = reinterpret_cast<int*>(used ? o[4] : 0); h.row_slot[i] = reinterpret_cast<int*>(used ? o[5] : 0);
    h.slot_count[i] = reinterpret_cast<int*>(used ? o[6] : 0);
  }
  for (int i = 0; i < EA_LMAX - 1; ++i) {
    const bool used = i < L;
    const int64_t* o = d + 48 + 4 * i;
    for (int t = 0; t < 4; ++t)
      if (used && !ea_ptr16(o[t])) return false;
    h.cluster_of[i] = reinterpret_cast<int*>(used ? o[0] : 0); h.coef[i] = reinterpret_cast<float*>(used ? o[1] : 0);
    h.bptr[i] = reinterpret_cast<int*>(used ? o[2] : 0); h.members[i] = reinterpret_cast<int*>(used ? o[3] : 0);
  }
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
