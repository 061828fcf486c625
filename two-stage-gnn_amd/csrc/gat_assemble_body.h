// What the two launches that write the GAT encoder's packed batch share: the assembler (gat_assemble.hip: pieces named by a host
// description) and the stream's gather (gat_stream.hip: pieces found on the device from the schedule's cursor).  The layout of a
// piece buffer, the copy of one chunk with the piece's offset added, and the body of one (piece, array, chunk) workgroup.
#pragma once
#include "common.h"

namespace {

constexpr int GA_HMAX = 4;          // head counts whose edge-less indicator [R, H] is written (one per layer of the encoder)
constexpr int GA_CHUNK = 2048;      // words per workgroup: 256 threads x two 16-byte stores
constexpr int GA_HEADER = 29;       // words of a description's header (include/tsgnn.h)
enum { GA_ROWPTR, GA_ROWPTR_T, GA_COL, GA_COL_T, GA_SRC, GA_INV, GA_X, GA_ROWS, GA_LIST, GA_KINDS };

struct GaPiece {
  const int* src;
  int n, nr, nnz, k, mult;          // real rows, rows with the representative, entries, listed edge-less columns, Nmax - n
  int row0, e0, i0, gidx, last;     // where the piece goes: first row / entry / listed column, its graph number, closes the batch
};
// the batch's arrays: what a launch's argument struct carries beside its pieces (the bodies below are templates over that struct)
#define GA_OUTPUT_FIELDS                                                                                                  \
  int ldf, nH, H[GA_HMAX];                                                                                                \
  int *rowptr, *col, *rowptr_t, *col_t, *src_e_t, *inv, *graph_ptr, *row_graph, *row_slot, *iso_idx, *iso_ptr;            \
  float *row_mult, *iso_w, *x, *iso_cols[GA_HMAX];

__host__ __device__ inline int64_t ga_a4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// section starts of a piece buffer, in words: the nine sections, then the total
__host__ __device__ inline void ga_layout(int64_t nr, int64_t nnz, int64_t k, int64_t ldf, int64_t* off) {
  off[0] = 0;
  off[1] = ga_a4(off[0] + nr + 1);
  off[2] = ga_a4(off[1] + nr + 1);
  off[3] = ga_a4(off[2] + nnz);
  off[4] = ga_a4(off[3] + nnz);
  off[5] = ga_a4(off[4] + nnz);
  off[6] = ga_a4(off[5] + nnz);
  off[7] = ga_a4(off[6] + k);
  off[8] = ga_a4(off[7] + k);
  off[9] = ga_a4(off[8] + nr * ldf);
}

// elements of one array a piece writes
__host__ __device__ inline int64_t ga_len(const GaPiece& q, int kind, int ldf) {
  switch (kind) {
    case GA_ROWPTR: case GA_ROWPTR_T: return (int64_t)q.nr + (q.last ? 1 : 0);
    case GA_COL: case GA_COL_T: case GA_SRC: case GA_INV: return q.nnz;
    case GA_X: return (int64_t)q.nr * ldf;
    case GA_ROWS: return q.nr;
    default: return q.k > 0 ? q.k : 1;           // GA_LIST: its first thread also writes graph_ptr / iso_ptr
  }
}
__host__ __device__ inline int64_t ga_chunks(const GaPiece& q, int kind, int ldf) { return (ga_len(q, kind, ldf) + GA_CHUNK - 1) / GA_CHUNK; }

typedef int ga_i4u __attribute__((ext_vector_type(4), aligned(4)));      // four words from an address that is only word-aligned
typedef int ga_i4 __attribute__((ext_vector_type(4)));

// dst[0, len) = src[0, len) + add for chunk c of this workgroup; dst_word: index of dst[0] from a 16-byte aligned base
__device__ __forceinline__ void ga_copy_add(int* __restrict__ dst, const int* __restrict__ src, int64_t len, int add, int64_t dst_word,
                                            int64_t c) {
  const int64_t head = min((int64_t)((4 - (dst_word & 3)) & 3), len);
  const int64_t nvec = (len - head) >> 2;
  const int64_t tail0 = head + 4 * nvec;
  const int t = (int)threadIdx.x;
  if (c == 0) {
    if (t < head) dst[t] = src[t] + add;
    if (t >= 64 && tail0 + (t - 64) < len) dst[tail0 + (t - 64)] = src[tail0 + (t - 64)] + add;
  }
  const int64_t v1 = min(nvec, (c + 1) * (GA_CHUNK / 4));
  for (int64_t v = c * (GA_CHUNK / 4) + t; v < v1; v += 256) {
    const ga_i4u a = *reinterpret_cast<const ga_i4u*>(src + head + 4 * v);
    ga_i4 o = {a.x + add, a.y + add, a.z + add, a.w + add};
    *reinterpret_cast<ga_i4*>(dst + head + 4 * v) = o;
  }
}

// the workgroup that takes block b of piece q: which array it writes (GA_KINDS: none — the grid is sized for the piece with the
// most chunks), and b becomes the chunk inside that array
__device__ __forceinline__ int ga_kind_of(const GaPiece& q, int ldf, int64_t& b) {
  int kind = 0;
  for (; kind < GA_KINDS; ++kind) {
    const int64_t nc = ga_chunks(q, kind, ldf);
    if (b < nc) break;
    b -= nc;
  }
  return kind;
}

// chunk b of array `kind` of piece q -> its place in the batch's arrays `a` (a struct with GA_OUTPUT_FIELDS)
template <class A>
__device__ __forceinline__ void ga_piece_chunk(const A& a, const GaPiece& q, int kind, int64_t b) {
  int64_t off[10];
  ga_layout(q.nr, q.nnz, q.k, a.ldf, off);
  const int* s = q.src;
  switch (kind) {
    case GA_ROWPTR:   ga_copy_add(a.rowptr + q.row0, s + off[0], ga_len(q, kind, a.ldf), q.e0, q.row0, b); break;
    case GA_ROWPTR_T: ga_copy_add(a.rowptr_t + q.row0, s + off[1], ga_len(q, kind, a.ldf), q.e0, q.row0, b); break;
    case GA_COL:      ga_copy_add(a.col + q.e0, s + off[2], q.nnz, q.row0, q.e0, b); break;
    case GA_COL_T:    ga_copy_add(a.col_t + q.e0, s + off[3], q.nnz, q.row0, q.e0, b); break;
    case GA_SRC:      ga_copy_add(a.src_e_t + q.e0, s + off[4], q.nnz, q.e0, q.e0, b); break;
    case GA_INV:      ga_copy_add(a.inv + q.e0, s + off[5], q.nnz, q.e0, q.e0, b); break;
    case GA_X:        // (float bits + 0; rows of ldf = 4 m floats: the destination of a piece starts on 16 bytes)
      ga_copy_add(reinterpret_cast<int*>(a.x) + (int64_t)q.row0 * a.ldf, s + off[8], (int64_t)q.nr * a.ldf, 0, 0, b);
      break;
    case GA_ROWS: {
      const int64_t i = b * GA_CHUNK + threadIdx.x;
      for (int64_t r = i; r < min((int64_t)q.nr, (b + 1) * GA_CHUNK); r += 256) {
        const float m = r < q.n ? 1.f : (float)q.mult;
        const int64_t row = q.row0 + r;
        a.row_mult[row] = m;
        a.row_graph[row] = q.gidx;
        a.row_slot[row] = (int)r;
        const float w = (s[off[1] + r + 1] == s[off[1] + r]) ? m : 0.f;     // a column without an edge, times what it stands for
        for (int v = 0; v < a.nH; ++v)
          for (int h = 0; h < a.H[v]; ++h) a.iso_cols[v][row * a.H[v] + h] = w;
      }
      break;
    }
    default: {
      if (b == 0 && threadIdx.x == 0) {
        a.graph_ptr[q.gidx] = q.row0;
        a.iso_ptr[q.gidx] = q.i0;
        if (q.last) {
          a.graph_ptr[q.gidx + 1] = q.row0 + q.nr;
          a.iso_ptr[q.gidx + 1] = q.i0 + q.k;
        }
      }
      for (int64_t i = b * GA_CHUNK + threadIdx.x; i < min((int64_t)q.k, (b + 1) * GA_CHUNK); i += 256) {
        a.iso_idx[q.i0 + i] = s[off[6] + i] + q.row0;
        a.iso_w[q.i0 + i] = __int_as_float(s[off[7] + i]);
      }
    }
  }
}

// a description's header (include/tsgnn.h: tsgnn_gat_assemble_f32) -> the batch's arrays in `a` and its sizes R, E, I, B; false: a
// header no kernel must see
template <class A>
inline bool ga_unpack_header(const int64_t* d, A& a, int64_t& R, int64_t& E, int64_t& I, int64_t& B) {
  if (!d || (reinterpret_cast<uintptr_t>(d) & 7)) return false;
  R = d[1]; E = d[2]; I = d[3]; B = d[4];
  const int64_t ldf = d[5], nH = d[6];
  const int64_t lim = 2147483647;
  if (R < 0 || E < 0 || I < 0 || B < 1 || ldf < 4 || (ldf & 3) || nH < 0 || nH > GA_HMAX) return false;
  if (R >= lim || E >= lim || I >= lim || B >= lim || ldf >= lim) return false;
  a.ldf = (int)ldf; a.nH = (int)nH;
  for (int v = 0; v < GA_HMAX; ++v) {
    a.H[v] = (int)d[7 + v];
    a.iso_cols[v] = reinterpret_cast<float*>(d[25 + v]);
    if (v < nH && (d[7 + v] < 1 || d[7 + v] > 64 || !a.iso_cols[v])) return false;
  }
  for (int t = 11; t < 25; ++t)
    if (!d[t] || (d[t] & 15)) return false;                // every output: present, on 16 bytes
  a.rowptr = reinterpret_cast<int*>(d[11]); a.col = reinterpret_cast<int*>(d[12]); a.rowptr_t = reinterpret_cast<int*>(d[13]);
  a.col_t = reinterpret_cast<int*>(d[14]); a.src_e_t = reinterpret_cast<int*>(d[15]); a.inv = reinterpret_cast<int*>(d[16]);
  a.row_mult = reinterpret_cast<float*>(d[17]); a.graph_ptr = reinterpret_cast<int*>(d[18]); a.row_graph = reinterpret_cast<int*>(d[19]);
  a.row_slot = reinterpret_cast<int*>(d[20]); a.iso_idx = reinterpret_cast<int*>(d[21]); a.iso_w = reinterpret_cast<float*>(d[22]);
  a.iso_ptr = reinterpret_cast<int*>(d[23]); a.x = reinterpret_cast<float*>(d[24]);
  return true;
}

}  // namespace
