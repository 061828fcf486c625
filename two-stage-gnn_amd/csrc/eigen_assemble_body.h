// What the two launches that write the EigenGCN encoder's batch share: the chunk assembler (eigen_assemble.hip: pieces named by a host
// description) and the triplet stream's gather (eigen_stream.hip: three pieces found on the device from the schedule's cursor).  The
// layout of a piece buffer, the copy of one chunk with the piece's offset added, the body of one (piece, array, chunk) workgroup and
// the host-side reading of a description's header.
#pragma once
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

inline bool ea_ptr16(int64_t v) { return v != 0 && (v & 15) == 0; }

// the header of a description -> h; false: a header the kernels must not see (K is the caller's to check)
inline bool ea_unpack_header(const int64_t* d, EaHead& h) {
  if (!d || (reinterpret_cast<uintptr_t>(d) & 7)) return false;
  const int64_t K = d[0], B = d[1], nlev = d[2], J = d[3], Jf = d[4], ldf = d[5], nmax = d[6], first = d[7];
  const int64_t lim = 2147483647;
  if (nlev < 1 || nlev > EA_LMAX || J < 1 || J > 5 || Jf < 0 || Jf > 4 || ldf < 4 || (ldf & 3) || ldf >= lim) return false;
  if (B < 1 || B >= lim || K < 1 || K > B || K > EA_KMAX || nmax < 1 || nmax >= lim || (first != 0 && first != 1)) return false;
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
  return true;
}

}  // namespace
