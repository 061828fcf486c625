// Eigen-pooling (EigenGCN, Code/eigengcn/encoders.py:384-417): X' = P^T Z with a block-sparse P (every node in at most one
// cluster), fused with the max readout of the same embedding rows Z.
//
//   pooled  : X'[c, j*C + f] = sum_{v in c} u_j(v) Z[v, f]            (c = a cluster = a row of the next level's packed layout)
//   final   : s[b, j*C + f]  = sum_{v in b} u_j(v) Z[v, f],  out = max(s, 0)   (one single-column matrix per j: the readout over
//             Nmax rows of a tensor whose only non-zero row is row 0)
//
// One workgroup per (graph, 32-column tile): 8 lanes x float4 per row, 32 row groups.  A row group owns whole clusters and sums
// their members in member order (fixed order, no atomics: bitwise repeatable); the max readout of the rows it reads is reduced
// over the row groups through LDS (ties: the lowest row wins, as torch.max's first index over the padded slots).
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int EP_LANES = 8;                 // lanes per row: 8 x 4 = 32 columns per tile
constexpr int EP_TILE = EP_LANES * 4;
constexpr int EP_GROUPS = 256 / EP_LANES;   // row groups per workgroup
constexpr int EP_JMAX = 5;

template <bool V4>
__device__ __forceinline__ void ld4(const float* __restrict__ p, int f, int C, float (&v)[4]) {
  if (V4) {
    if (f < C) {
      const float4 t = *reinterpret_cast<const float4*>(p + f);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (f + k < C) ? p[f + k] : 0.f;
  }
}

template <bool V4>
__device__ __forceinline__ void st4(float* __restrict__ p, int f, int C, const float (&v)[4]) {
  if (V4) {
    if (f < C) *reinterpret_cast<float4*>(p + f) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (f + k < C) p[f + k] = v[k];
  }
}

__device__ __forceinline__ void take_max(float& bv, int& br, float v, int r) {
  // larger value wins; on a tie the lower row (NaN-free inputs)
  if (v > bv || (v == bv && r < br)) { bv = v; br = r; }
}

struct EpFwd {
  const float* z; int64_t ldz; int C;
  const int* gp0; int64_t n_rows0; int nmax; int ghost_mode;   // ghost_mode 0: no ghost rows, 1: ghost rows are zero, 2: read them
  const int* gp1; const int* bptr; const int* members;         // non-final: the next level's graph_ptr, the bucket CSR of the rows
  const float* coef; int J;                                     // [n_rows0, J]
  float* out; int64_t ldo; int64_t n_rows1; int n_ghost1;      // non-final: pooled rows [n_rows1 + n_ghost1, ldo]; final: [B, ldo]
  float* fsum;                                                  // final: s [B, J*C]
  float* ro; int64_t ldro; int* arg;                            // readout of z (nullable), arg [B, C] = winning row or -1
  int B;
};

// CAP (pooled levels of a capacity batch, eigen_stream.py): n_rows1 is the row capacity of the next level and gp1[B] its real row
// count; the padding rows [gp1[B], n_rows1) are zeroed with the ghost rows
template <bool FINAL, bool V4, bool CAP = false>
__global__ __launch_bounds__(256) void eigen_pool_fwd(EpFwd a) {
  __shared__ float s_val[EP_GROUPS][EP_TILE];
  __shared__ int s_row[EP_GROUPS][EP_TILE];
  __shared__ float s_sum[FINAL ? EP_GROUPS : 1][FINAL ? EP_JMAX * EP_TILE : 1];
  const int b = blockIdx.x;
  const int lane = threadIdx.x % EP_LANES, grp = threadIdx.x / EP_LANES;
  const int f = blockIdx.y * EP_TILE + lane * 4;
  const int r0 = a.gp0[b], r1 = a.gp0[b + 1];
  const bool want_ro = a.ro != nullptr;
  float bv[4];
  int br[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { bv[k] = -INFINITY; br[k] = 0x7fffffff; }

  auto readout = [&](const float (&v)[4], int r) {
#pragma unroll
    for (int k = 0; k < 4; ++k) take_max(bv[k], br[k], v[k], r);
  };

  if (FINAL) {
    // one "cluster" per graph: row group g sums rows r0 + g, r0 + g + 32, ... then the partial sums are added in group order
    float acc[EP_JMAX][4];
#pragma unroll
    for (int j = 0; j < EP_JMAX; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[j][k] = 0.f;
    for (int r = r0 + grp; r < r1; r += EP_GROUPS) {
      float v[4];
      ld4<V4>(a.z + (int64_t)r * a.ldz, f, a.C, v);
      if (want_ro) readout(v, r);
#pragma unroll
      for (int j = 0; j < EP_JMAX; ++j) {
        if (j < a.J) {
          const float u = a.coef[(int64_t)r * a.J + j];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[j][k] = fmaf(u, v[k], acc[j][k]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < EP_JMAX; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) s_sum[grp][j * EP_TILE + lane * 4 + k] = acc[j][k];
  } else {
    // clusters of graph b: rows [gp1[b], gp1[b+1]) of the next level.  Buckets (tsgnn_eigen_pool_from_dense_f32's key): gp1[b] + b
    // holds the graph's unassigned rows (cluster_of = -1: readout only), c + b + 1 the members of cluster c
    const int c0 = a.gp1[b], c1 = a.gp1[b + 1];
    for (int m = a.bptr[c0 + b] + grp; m < a.bptr[c0 + b + 1]; m += EP_GROUPS) {
      const int r = a.members[m];
      float v[4];
      ld4<V4>(a.z + (int64_t)r * a.ldz, f, a.C, v);
      if (want_ro) readout(v, r);
    }
    for (int c = c0 + grp; c < c1; c += EP_GROUPS) {
      const int mb = a.bptr[c + b + 1], me = a.bptr[c + b + 2];
      float acc[EP_JMAX][4];
#pragma unroll
      for (int j = 0; j < EP_JMAX; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[j][k] = 0.f;
      for (int m = mb; m < me; ++m) {
        const int r = a.members[m];
        float v[4];
        ld4<V4>(a.z + (int64_t)r * a.ldz, f, a.C, v);
        if (want_ro) readout(v, r);
#pragma unroll
        for (int j = 0; j < EP_JMAX; ++j) {
          if (j < a.J) {
            const float u = a.coef[(int64_t)r * a.J + j];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[j][k] = fmaf(u, v[k], acc[j][k]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < EP_JMAX; ++j)
        if (j < a.J) st4<V4>(a.out + (int64_t)c * a.ldo + (int64_t)j * a.C, f, a.C, acc[j]);
    }
    // the next level's ghost-slot rows are zero (rows >= K_b of the padded P^T Z); shared out over the batch's workgroups
    // (CAP: and so are the padding rows behind the batch's last real cluster, which sit right in front of them)
    const int64_t pad = CAP ? a.n_rows1 - a.gp1[a.B] : 0;
    for (int64_t s = b + a.B * grp - pad; s < a.n_ghost1; s += a.B * EP_GROUPS) {
      const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < a.J; ++j) st4<V4>(a.out + (a.n_rows1 + s) * a.ldo + (int64_t)j * a.C, f, a.C, zero4);
    }
  }

  if (want_ro) {
    const int n_b = r1 - r0;
    if (a.ghost_mode == 1 && n_b < a.nmax && grp == 0) {
      const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
      readout(zero4, (int)(a.n_rows0 + n_b));                 // the padded slots' zeros (the masked embedding)
    } else if (a.ghost_mode == 2) {
      for (int s = n_b + grp; s < a.nmax; s += EP_GROUPS) {
        const int r = (int)(a.n_rows0 + s);
        float v[4];
        ld4<V4>(a.z + (int64_t)r * a.ldz, f, a.C, v);
        readout(v, r);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { s_val[grp][lane * 4 + k] = bv[k]; s_row[grp][lane * 4 + k] = br[k]; }
  }
  __syncthreads();
  if (threadIdx.x < EP_TILE) {
    const int col = threadIdx.x, fc = blockIdx.y * EP_TILE + col;
    if (fc < a.C) {
      if (want_ro) {
        float v = s_val[0][col];
        int r = s_row[0][col];
        for (int g = 1; g < EP_GROUPS; ++g) take_max(v, r, s_val[g][col], s_row[g][col]);
        const bool none = r == 0x7fffffff;
        a.ro[(int64_t)b * a.ldro + fc] = none ? 0.f : v;
        a.arg[(int64_t)b * a.C + fc] = none ? -1 : r;
      }
      if (FINAL) {
        for (int j = 0; j < a.J; ++j) {
          float s = 0.f;
          for (int g = 0; g < EP_GROUPS; ++g) s += s_sum[g][j * EP_TILE + col];
          a.fsum[(int64_t)b * a.J * a.C + (int64_t)j * a.C + fc] = s;
          a.out[(int64_t)b * a.ldo + (int64_t)j * a.C + fc] = fmaxf(s, 0.f);
        }
      }
    }
  }
}

// (A capacity batch needs no form of its own: its padding rows have cluster_of = -1, zero coef and a valid row_graph, and win no readout.)
// dZ[r, f] = sum_j u_j(r) dX'[cluster(r), j*C + f]  (+ dro[b, f] where r won graph b's readout).  One thread per (row, 4 columns);
// ghost rows: 0 (ghost_mode 1: the caller discards them) or the readout gradient of the graphs they won (ghost_mode 2, summed
// over b in order).  FINAL: dX' is the gradient of out = max(s, 0), passed where s >= 0 (torch.max's first index: row 0 on a tie).
struct EpBwd {
  const float* dxp; int64_t lddxp;        // non-final: [n_rows1 + nmax, J*C]; final: [B, J*C] (readout columns)
  const float* fsum;                      // final: s [B, J*C]
  const int* cluster_of; const int* row_graph; const float* coef; int J; int C;
  const float* dro; int64_t lddro; const int* arg;   // nullable
  int64_t n_rows0; int nmax; int ghost_mode; int B;
  float* dz; int64_t lddz; int64_t rows_total;
};

template <bool FINAL>
__global__ __launch_bounds__(256) void eigen_pool_bwd(EpBwd a) {
  const int C4 = (a.C + 3) / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.rows_total * C4) return;
  const int64_t r = i / C4;
  const int f0 = 4 * (int)(i - r * C4);
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  if (r < a.n_rows0) {
    const int b = a.row_graph[r];
    const int c = FINAL ? b : a.cluster_of[r];
    if (c >= 0) {
      for (int j = 0; j < a.J; ++j) {
        const float u = a.coef[r * a.J + j];
        const float* g = a.dxp + (int64_t)c * a.lddxp + (int64_t)j * a.C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (f0 + k < a.C) {
            float gv = g[f0 + k];
            if (FINAL && !(a.fsum[(int64_t)c * a.J * a.C + (int64_t)j * a.C + f0 + k] >= 0.f)) gv = 0.f;
            d[k] = fmaf(u, gv, d[k]);
          }
        }
      }
    }
    if (a.dro) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (f0 + k < a.C && a.arg[(int64_t)b * a.C + f0 + k] == (int)r) d[k] += a.dro[(int64_t)b * a.lddro + f0 + k];
    }
  } else if (a.dro && a.ghost_mode == 2) {
    for (int b = 0; b < a.B; ++b)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (f0 + k < a.C && a.arg[(int64_t)b * a.C + f0 + k] == (int)r) d[k] += a.dro[(int64_t)b * a.lddro + f0 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (f0 + k < a.C) a.dz[r * a.lddz + f0 + k] = d[k];
}

// dense padded pooling matrices -> compact form.  One wave per real row r (graph b, slot v): the first column c with a non-zero
// entry in any of the J matrices is the row's cluster (cluster_of = gp1[b] + c, or -1 when all J entries are zero: such a row
// adds nothing to the dense product either), coef[r, j] = P_j[b, v, c].  final: the column is 0 and cluster_of = b.
// key (non-final, nullable): the row's bucket, gp1[b] + b for an unassigned row, cluster_of + b + 1 otherwise — grouped by
// tsgnn_coo_count / tsgnn_coo_fill (rows ascending inside a bucket), the buckets of graph b are its unassigned rows, then its
// clusters in order.  bad: a column outside the graph's K_b clusters (set to 1).
__global__ __launch_bounds__(256) void eigen_pool_from_dense(const float* __restrict__ P, int J, int B, int nmax, const int* __restrict__ row_graph,
                                                             const int* __restrict__ row_slot, const int* __restrict__ gp1, int64_t n_rows,
                                                             int final_level, int* __restrict__ cluster_of, float* __restrict__ coef,
                                                             int64_t* __restrict__ key, int* __restrict__ bad) {
  const int64_t r = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (r >= n_rows) return;
  const int b = row_graph[r], v = row_slot[r];
  const int64_t mat = (int64_t)B * nmax * nmax;
  const float* row = P + ((int64_t)b * nmax + v) * nmax;
  int c = -1;
  if (final_level) {
    c = 0;
  } else {
    for (int c0 = 0; c0 < nmax && c < 0; c0 += 64) {
      bool nz = false;
      if (c0 + lane < nmax)
        for (int j = 0; j < J; ++j) nz |= row[j * mat + c0 + lane] != 0.f;
      const unsigned long long m = __ballot(nz);
      if (m) c = c0 + __builtin_ctzll(m);
    }
  }
  if (lane < J) coef[r * J + lane] = c >= 0 ? row[lane * mat + c] : 0.f;
  if (lane == 0) {
    if (final_level) {
      cluster_of[r] = b;
    } else {
      if (c >= gp1[b + 1] - gp1[b]) {
        bad[0] = 1;
        c = -1;
      }
      cluster_of[r] = c >= 0 ? gp1[b] + c : -1;
      if (key) key[r] = c >= 0 ? (int64_t)gp1[b] + c + b + 1 : (int64_t)gp1[b] + b;
    }
  }
}

}  // namespace

// both forms of the forward launch (cap: tsgnn_eigen_pool_fwd_cap_f32)
static int ep_fwd_launch(const float* z, int64_t ldz, int C, const int* graph_ptr0, int B, int nmax, int64_t n_rows0,
                         int ghost_mode, const int* graph_ptr1, const int* bptr, const int* members, const float* coef, int J,
                         int final_level, float* out, int64_t ldo, int64_t n_rows1, int n_ghost1, float* fsum, float* ro,
                         int64_t ldro, int* arg, bool cap, tsgnn_stream_t stream) {
  if (!z || !graph_ptr0 || !coef || !out || B <= 0 || nmax <= 0 || C <= 0 || J < 1 || J > EP_JMAX || ldz < C ||
      ghost_mode < 0 || ghost_mode > 2 || (ro && (!arg || ldro < C)) || n_rows0 < 0 || n_rows1 < 0 || n_ghost1 < 0)
    return TSGNN_EINVAL;
  if (cap && final_level) return TSGNN_EINVAL;
  if (final_level ? (!fsum || ldo < (int64_t)J * C) : (!graph_ptr1 || !bptr || !members || ldo < (int64_t)J * C))
    return TSGNN_EINVAL;
  EpFwd a{z, ldz, C, graph_ptr0, n_rows0, nmax, ghost_mode, graph_ptr1, bptr, members, coef, J, out, ldo, n_rows1, n_ghost1, fsum,
          ro, ldro, arg, B};
  const bool v4 = C % 4 == 0 && ldz % 4 == 0 && ldo % 4 == 0 && (uintptr_t)z % 16 == 0 && (uintptr_t)out % 16 == 0;
  dim3 grid((unsigned)B, (unsigned)ceil_div64(C, EP_TILE));
  if (final_level) {
    if (v4) eigen_pool_fwd<true, true><<<grid, 256, 0, stream>>>(a);
    else eigen_pool_fwd<true, false><<<grid, 256, 0, stream>>>(a);
    TSGNN_KNAME("eigen_pool_fwd<final,%d>", (int)v4);
  } else {
    if (cap) {
      if (v4) eigen_pool_fwd<false, true, true><<<grid, 256, 0, stream>>>(a);
      else eigen_pool_fwd<false, false, true><<<grid, 256, 0, stream>>>(a);
      TSGNN_KNAME("eigen_pool_fwd<pooled,%d,cap>", (int)v4);
    } else {
      if (v4) eigen_pool_fwd<false, true><<<grid, 256, 0, stream>>>(a);
      else eigen_pool_fwd<false, false><<<grid, 256, 0, stream>>>(a);
      TSGNN_KNAME("eigen_pool_fwd<pooled,%d>", (int)v4);
    }
  }
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

extern "C" {

int tsgnn_eigen_pool_fwd_f32(const float* z, int64_t ldz, int C, const int* graph_ptr0, int B, int nmax, int64_t n_rows0,
                             int ghost_mode, const int* graph_ptr1, const int* bptr, const int* members, const float* coef, int J,
                             int final_level, float* out, int64_t ldo, int64_t n_rows1, int n_ghost1, float* fsum, float* ro,
                             int64_t ldro, int* arg, tsgnn_stream_t stream) {
  return ep_fwd_launch(z, ldz, C, graph_ptr0, B, nmax, n_rows0, ghost_mode, graph_ptr1, bptr, members, coef, J, final_level, out, ldo,
                       n_rows1, n_ghost1, fsum, ro, ldro, arg, false, stream);
}

int tsgnn_eigen_pool_fwd_cap_f32(const float* z, int64_t ldz, int C, const int* graph_ptr0, int B, int nmax, int64_t n_rows0,
                                 int ghost_mode, const int* graph_ptr1, const int* bptr, const int* members, const float* coef, int J,
                                 int final_level, float* out, int64_t ldo, int64_t n_rows1, int n_ghost1, float* fsum, float* ro,
                                 int64_t ldro, int* arg, tsgnn_stream_t stream) {
  return ep_fwd_launch(z, ldz, C, graph_ptr0, B, nmax, n_rows0, ghost_mode, graph_ptr1, bptr, members, coef, J, final_level, out, ldo,
                       n_rows1, n_ghost1, fsum, ro, ldro, arg, true, stream);
}

int tsgnn_eigen_pool_bwd_f32(const float* dxp, int64_t lddxp, const float* fsum, const int* cluster_of, const int* row_graph,
                             const float* coef, int J, int C, const float* dro, int64_t lddro, const int* arg, int B, int nmax,
                             int64_t n_rows0, int ghost_mode, int final_level, float* dz, int64_t lddz, int64_t rows_total,
                             tsgnn_stream_t stream) {
  if (!dxp || !row_graph || !coef || !dz || B <= 0 || nmax <= 0 || C <= 0 || J < 1 || J > EP_JMAX || lddz < C ||
      lddxp < (int64_t)J * C || (dro && (!arg || lddro < C)) || rows_total < n_rows0 || n_rows0 < 0 ||
      (final_level ? !fsum : !cluster_of))
    return TSGNN_EINVAL;
  EpBwd a{dxp, lddxp, fsum, cluster_of, row_graph, coef, J, C, dro, lddro, arg, n_rows0, nmax, ghost_mode, B, dz, lddz, rows_total};
  const int64_t n = rows_total * ((C + 3) / 4);
  if (n == 0) return TSGNN_OK;
  if (final_level) eigen_pool_bwd<true><<<(unsigned)ceil_div64(n, 256), 256, 0, stream>>>(a);
  else eigen_pool_bwd<false><<<(unsigned)ceil_div64(n, 256), 256, 0, stream>>>(a);
  TSGNN_KNAME("eigen_pool_bwd<%s>", final_level ? "final" : "pooled");
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_eigen_pool_from_dense_f32(const float* P, int J, int B, int nmax, const int* row_graph, const int* row_slot,
                                    const int* graph_ptr1, int64_t n_rows, int final_level, int* cluster_of, float* coef, int64_t* key,
                                    int* bad, tsgnn_stream_t stream) {
  if (!P || !row_graph || !row_slot || !cluster_of || !coef || !bad || J < 1 || J > EP_JMAX || B <= 0 || nmax <= 0 ||
      n_rows < 0 || (!final_level && !graph_ptr1))
    return TSGNN_EINVAL;
  if (n_rows == 0) return TSGNN_OK;
  eigen_pool_from_dense<<<(unsigned)ceil_div64(n_rows, 4), 256, 0, stream>>>(P, J, B, nmax, row_graph, row_slot, graph_ptr1, n_rows,
                                                                            final_level, cluster_of, coef, key, bad);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
