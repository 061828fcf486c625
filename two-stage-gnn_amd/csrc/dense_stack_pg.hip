// GCN layers of a pooled DiffPool level (encoders.py:378-380 -> gcn_forward :140-167 on the dense, differentiable adjacency
// A' = S^T A S of :375) under PER-GRAPH statistics: the triplet step and stage two of the two-stage scheme, where every graph
// is normalised as if it were alone in its batch (tripletnet.py:36-38 calls the encoder at B = 1).
//
// BatchNorm1d(K) on a [1, K, F] tensor is a layer norm of every row over its features, so every post-op of a layer is row-local
// and the only thing that couples rows is the product with the adjacency.  A layer is therefore ONE launch with no
// synchronisation between workgroups (csrc/dense_stack.hip needs device-wide spin barriers only because the slot batch-norm
// couples graphs), and the launch boundary between two layers is the only barrier of the stack:
//   forward, per layer :  agg = A_b[rows] x_b,  u = agg W + b,  v = u / max(|u|, 1e-12),  y = LN(ReLU(v)) (hidden) | v (last)
//   backward, per layer:  dy = dcat[:, off : off + n] + (A_b[:, rows])^T dagg_{l+1}   (the input gradient of the layer above, formed
//                         as this launch's prologue from what the previous launch wrote),  dy -> dv -> du,  dagg = du W^T,  the
//                         tile's slab partial of (dW, db),  dA_b[rows] (+)= dagg xin_b^T
//   tsgnn_dense_pg_dx_f32: dx_b[rows] = (A_b[:, rows])^T dagg_0
// One workgroup (1,024 threads) owns one 16-row tile of one graph: grid = B * ceil(K / 16); rows past K of a graph's last tile are
// masked.  The same workgroup owns the same rows of dA in every layer's launch: accumulation needs no atomics, the first launch
// stores.  Weight gradients leave as one slab [fin + 1][n] per workgroup (row fin = the bias partial) for the fixed-order
// reduction tsgnn_wgrad_reduce_sets_f32.  No atomics, no arrival words, nothing to hang on.
//
// Every product is a 16-row tile on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate) with both operands in LDS: the 16-row side
// whole, the other side staged from global memory in chunks of as many rows of the sum as fit PG_BS floats.  Every thread requests
// all its loads of a stage before it waits for the first (registers, then LDS), the next chunk — or the next product's first — is in
// flight while the current one is multiplied.  The grid is a few dozen workgroups, each alone on its compute unit, and what bounds a
// launch is the serial work of a wave, not the round trips: with four waves per workgroup batching and prefetching the loads moved
// nothing (K 100, fin 192, n 64: forward 17.4 us, backward 29.7 us either way), sixteen waves — a row per wave in the row-local
// passes, one or two column tiles per wave in a product — brought 13.8 / 22.0 us (profiles/r14/diffpool_triplet.txt).
//
// Envelope (tsgnn_dense_pg_supported): 4 <= K <= 128, 4 <= fin <= 384, 4 <= n <= 128, all multiples of 4.  LDS at the largest
// shape: 16 * (132 + 2 * 388 + 132) + 16384 floats = 129 KB (backward).
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

#ifndef TSGNN_PG_THREADS
#define TSGNN_PG_THREADS 1024
#endif
constexpr int PG_NT = TSGNN_PG_THREADS;   // 16 waves: a row of the tile per wave in the row-local passes, one or two column tiles per wave in a product
constexpr int PG_NW = PG_NT / 64;
constexpr int PG_RPW = 16 / PG_NW;        // rows of the tile per wave
static_assert(PG_NT == 256 || PG_NT == 512 || PG_NT == 1024, "16 rows over 4, 8 or 16 waves");
constexpr int PG_BS = 16384;              // floats of the staging buffer of the streamed operand
constexpr int PG_STG = PG_BS / 4 / PG_NT; // float4 a thread carries per staged chunk
constexpr int PG_MAXT = (384 / 16 + PG_NW - 1) / PG_NW;     // 16-column tiles per wave at the widest shape
constexpr int PG_KMAX = 128, PG_FMAX = 384, PG_NMAX = 128;
constexpr float PG_NORM_EPS = 1e-12f;     // F.normalize
constexpr float PG_BN_EPS = 1e-5f;

typedef float pg_f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int pg_pad16(int n) { return (n + 15) & ~15; }
// LDS row strides: the 16-row operands [16][w] (rows on lanes & 15), the streamed operand [kc][w] (columns on lanes & 15: 16 mod 32
// keeps the four rows of one MFMA step on different banks)
__host__ __device__ inline int pg_ld_rows(int w) { return pg_pad16(w) + 4; }
__host__ __device__ inline int pg_ld_stream(int w) { const int p = pg_pad16(w); return (p & 16) ? p : p + 16; }

// A chunk of the streamed operand, rows [k0, k0 + kc) of the sum.  Element e: !BT: (k, j) = (e / n4, 4 (e % n4)), four columns of one row
// of the sum; BT: (j, k) = (e / k4, 4 (e % k4)), four rows of the sum of one column.  kc * ldbs <= PG_BS, so a chunk has at most
// PG_STG * PG_NT elements.  pg_fetch requests every load of the thread; pg_stash writes them to LDS (and waits for them there).
template <bool BT>
__device__ __forceinline__ void pg_fetch(float4 (&stg)[PG_STG], const float* __restrict__ bg, int64_t ldb, int Kd, int N, int NP, int k0, int kc) {
  const int per = BT ? kc >> 2 : NP >> 2, total = BT ? NP * per : kc * per;
#pragma unroll
  for (int u = 0; u < PG_STG; ++u) {
    const int e = threadIdx.x + u * PG_NT;
    const int q = e / per, r4 = (e - q * per) * 4;
    const int k = BT ? r4 : q, j = BT ? q : r4;
    const bool ok = e < total && k0 + k < Kd && j < N;
    const float* src = BT ? bg + (int64_t)j * ldb + k0 + k : bg + (int64_t)(k0 + k) * ldb + j;
    stg[u] = ok ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
template <bool BT>
__device__ __forceinline__ void pg_stash(const float4 (&stg)[PG_STG], float* bs, int ldbs, int NP, int kc) {
  const int per = BT ? kc >> 2 : NP >> 2, total = BT ? NP * per : kc * per;
#pragma unroll
  for (int u = 0; u < PG_STG; ++u) {
    const int e = threadIdx.x + u * PG_NT;
    if (e < total) {
      const int q = e / per, r4 = (e - q * per) * 4;
      if (!BT) {
        *reinterpret_cast<float4*>(bs + q * ldbs + r4) = stg[u];
      } else {
        bs[(r4 + 0) * ldbs + q] = stg[u].x; bs[(r4 + 1) * ldbs + q] = stg[u].y; bs[(r4 + 2) * ldbs + q] = stg[u].z; bs[(r4 + 3) * ldbs + q] = stg[u].w;
      }
    }
  }
}

// rows of the sum the first chunk of a product covers
__device__ __forceinline__ int pg_kc0(int Kd, int N) {
  const int KdP = pg_pad16(Kd), KC = (PG_BS / pg_ld_stream(N)) & ~15;
  return KC < KdP ? KC : KdP;
}
// requests the first chunk of a product: a kernel calls it as early as the operand exists — with the loads of the stage before it,
// or (the `next` of pg_product) under the last chunk of the product before it
template <bool BT>
__device__ __forceinline__ void pg_fetch0(float4 (&stg)[PG_STG], const float* __restrict__ bg, int64_t ldb, int Kd, int N) {
  pg_fetch<BT>(stg, bg, ldb, Kd, N, pg_pad16(N), 0, pg_kc0(Kd, N));
}
struct PgNone { __device__ __forceinline__ void operator()() const {} };

// cs[16][pad16(N)] = as[16][Kd] . Bm[Kd][N].  as: LDS, as[i * lda + k], zero for k in [Kd, pad16(Kd)).  Bm from global memory through
// the staging buffer bs: Bm(k, j) = BT ? bg[j * ldb + k] : bg[k * ldb + j] (16-byte aligned rows; Kd, N multiples of 4).  Columns
// [N, pad16(N)) of cs come out zero.  Starts and ends with a workgroup barrier.
// TPW: 16-column tiles per wave, ceil(ntile / PG_NW); a wave whose last tile does not exist multiplies the tile before it again and drops it.
// The product's first chunk is already on its way in stg (pg_fetch0); next() runs when stg is free again, under the last chunk.
template <bool BT, int TPW, class Next>
__device__ __forceinline__ void pg_product_t(float4 (&stg)[PG_STG], const float* as, int lda, const float* __restrict__ bg, int64_t ldb, int Kd, int N,
                                             float* bs, float* cs, int ldc, const Next& next) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
  const int NP = pg_pad16(N), ldbs = pg_ld_stream(N), ntile = NP >> 4, KdP = pg_pad16(Kd);
  const int KC = pg_kc0(Kd, N);
  pg_f32x4 acc[TPW];
  int col[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    acc[t] = pg_f32x4{0.f, 0.f, 0.f, 0.f};
    const int ct = wave + PG_NW * t;
    col[t] = (ct < ntile ? ct : ntile - 1) * 16;
  }
  for (int k0 = 0; k0 < KdP; k0 += KC) {
    const int kc = KC < KdP - k0 ? KC : KdP - k0;
    __syncthreads();                                     // the last chunk has been read (first pass: `as` is complete)
    pg_stash<BT>(stg, bs, ldbs, NP, kc);
    __syncthreads();
    if (k0 + KC < KdP) pg_fetch<BT>(stg, bg, ldb, Kd, N, NP, k0 + KC, KC < KdP - k0 - KC ? KC : KdP - k0 - KC);   // in flight while this chunk is multiplied
    else next();
    for (int kk = 0; kk < kc; kk += 16) {                 // (kc is a multiple of 16)
#pragma unroll
      for (int s4 = 0; s4 < 16; s4 += 4) {
        const float af = as[li * lda + k0 + kk + s4 + lq];       // A[i = lane & 15][k = lane >> 4]
        const float* brow = bs + (kk + s4 + lq) * ldbs + li;     // B[k = lane >> 4][j = lane & 15]
#pragma unroll
        for (int t = 0; t < TPW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, brow[col[t]], acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    if (wave + PG_NW * t < ntile) {
#pragma unroll
      for (int r = 0; r < 4; ++r) cs[(lq * 4 + r) * ldc + col[t] + li] = acc[t][r];       // C: row = (lane >> 4) * 4 + r, col = lane & 15
    }
  }
  __syncthreads();
}

template <bool BT, class Next>
__device__ __forceinline__ void pg_product(float4 (&stg)[PG_STG], const float* as, int lda, const float* __restrict__ bg, int64_t ldb, int Kd, int N,
                                           float* bs, float* cs, int ldc, const Next& next) {
  switch (((pg_pad16(N) >> 4) + PG_NW - 1) / PG_NW) {
    case 1: pg_product_t<BT, 1>(stg, as, lda, bg, ldb, Kd, N, bs, cs, ldc, next); break;
    case 2: if constexpr (PG_MAXT > 2) { pg_product_t<BT, 2>(stg, as, lda, bg, ldb, Kd, N, bs, cs, ldc, next); break; }
    case 3: if constexpr (PG_MAXT > 3) { pg_product_t<BT, 3>(stg, as, lda, bg, ldb, Kd, N, bs, cs, ldc, next); break; }
    case 4: if constexpr (PG_MAXT > 4) { pg_product_t<BT, 4>(stg, as, lda, bg, ldb, Kd, N, bs, cs, ldc, next); break; }
    case 5: if constexpr (PG_MAXT > 5) { pg_product_t<BT, 5>(stg, as, lda, bg, ldb, Kd, N, bs, cs, ldc, next); break; }
    default: pg_product_t<BT, PG_MAXT>(stg, as, lda, bg, ldb, Kd, N, bs, cs, ldc, next); break;
  }
}

// the 16 x pad16(K) tile of the adjacency of graph b the workgroup multiplies with: its rows [r0, r0 + 16) (trans = 0) or, for the
// products with A^T, its columns: at[i][k] = A_b[k][r0 + i].  Zero outside the graph.  Loads and LDS stores apart, so that the loads
// travel with the others of the kernel's first stage.
constexpr int PG_ADJ = 16 * PG_KMAX / PG_NT;
constexpr int PG_AGG = (16 * PG_FMAX / 4 + PG_NT - 1) / PG_NT;    // float4 of the agg tile per thread
__device__ __forceinline__ void pg_adj_load(const float* __restrict__ adj_b, int K, int r0, bool trans, float (&v)[PG_ADJ]) {
  const int KP = pg_pad16(K);
#pragma unroll
  for (int u = 0; u < PG_ADJ; ++u) {
    const int e = threadIdx.x + u * PG_NT;
    const int i = trans ? e & 15 : e / KP, k = trans ? e >> 4 : e - (e / KP) * KP;       // trans: 16 lanes read 64 contiguous bytes of row k
    v[u] = (e < 16 * KP && r0 + i < K && k < K) ? (trans ? adj_b[(int64_t)k * K + r0 + i] : adj_b[(int64_t)(r0 + i) * K + k]) : 0.f;
  }
}
__device__ __forceinline__ void pg_adj_store(const float (&v)[PG_ADJ], int K, bool trans, float* at, int lda) {
  const int KP = pg_pad16(K);
#pragma unroll
  for (int u = 0; u < PG_ADJ; ++u) {
    const int e = threadIdx.x + u * PG_NT;
    const int i = trans ? e & 15 : e / KP, k = trans ? e >> 4 : e - (e / KP) * KP;
    if (e < 16 * KP) at[i * lda + k] = v[u];
  }
}

struct PgFwd {
  const float* x; int64_t ldx; const float* adj; const float* w; int64_t ldw; const float* bias;
  int B, K, fin, n, hidden;
  float* agg; float* v; float* rinv; float* mean; float* rstd; float* y; int64_t ldy;
};

__global__ __launch_bounds__(PG_NT) void dense_pg_fwd_kernel(PgFwd a) {
  extern __shared__ __attribute__((aligned(16))) float pg_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = (a.K + 15) >> 4, b = blockIdx.x / tiles, r0 = (blockIdx.x - b * tiles) * 16;
  const int ldA = pg_ld_rows(a.K), ldG = pg_ld_rows(a.fin), ldU = pg_ld_rows(a.n);
  float* As = pg_smem;
  float* aggs = As + 16 * ldA;
  float* us = aggs + 16 * ldG;
  float* bs = us + 16 * ldU;
  const int64_t row0 = (int64_t)b * a.K;
  float4 stg[PG_STG];
  float av[PG_ADJ];
  pg_adj_load(a.adj + row0 * a.K, a.K, r0, false, av);                                         // one round trip: the adjacency tile and the
  pg_fetch0<false>(stg, a.x + row0 * a.ldx, a.ldx, a.K, a.fin);                                // first rows of x_b
  pg_adj_store(av, a.K, false, As, ldA);
  pg_product<false>(stg, As, ldA, a.x + row0 * a.ldx, a.ldx, a.K, a.fin, bs, aggs, ldG,        // agg = A_b[rows] . x_b
                    [&]() { pg_fetch0<false>(stg, a.w, a.ldw, a.fin, a.n); });                 // (W arrives under its last chunk)
  const int f4 = a.agg ? a.fin >> 2 : 0;                 // (agg, v, rinv, mean, rstd: what the backward reads; NULL in a forward-only call)
  for (int e = tid; e < 16 * f4; e += PG_NT) {
    const int i = e / f4, j = (e - i * f4) * 4;
    if (r0 + i < a.K) *reinterpret_cast<float4*>(a.agg + (row0 + r0 + i) * a.fin + j) = *reinterpret_cast<const float4*>(aggs + i * ldG + j);
  }
  pg_product<false>(stg, aggs, ldG, a.w, a.ldw, a.fin, a.n, bs, us, ldU, PgNone());            // u = agg . W
  // row-local tail: one wave per row, features lane and lane + 64
  for (int q = 0; q < PG_RPW; ++q) {
    const int i = wave * PG_RPW + q;
    const int64_t row = row0 + r0 + i;
    const bool live = r0 + i < a.K;
    float u[2], vv[2], yy[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int f = lane + 64 * c;
      u[c] = f < a.n ? us[i * ldU + f] + (a.bias ? a.bias[f] : 0.f) : 0.f;
    }
    const float ri = 1.0f / fmaxf(sqrtf(wave_sum(fmaf(u[0], u[0], u[1] * u[1]))), PG_NORM_EPS);
    vv[0] = u[0] * ri; vv[1] = u[1] * ri;
    float mu = 0.f, rs = 0.f;
    if (a.hidden) {
      const float p0 = fmaxf(vv[0], 0.f), p1 = fmaxf(vv[1], 0.f);
      mu = wave_sum(p0 + p1) / (float)a.n;
      const float d0 = lane < a.n ? p0 - mu : 0.f, d1 = lane + 64 < a.n ? p1 - mu : 0.f;
      rs = 1.0f / sqrtf(wave_sum(fmaf(d0, d0, d1 * d1)) / (float)a.n + PG_BN_EPS);
      yy[0] = d0 * rs; yy[1] = d1 * rs;
    } else {
      yy[0] = vv[0]; yy[1] = vv[1];
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int f = lane + 64 * c;
        if (f < a.n) {
          if (a.hidden && a.v) a.v[row * a.n + f] = vv[c];
          st_out(a.y + row * a.ldy + f, yy[c]);          // the next layer's launch reads it
        }
      }
      if (lane == 0) {
        if (a.rinv) a.rinv[row] = ri;
        if (a.hidden && a.mean && a.rstd) { a.mean[row] = mu; a.rstd[row] = rs; }
      }
    }
  }
}

struct PgBwd {
  const float* adj; const float* w; int64_t ldw; const float* agg; const float* v; int64_t ldv; const float* rinv; const float* mean;
  const float* rstd; const float* xin; int64_t ldx; const float* dcat; int64_t lddc; const float* dagg_next;
  int B, K, fin, n, hidden;
  float* dagg; float* slab; float* dadj; int accumulate;
};

__global__ __launch_bounds__(PG_NT) void dense_pg_bwd_kernel(PgBwd a) {
  extern __shared__ __attribute__((aligned(16))) float pg_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
  const int tiles = (a.K + 15) >> 4, b = blockIdx.x / tiles, r0 = (blockIdx.x - b * tiles) * 16;
  const int ldA = pg_ld_rows(a.K), ldG = pg_ld_rows(a.fin), ldU = pg_ld_rows(a.n);
  float* At = pg_smem;                     // A_b[:, rows]^T, later the tile of dA
  float* aggs = At + 16 * ldA;
  float* daggs = aggs + 16 * ldG;
  float* dus = daggs + 16 * ldG;           // the layer above's input gradient, then du
  float* bs = dus + 16 * ldU;
  const int64_t row0 = (int64_t)b * a.K;
  const int nP = pg_pad16(a.n), finP = pg_pad16(a.fin);
  const bool want_dagg = a.dagg || a.dadj;
  // the kernel's first round trip: everything that does not depend on a product — the rows of dcat and v and their statistics, the agg
  // rows, the adjacency tile and the first chunk of the first product
  float4 stg[PG_STG];
  float av[PG_ADJ];
  if (a.dagg_next) {
    pg_adj_load(a.adj + row0 * a.K, a.K, r0, true, av);
    pg_fetch0<false>(stg, a.dagg_next + row0 * a.n, a.n, a.K, a.n);
  } else if (want_dagg) {
    pg_fetch0<true>(stg, a.w, a.ldw, a.n, a.fin);
  }
  float dy4[PG_RPW][2], vv4[PG_RPW][2], mu4[PG_RPW], rs4[PG_RPW], ri4[PG_RPW];
#pragma unroll
  for (int q = 0; q < PG_RPW; ++q) {                          // the four rows' loads requested together
    const int i = wave * PG_RPW + q;
    const int64_t row = row0 + r0 + i;
    const bool live = r0 + i < a.K;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int f = lane + 64 * c;
      const bool ok = live && f < a.n;
      dy4[q][c] = ok ? a.dcat[row * a.lddc + f] : 0.f;
      vv4[q][c] = ok ? a.v[row * a.ldv + f] : 0.f;
    }
    mu4[q] = (live && a.hidden) ? a.mean[row] : 0.f;
    rs4[q] = (live && a.hidden) ? a.rstd[row] : 0.f;
    ri4[q] = live ? a.rinv[row] : 0.f;
  }
  float4 g[PG_AGG];
  if (a.slab) {
#pragma unroll
    for (int u = 0; u < PG_AGG; ++u) {
      const int e = tid + u * PG_NT, i = e / (finP >> 2), f = (e - i * (finP >> 2)) * 4;
      g[u] = (e < 4 * finP && r0 + i < a.K && f < a.fin) ? *reinterpret_cast<const float4*>(a.agg + (row0 + r0 + i) * a.fin + f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  if (a.dagg_next) {                                                                           // (A_b[:, rows])^T . dagg_{l+1}
    pg_adj_store(av, a.K, true, At, ldA);
    pg_product<false>(stg, At, ldA, a.dagg_next + row0 * a.n, a.n, a.K, a.n, bs, dus, ldU,
                      [&]() { if (want_dagg) pg_fetch0<true>(stg, a.w, a.ldw, a.n, a.fin); });
  }
  // dy -> dv (row layer norm + ReLU backward) -> du (L2-normalise backward): one wave per row, features lane and lane + 64
#pragma unroll
  for (int q = 0; q < PG_RPW; ++q) {
    const int i = wave * PG_RPW + q;
    const bool live = r0 + i < a.K;
    float dy[2], vv[2], dv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int f = lane + 64 * c;
      dy[c] = dy4[q][c] + ((a.dagg_next && live && f < a.n) ? dus[i * ldU + f] : 0.f);
      vv[c] = vv4[q][c];
    }
    if (a.hidden) {
      const float mu = mu4[q], rs = rs4[q];
      float xh[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) xh[c] = (live && lane + 64 * c < a.n) ? (fmaxf(vv[c], 0.f) - mu) * rs : 0.f;
      const float m1 = wave_sum(dy[0] + dy[1]) / (float)a.n;
      const float m2 = wave_sum(fmaf(dy[0], xh[0], dy[1] * xh[1])) / (float)a.n;
#pragma unroll
      for (int c = 0; c < 2; ++c) dv[c] = (vv[c] > 0.f) ? rs * (dy[c] - m1 - xh[c] * m2) : 0.f;
    } else {
      dv[0] = dy[0]; dv[1] = dy[1];
    }
    const float dot = wave_sum(fmaf(vv[0], dv[0], vv[1] * dv[1]));
    const float ri = ri4[q];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int f = lane + 64 * c;
      if (f < nP) dus[i * ldU + f] = (live && f < a.n) ? ri * (dv[c] - vv[c] * dot) : 0.f;
    }
  }
  if (a.slab) {                                                                                // agg rows, kept by the forward
#pragma unroll
    for (int u = 0; u < PG_AGG; ++u) {
      const int e = tid + u * PG_NT, i = e / (finP >> 2), f = (e - i * (finP >> 2)) * 4;
      if (e < 4 * finP) *reinterpret_cast<float4*>(aggs + i * ldG + f) = g[u];
    }
  }
  __syncthreads();
  if (want_dagg) {                                                                             // dagg = du . W^T
    pg_product<true>(stg, dus, ldU, a.w, a.ldw, a.n, a.fin, bs, daggs, ldG,
                     [&]() { if (a.dadj) pg_fetch0<true>(stg, a.xin + row0 * a.ldx, a.ldx, a.fin, a.K); });
    if (a.dagg)
      for (int e = tid; e < 16 * a.fin; e += PG_NT) {
        const int i = e / a.fin, f = e - i * a.fin;
        if (r0 + i < a.K) st_out(a.dagg + (row0 + r0 + i) * a.fin + f, daggs[i * ldG + f]);   // the next launch's prologue reads it
      }
  }
  if (a.slab) {                                                                                // this tile's partial of dW = agg^T du and of db
    float* slab = a.slab + (int64_t)blockIdx.x * (a.fin + 1) * a.n;
    const int ntn = nP >> 4, nt = (finP >> 4) * ntn;
    for (int t = wave; t < nt; t += PG_NT / 64) {
      const int tf = t / ntn, tn = t - tf * ntn;
      pg_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int rr = 4 * s + lq;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aggs[rr * ldG + tf * 16 + li], dus[rr * ldU + tn * 16 + li], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = tf * 16 + lq * 4 + r, j = tn * 16 + li;
        if (f < a.fin && j < a.n) st_out(slab + (int64_t)f * a.n + j, acc[r]);
      }
    }
    if (tid < a.n) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) s += dus[i * ldU + tid];
      st_out(slab + (int64_t)a.fin * a.n + tid, s);
    }
  }
  if (a.dadj) {                                                                                // dA_b[rows] (+)= dagg . xin_b^T
    pg_product<true>(stg, daggs, ldG, a.xin + row0 * a.ldx, a.ldx, a.fin, a.K, bs, At, ldA, PgNone());
    float old[16 * PG_KMAX / PG_NT];
#pragma unroll
    for (int u = 0; u < 16 * PG_KMAX / PG_NT; ++u) {
      const int e = tid + u * PG_NT, i = e / a.K, j = e - i * a.K;
      old[u] = (a.accumulate && e < 16 * a.K && r0 + i < a.K) ? a.dadj[(row0 + r0 + i) * a.K + j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 16 * PG_KMAX / PG_NT; ++u) {
      const int e = tid + u * PG_NT, i = e / a.K, j = e - i * a.K;
      if (e < 16 * a.K && r0 + i < a.K) a.dadj[(row0 + r0 + i) * a.K + j] = old[u] + At[i * ldA + j];
    }
  }
}

struct PgDx { const float* adj; const float* dagg; int B, K, fin; float* dx; int64_t lddx; };

__global__ __launch_bounds__(PG_NT) void dense_pg_dx_kernel(PgDx a) {
  extern __shared__ __attribute__((aligned(16))) float pg_smem[];
  const int tid = threadIdx.x;
  const int tiles = (a.K + 15) >> 4, b = blockIdx.x / tiles, r0 = (blockIdx.x - b * tiles) * 16;
  const int ldA = pg_ld_rows(a.K), ldG = pg_ld_rows(a.fin);
  float* At = pg_smem;
  float* cs = At + 16 * ldA;
  float* bs = cs + 16 * ldG;
  const int64_t row0 = (int64_t)b * a.K;
  float4 stg[PG_STG];
  float av[PG_ADJ];
  pg_adj_load(a.adj + row0 * a.K, a.K, r0, true, av);
  pg_fetch0<false>(stg, a.dagg + row0 * a.fin, a.fin, a.K, a.fin);
  pg_adj_store(av, a.K, true, At, ldA);
  pg_product<false>(stg, At, ldA, a.dagg + row0 * a.fin, a.fin, a.K, a.fin, bs, cs, ldG, PgNone());
  for (int e = tid; e < 16 * a.fin; e += PG_NT) {
    const int i = e / a.fin, f = e - i * a.fin;
    if (r0 + i < a.K) a.dx[(row0 + r0 + i) * a.lddx + f] = cs[i * ldG + f];
  }
}

size_t pg_lds_fwd(int K, int fin, int n) { return sizeof(float) * (16 * (pg_ld_rows(K) + pg_ld_rows(fin) + pg_ld_rows(n)) + PG_BS); }
size_t pg_lds_bwd(int K, int fin, int n) { return sizeof(float) * (16 * (pg_ld_rows(K) + 2 * pg_ld_rows(fin) + pg_ld_rows(n)) + PG_BS); }
size_t pg_lds_dx(int K, int fin) { return sizeof(float) * (16 * (pg_ld_rows(K) + pg_ld_rows(fin)) + PG_BS); }

// the kernels' dynamic-LDS limit, raised once per DEVICE (the attribute is per device) to what the largest shape of the envelope needs
bool pg_prepare() {
  static int done[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return false; }
  if (done[dev]) return done[dev] > 0;
  bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(dense_pg_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)pg_lds_fwd(PG_KMAX, PG_FMAX, PG_NMAX)) == hipSuccess;
  ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(dense_pg_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)pg_lds_bwd(PG_KMAX, PG_FMAX, PG_NMAX)) == hipSuccess;
  ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(dense_pg_dx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)pg_lds_dx(PG_KMAX, PG_FMAX)) == hipSuccess;
  if (!ok) (void)hipGetLastError();
  done[dev] = ok ? 1 : -1;
  return ok;
}

inline bool pg_mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool pg_shape_ok(int B, int K, int fin, int n) {
  return B >= 1 && (int64_t)B * ((K + 15) / 16) <= (1 << 20) && K >= 4 && K <= PG_KMAX && !(K % 4) && fin >= 4 && fin <= PG_FMAX && !(fin % 4) &&
         n >= 4 && n <= PG_NMAX && !(n % 4);
}

}  // namespace

extern "C" {

int tsgnn_dense_pg_supported(int B, int K, int fin, int n) { return pg_shape_ok(B, K, fin, n) ? 1 : 0; }

int tsgnn_dense_pg_layer_fwd_f32(const float* x, int64_t ldx, const float* adj, const float* w, int64_t ldw, const float* bias, int B, int K,
                                 int fin, int n, int hidden, float* agg, float* v, float* rinv, float* mean, float* rstd, float* y,
                                 int64_t ldy, tsgnn_stream_t stream) {
  if (!x || !adj || !w || !y || ((mean == nullptr) != (rstd == nullptr)) || B <= 0 || K <= 0 || fin <= 0 || n <= 0 ||
      ldx < fin || ldw < n || ldy < n)
    return TSGNN_EINVAL;
  if (!pg_shape_ok(B, K, fin, n) || (ldx % 4) || (ldw % 4) || pg_mis16(x) || pg_mis16(w) || (agg && pg_mis16(agg))) return TSGNN_EUNSUPPORTED;
  if (!pg_prepare()) return TSGNN_ELAUNCH;
  PgFwd a{x, ldx, adj, w, ldw, bias, B, K, fin, n, hidden ? 1 : 0, agg, v, rinv, mean, rstd, y, ldy};
  TSGNN_KNAME("dense_pg_fwd_kernel");
  dense_pg_fwd_kernel<<<(unsigned)(B * ((K + 15) / 16)), PG_NT, pg_lds_fwd(K, fin, n), stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_dense_pg_layer_bwd_f32(const float* adj, const float* w, int64_t ldw, const float* agg, const float* v, int64_t ldv,
                                 const float* rinv, const float* mean, const float* rstd, const float* xin, int64_t ldx, const float* dcat,
                                 int64_t lddc, const float* dagg_next, int B, int K, int fin, int n, int hidden, float* dagg, float* slab,
                                 float* dadj, int accumulate, tsgnn_stream_t stream) {
  if (!adj || !w || !v || !rinv || !dcat || (hidden && (!mean || !rstd)) || (slab && !agg) || (dadj && !xin) || B <= 0 || K <= 0 ||
      fin <= 0 || n <= 0 || ldw < n || ldv < n || lddc < n || (dadj && ldx < fin))
    return TSGNN_EINVAL;
  if (!pg_shape_ok(B, K, fin, n) || (ldw % 4) || pg_mis16(w) || (dagg_next && pg_mis16(dagg_next)) || (dadj && ((ldx % 4) || pg_mis16(xin))))
    return TSGNN_EUNSUPPORTED;
  if (!pg_prepare()) return TSGNN_ELAUNCH;
  PgBwd a{adj, w, ldw, agg, v, ldv, rinv, mean, rstd, xin, ldx, dcat, lddc, dagg_next, B, K, fin, n, hidden ? 1 : 0, dagg, slab, dadj,
          accumulate ? 1 : 0};
  TSGNN_KNAME("dense_pg_bwd_kernel");
  dense_pg_bwd_kernel<<<(unsigned)(B * ((K + 15) / 16)), PG_NT, pg_lds_bwd(K, fin, n), stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_dense_pg_dx_f32(const float* adj, const float* dagg, int B, int K, int fin, float* dx, int64_t lddx, tsgnn_stream_t stream) {
  if (!adj || !dagg || !dx || B <= 0 || K <= 0 || fin <= 0 || lddx < fin) return TSGNN_EINVAL;
  if (!pg_shape_ok(B, K, fin, 4) || pg_mis16(dagg)) return TSGNN_EUNSUPPORTED;
  if (!pg_prepare()) return TSGNN_ELAUNCH;
  PgDx a{adj, dagg, B, K, fin, dx, lddx};
  TSGNN_KNAME("dense_pg_dx_kernel");
  dense_pg_dx_kernel<<<(unsigned)(B * ((K + 15) / 16)), PG_NT, pg_lds_dx(K, fin), stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
