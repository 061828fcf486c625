// The row-tile bodies of the 2stg+ post-training "head" kernels (posttrain_cls.hip, posttrain_head.hip): a small MLP on R <= 8
// readout rows, one launch each way.  RT is the height of the row tile: R rounded up to 1, 2, 4 or 8.  Every body is called by ALL
// threads of the workgroup.
//   forward  (one workgroup of WAVES waves): rows_dense16 (16-byte weight rows), rows_dense1 (scalar weight rows)
//   backward (256 threads, a workgroup per 32 columns of r): rows_chain / rows_dh1 (the chain down to the first layer's gradient,
//             re-derived by every workgroup), rows_input_columns (its columns of dr and of the first dW), rows_outer_tail (its
//             grid-strided share of the small gradients)
// Tiles in LDS are [RT][n] at the row stride the caller names; the backward's are compact (row stride n) with zero rows past R, so
// every row loop has a compile-time length and the accumulators stay in registers.  Every output element has one writer and every
// sum a fixed order (rows 0 .. RT - 1, the partial sums of a column in order): two runs give the same bits.
// Every dot product here is an explicit fmaf chain, so a body gives its callers the bits their own loops gave.  (Not here for that
// reason: p3_dense, the 16-byte dense layer of posttrain_cls.hip's mlp3 head.  It adds  (wx ax + wy ay) + (wz az + ww aw)  and
// leaves the contraction into fused operations to the compiler, which decides it per instantiation.)
// The triplet tails (triplet.hip, mlp2_triplet.hip, the second half of mlp_head.hip) are the same loops at three rows and keep their
// own: through these bodies their replayed steps measured 0.3 to 3.8 us slower (profiles/r27/README.md).
// "rows past N: a mapped row, result dropped": a weight row index is clamped to N - 1 so that all RPW loads of a pass can be requested
// together without a branch; what such a row gives is never stored.
#pragma once
#include "common.h"

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float rows_leaky(float v, float slope) { return v > 0.f ? v : slope * v; }

// label of row i: labels[ids[i]], both clamped into their tables (the host validates what it can see; these live on the device)
__device__ __forceinline__ int row_label(const int* ids, const int* labels, int n_labels, int C, int i) {
  const int id = min(max(ids[i], 0), n_labels - 1);
  return min(max(labels[id], 0), C - 1);
}

// an input row's index.  Eight rows: kept in a vector register, so that the eight row addresses are formed per lane (as eight scalar
// pointers they do not fit the scalar registers beside the kernel's arguments and would be spilled)
template <int RT>
__device__ __forceinline__ int rows_row(int i) {
  if (RT == 8) asm volatile("" : "+v"(i));
  return i;
}

// vs[i][n] = act(W[n, :] . in_i + bias[n]) for i < RT, n < N, and out[i][n] (row stride N) for i < R where out is given.
// W [N, K] at row stride ldw, K % 4 == 0, 16-byte rows; in_i = in + min(i, rows - 1) * ldin, 16-byte rows in memory or LDS; vs in LDS
// at row stride ldv.  A wave takes RPW weight rows at a time, requested together, every weight row streamed once for all RT rows.
template <int RT, int RPW, int WAVES, bool RELU>
__device__ __forceinline__ void rows_dense16(const float* in, int64_t ldin, int rows, int K, const float* __restrict__ w, int64_t ldw,
                                             const float* __restrict__ bias, int N, float* vs, int ldv, float* __restrict__ out, int R) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int K4 = K >> 2;
  for (int n0 = wid * RPW; n0 < N; n0 += WAVES * RPW) {
    float s[RPW][RT];
#pragma unroll
    for (int j = 0; j < RPW; ++j)
#pragma unroll
      for (int i = 0; i < RT; ++i) s[j][i] = 0.f;
    for (int c = lane; c < K4; c += 64) {
      float4 wv[RPW];
#pragma unroll
      for (int j = 0; j < RPW; ++j) wv[j] = ld4(w + (int64_t)min(n0 + j, N - 1) * ldw + 4 * c);
#pragma unroll
      for (int i = 0; i < RT; ++i) {                                         // rows past `rows`: the last row again
        const float4 x = ld4(in + (int64_t)rows_row<RT>(min(i, rows - 1)) * ldin + 4 * c);
#pragma unroll
        for (int j = 0; j < RPW; ++j)
          s[j][i] = fmaf(wv[j].x, x.x, fmaf(wv[j].y, x.y, fmaf(wv[j].z, x.z, fmaf(wv[j].w, x.w, s[j][i]))));
      }
    }
    float bv[RPW];                                                           // requested together, ahead of the wave sums
#pragma unroll
    for (int j = 0; j < RPW; ++j) bv[j] = bias ? bias[min(n0 + j, N - 1)] : 0.f;
#pragma unroll
    for (int j = 0; j < RPW; ++j)
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float t = wave_sum(s[j][i]);
        const int n = n0 + j;
        if (lane == 0 && n < N) {
          const float z = t + bv[j];
          const float v = RELU ? fmaxf(z, 0.f) : z;
          vs[i * ldv + n] = v;
          if (out && i < R) out[i * N + n] = v;
        }
      }
  }
}

// the same for weight rows that are not 16-byte rows (W [N, K] dense): scalar loads, lanes along the row; in [RT][ldin] in LDS.  For
// i < R: the pre-activation z to zg[i][n] (row stride N) where zg is given, leaky(z) or z to vs[i][n]
template <int RT, int RPW, int WAVES>
__device__ __forceinline__ void rows_dense1(const float* in, int ldin, int K, const float* __restrict__ w, const float* __restrict__ bias,
                                            int N, int R, bool leaky, float slope, float* __restrict__ zg, float* vs, int ldv) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int n0 = wid * RPW; n0 < N; n0 += WAVES * RPW) {
    float s[RPW][RT];
#pragma unroll
    for (int j = 0; j < RPW; ++j)
#pragma unroll
      for (int i = 0; i < RT; ++i) s[j][i] = 0.f;
    for (int k = lane; k < K; k += 64) {
      float wv[RPW];
#pragma unroll
      for (int j = 0; j < RPW; ++j) wv[j] = w[(int64_t)min(n0 + j, N - 1) * K + k];
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float x = in[i * ldin + k];
#pragma unroll
        for (int j = 0; j < RPW; ++j) s[j][i] = fmaf(wv[j], x, s[j][i]);
      }
    }
    float bv[RPW];                                                           // requested together, ahead of the wave sums
#pragma unroll
    for (int j = 0; j < RPW; ++j) bv[j] = bias ? bias[min(n0 + j, N - 1)] : 0.f;
#pragma unroll
    for (int j = 0; j < RPW; ++j)
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float t = wave_sum(s[j][i]);
        const int n = n0 + j;
        if (lane == 0 && n < N && i < R) {
          const float z = t + bv[j];
          if (zg) zg[i * N + n] = z;
          vs[i * ldv + n] = leaky ? rows_leaky(z, slope) : z;
        }
      }
  }
}

// out[i][n] = gate(i, n) * sum_q g[i][q] W[q, n]  for i < RT, n < N   (W [Q, N] row-major; g [RT][Q], act [RT][N], out [RT][N],
// part [RT][4][64] in LDS; gate = scale where act[i][n] > 0, else 0).  64 columns x 4 row lanes per pass.
template <int RT, int T>
__device__ __forceinline__ void rows_chain(const float* g, int Q, const float* __restrict__ W, int N, const float* act, float scale,
                                           float* out, float* part) {
  static_assert(T == 256, "64 columns x 4 row lanes");
  const int tid = threadIdx.x, j = tid & 63, k = tid >> 6;
  for (int n0 = 0; n0 < N; n0 += 64) {
    const int n = n0 + j;
    const int nc = n < N ? n : 0;
    float s[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) s[i] = 0.f;
#pragma unroll 8
    for (int q = k; q < Q; q += 4) {
      const float wv = W[(int64_t)q * N + nc];
#pragma unroll
      for (int i = 0; i < RT; ++i) s[i] = fmaf(g[i * Q + q], wv, s[i]);
    }
#pragma unroll
    for (int i = 0; i < RT; ++i) part[(i * 4 + k) * 64 + j] = s[i];
    __syncthreads();
    for (int t = tid; t < RT * 64; t += T) {
      const int i = t >> 6, jj = t & 63, nn = n0 + jj;
      if (nn < N) {
        const float v = (part[(i * 4 + 0) * 64 + jj] + part[(i * 4 + 1) * 64 + jj]) + (part[(i * 4 + 2) * 64 + jj] + part[(i * 4 + 3) * 64 + jj]);
        out[i * N + nn] = act[i * N + nn] > 0.f ? v * scale : 0.f;
      }
    }
    __syncthreads();
  }
}

// out[i][n] = (act[i][n] > 0) sum_q g[i][q] W[q, n]  for a W whose rows are short: threads along a row of W, eight rows requested
// together (W [Q, N] row-major; g [RT][Q], act and out [RT][N] in LDS)
template <int RT, int T>
__device__ __forceinline__ void rows_dh1(const float* g, int Q, const float* __restrict__ W, int N, const float* act, float* out) {
  for (int n = threadIdx.x; n < N; n += T) {
    float s[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) s[i] = 0.f;
    for (int q0 = 0; q0 < Q; q0 += 8) {
      float wv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) wv[u] = W[(int64_t)min(q0 + u, Q - 1) * N + n];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (q0 + u < Q) {
#pragma unroll
          for (int i = 0; i < RT; ++i) s[i] = fmaf(g[i * Q + q0 + u], wv[u], s[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < RT; ++i) out[i * N + n] = act[i * N + n] > 0.f ? s[i] : 0.f;
  }
}

// this workgroup's 32 columns [32 bx, 32 bx + 32) of r: dr = dz W, dW = dz^T r (W [N, D] at row stride ldw, dW at lddw; dz [RT][N] in
// LDS, zero rows past R; part [RT][8][32] in LDS).  Thread (j = tid & 31, k = tid >> 5): column j, rows k, k + 8, ... of W.
template <int RT, int T>
__device__ __forceinline__ void rows_input_columns(const float* __restrict__ r, int64_t ldr, int R, int D, const float* __restrict__ w,
                                                   int64_t ldw, int N, const float* dz, float* __restrict__ dr, int64_t lddr,
                                                   float* __restrict__ dw, int64_t lddw, float* part) {
  static_assert(T == 256, "32 columns x 8 row lanes");
  const int tid = threadIdx.x, j = tid & 31, k = tid >> 5;
  const int d = 32 * (int)blockIdx.x + j;
  const bool ok = d < D;
  const int dc = ok ? d : 0;
  float rv[RT], acc[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    rv[i] = (ok && i < R) ? r[(int64_t)i * ldr + d] : 0.f;
    acc[i] = 0.f;
  }
  for (int o0 = k; o0 < N; o0 += 64) {                                       // eight rows of W per pass, requested together
    float wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) wv[u] = w[(int64_t)min(o0 + 8 * u, N - 1) * ldw + dc];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int o = o0 + 8 * u;
      if (ok && o < N) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          const float gi = dz[i * N + o];
          acc[i] = fmaf(gi, wv[u], acc[i]);
          s = fmaf(gi, rv[i], s);
        }
        dw[(int64_t)o * lddw + d] = s;
      }
    }
  }
  if (dr) {
#pragma unroll
    for (int i = 0; i < RT; ++i) part[(i * 8 + k) * 32 + j] = acc[i];
    __syncthreads();
    for (int t = tid; t < RT * 32; t += T) {
      const int i = t >> 5, jj = t & 31, dd = 32 * (int)blockIdx.x + jj;
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) s += part[(i * 8 + q) * 32 + jj];
      if (i < R && dd < D) dr[(int64_t)i * lddr + dd] = s;
    }
  }
}

// this workgroup's grid-strided share of the small gradients of a three-layer head, dW2 | dW3 | db1 | db2 | db3 as one index range:
// dW2 [D2, D1] = dz2^T a1, dW3 [C, D2] = dlg^T a2, db = the column sums of dz1, dz2, dlg (all [RT][.] in LDS, zero rows past R; a bias
// gradient may be NULL).  A two-layer head is the case C = 0: dW2 | db1 | db2.
template <int RT, int T>
__device__ __forceinline__ void rows_outer_tail(const float* dz1, const float* dz2, const float* dlg, const float* a1s, const float* a2s,
                                                int D1, int D2, int C, float* dw2, float* dw3, float* db1, float* db2, float* db3) {
  const int n2 = D2 * D1, n3 = C * D2;
  const int total = n2 + n3 + D1 + D2 + C;
  const int tid = threadIdx.x;
  for (int idx = (int)blockIdx.x * T + tid; idx < total; idx += (int)gridDim.x * T) {
    float s = 0.f;
    if (idx < n2) {
      const int k = idx / D1, o = idx - k * D1;
#pragma unroll
      for (int i = 0; i < RT; ++i) s = fmaf(dz2[i * D2 + k], a1s[i * D1 + o], s);
      dw2[idx] = s;
    } else if (idx < n2 + n3) {
      const int t = idx - n2, c = t / D2, k = t - c * D2;
#pragma unroll
      for (int i = 0; i < RT; ++i) s = fmaf(dlg[i * C + c], a2s[i * D2 + k], s);
      dw3[t] = s;
    } else if (idx < n2 + n3 + D1) {
      const int o = idx - n2 - n3;
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dz1[i * D1 + o];
      if (db1) db1[o] = s;
    } else if (idx < n2 + n3 + D1 + D2) {
      const int k = idx - n2 - n3 - D1;
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dz2[i * D2 + k];
      if (db2) db2[k] = s;
    } else {
      const int c = idx - n2 - n3 - D1 - D2;
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dlg[i * C + c];
      if (db3) db3[c] = s;
    }
  }
}

// ---------------------------------------------------------------- host side: the RT instantiation of a launch
constexpr int ROWS_MAXR = 8;
inline int rt_of(int R) { return R <= 1 ? 1 : R <= 2 ? 2 : R <= 4 ? 4 : 8; }

// LDS above 64 KB, the kernel's few static words included, has to be asked for (R = 8 at the corner of posttrain_mlp3_nll's envelope:
// 120 KB of the 160 KB a workgroup may have on gfx950).  Asked ONCE per instantiation, for the most any call of it needs, at the first
// call that needs it; a refusal is remembered and every such call is TSGNN_EUNSUPPORTED before anything is launched.  A kernel without
// dynamic LDS never gets here.
constexpr int ROWS_MAX_DYN_LDS = 128 * 1024;
template <typename K>
inline bool rows_allow_lds(K kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, ROWS_MAX_DYN_LDS) == hipSuccess;
}

#define TSGNN_ROWS_LAUNCH(KERNEL, RT, GRID, BLOCK, LDS)                          \
  do {                                                                           \
    if ((LDS) + 1024 > 64 * 1024) {                                              \
      static const bool allowed_ = rows_allow_lds(KERNEL<RT>);                   \
      if (!allowed_) return TSGNN_EUNSUPPORTED;                                  \
    }                                                                            \
    KERNEL<RT><<<GRID, BLOCK, LDS, stream>>>(a);                                 \
  } while (0)

// KERNEL<rt_of(R)><<<GRID, BLOCK, LDS, stream>>>(a) under the name "KERNEL<rt>"
#define TSGNN_ROWS_DISPATCH(KERNEL, R, GRID, BLOCK, LDS)                         \
  do {                                                                           \
    const int rt_ = rt_of(R);                                                    \
    TSGNN_KNAME(#KERNEL "<%d>", rt_);                                            \
    if (rt_ == 1) TSGNN_ROWS_LAUNCH(KERNEL, 1, GRID, BLOCK, LDS);                \
    else if (rt_ == 2) TSGNN_ROWS_LAUNCH(KERNEL, 2, GRID, BLOCK, LDS);           \
    else if (rt_ == 4) TSGNN_ROWS_LAUNCH(KERNEL, 4, GRID, BLOCK, LDS);           \
    else TSGNN_ROWS_LAUNCH(KERNEL, 8, GRID, BLOCK, LDS);                         \
  } while (0)
