// Classification heads of the 2stg+ post-training step of the two families whose step is the "original" setting's at B = 1:
//   SAGPool  (Code/sag/train_triplet_pre_train.py:219-263 on network.py:48-53):  loss = F.nll_loss(model(data), data.y)
//       a1 = dropout(relu(lin1(r)))   a2 = relu(lin2(a1))   logp = log_softmax(lin3(a2))   loss = mean_i -logp[i, label_i]
//   EigenGCN (Code/eigengcn/train_triplet_pre_train.py:170-249 on encoders.py:377): loss = F.cross_entropy(pred_model(r), label)
//       h = relu(W1 r + b1)   z = W2 h + b2   p = softmax(z)   loss = mean_i (logsumexp(z_i) - z_i[label_i])
// on the readout rows r [R, .] of the step's graphs (R = 1 in the reference's loops, up to 8 here), label_i = labels[ids[i]] read on
// the device (ids: what the gather launch of a stream wrote), each in ONE launch forward and ONE backward.
//
// Forward: one workgroup.  A wave takes a few weight rows at a time (nn.Linear's [out, in] layout), 16-byte loads where the rows are
// 16-byte rows (all three layers of the SAGPool head, W1 of the EigenGCN head; its W2 rows are H floats, 50 in the reference's
// default: scalar loads, lanes along the row), every weight row streamed once for all R readout rows, the dot products closed with
// DPP wave sums.  Soft-max: one wave per row, lanes along the classes.
// Backward: a grid over slices of 32 columns of r; every workgroup re-derives the short chain from the logits' gradient down to the
// first layer's in LDS (cheaper than a launch of its own and a hand-off between workgroups), then owns its columns of dr and of dW1,
// the largest gradient, and a grid-strided share of the small ones.
// Every output element is written once, every sum runs in a fixed order (rows 0 .. R - 1, the partial sums of a column in order), no
// read-modify-write anywhere: two runs give the same bits.  Rows R .. RT - 1 of the LDS tiles repeat row R - 1 (forward) or hold
// zeros (backward), so the row loops have a compile-time length and the accumulators stay in registers.
// The loops are csrc/head_rows_body.h's bodies at RT = 1, 2, 4, 8: rows_dense16 / rows_dense1 (the EigenGCN head's two layers),
// rows_chain / rows_dh1, rows_input_columns, rows_outer_tail.  Two stay here: p3_dense, the SAGPool head's 16-byte dense layer,
// whose pairwise dot product  (wx ax + wy ay) + (wz az + ww aw)  is left to the compiler's contraction, so its bits belong to this
// very instantiation (as a call of a shared body the forward's outputs changed in the last place); and the mlp3 backward's tail.
#include "common.h"
#include "head_rows_body.h"
#include "mlp3_drop.h"
#include "../../include/tsgnn.h"

namespace {

// ================================================================================================ SAGPool: mlp3 + nll
constexpr int P3_WAVES = 8;                  // forward: 512 threads
constexpr int P3_BT = 256;                   // backward

struct P3Fwd {
  const float* r; int64_t ldr;
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  const int *ids, *labels;
  int n_labels, R, D0, D1, D2, C;
  float keep_scale;
  Mlp3Drop drop;
  float *a1, *a2, *logp, *loss;
};

struct P3Bwd {
  const float* r; int64_t ldr;
  const float *w1, *w2, *w3, *a1, *a2, *logp;
  const int *ids, *labels;
  const float* g;
  int n_labels, R, D0, D1, D2, C;
  float keep_scale;
  float* dr; int64_t lddr;
  float *dw1, *db1, *dw2, *db2, *dw3, *db3;
};

// vs[i][j] = act(W[j, :] . in_i + bias[j]) for i < RT, j < N   (W [N, K] row-major, K % 4 == 0; in_i = in + min(i, rows - 1) * ldin,
// 16-byte aligned rows in memory or LDS; vs [RT][N] in LDS)
template <int RT, bool RELU>
__device__ __forceinline__ void p3_dense(const float* in, int64_t ldin, int rows, int K, const float* __restrict__ w,
                                         const float* __restrict__ bias, int N, float* vs) {
  constexpr int EPW = RT <= 2 ? 8 : 4;       // weight rows a wave requests together
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int K4 = K >> 2;
  for (int j0 = wid; j0 < N; j0 += EPW * P3_WAVES) {
    float s[EPW][RT];
#pragma unroll
    for (int u = 0; u < EPW; ++u)
#pragma unroll
      for (int i = 0; i < RT; ++i) s[u][i] = 0.f;
    for (int k4 = lane; k4 < K4; k4 += 64) {
      float4 wv[EPW];
#pragma unroll
      for (int u = 0; u < EPW; ++u) {                                      // rows past N: a mapped row, result dropped
        const int j = j0 + P3_WAVES * u;
        wv[u] = ld4(w + (int64_t)(j < N ? j : 0) * K + 4 * k4);
      }
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float4 x = ld4(in + (int64_t)rows_row<RT>(min(i, rows - 1)) * ldin + 4 * k4);
#pragma unroll
        for (int u = 0; u < EPW; ++u) s[u][i] += (wv[u].x * x.x + wv[u].y * x.y) + (wv[u].z * x.z + wv[u].w * x.w);
      }
    }
#pragma unroll
    for (int u = 0; u < EPW; ++u) {
      const int j = j0 + P3_WAVES * u;
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float t = wave_sum(s[u][i]);
        if (lane == 0 && j < N) {
          const float v = t + (bias ? bias[j] : 0.f);
          vs[i * N + j] = RELU ? fmaxf(v, 0.f) : v;
        }
      }
    }
  }
}

template <int RT>
__global__ __launch_bounds__(64 * P3_WAVES) void posttrain_mlp3_nll_fwd_kernel(const P3Fwd a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float li[ROWS_MAXR];
  const int R = a.R, D0 = a.D0, D1 = a.D1, D2 = a.D2, C = a.C;
  float* v1 = smem;                      // [RT][D1]
  float* v2 = v1 + RT * D1;              // [RT][D2]
  float* lg = v2 + RT * D2;              // [RT][C]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  unsigned long long ctr = 0ull;
  if (a.drop.state) ctr = __hip_atomic_load(a.drop.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  p3_dense<RT, true>(a.r, a.ldr, R, D0, a.w1, a.b1, D1, v1);
  __syncthreads();
  const unsigned klo = a.drop.seed_lo + (unsigned)(ctr & 0xffffffffull), khi = a.drop.seed_hi + (unsigned)(ctr >> 32);
  for (int k = tid; k < RT * D1; k += 64 * P3_WAVES) {
    const int i = k / D1, j = k - i * D1;
    float m = 1.f;                                                          // dropout after the ReLU (network.py:48-49)
    if (a.drop.state) m = mlp3_keep(a.drop.thresh, klo, khi, (unsigned)i, (unsigned)j) * a.keep_scale;
    const float v = v1[k] * m;
    v1[k] = v;
    if (i < R) a.a1[k] = v;
  }
  __syncthreads();
  p3_dense<RT, true>(v1, D1, RT, D1, a.w2, a.b2, D2, v2);
  __syncthreads();
  for (int k = tid; k < R * D2; k += 64 * P3_WAVES) a.a2[k] = v2[k];
  p3_dense<RT, false>(v2, D2, RT, D2, a.w3, a.b3, C, lg);
  __syncthreads();
  if (wid < R) {                                                            // log_softmax and the row's loss: one wave per row
    const float* row = lg + wid * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(row[c] - m);
    s = wave_sum(s);
    const float lse = m + logf(s);
    for (int c = lane; c < C; c += 64) a.logp[wid * C + c] = row[c] - lse;
    if (lane == 0) li[wid] = lse - row[row_label(a.ids, a.labels, a.n_labels, C, wid)];
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < R; ++i) s += li[i];
    a.loss[0] = s / (float)R;
    if (a.drop.state) {                                                     // the only workgroup: the next launch's key, one writer
      a.drop.used[0] = ctr;
      __hip_atomic_store(a.drop.state, ctr + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int RT>
__global__ __launch_bounds__(P3_BT) void posttrain_mlp3_nll_bwd_kernel(const P3Bwd p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int ys[ROWS_MAXR];
  const int tid = threadIdx.x;
  const int R = p.R, D0 = p.D0, D1 = p.D1, D2 = p.D2, C = p.C;
  float* dlg = smem;                     // [RT][C]
  float* a2s = dlg + RT * C;             // [RT][D2]
  float* dz2 = a2s + RT * D2;            // [RT][D2]
  float* a1s = dz2 + RT * D2;            // [RT][D1]
  float* dz1 = a1s + RT * D1;            // [RT][D1]
  float* part = dz1 + RT * D1;           // [RT][4][64] (chain) / [RT][8][32] (dr)
  if (tid < RT) ys[tid] = tid < R ? row_label(p.ids, p.labels, p.n_labels, C, tid) : -1;
  __syncthreads();
  const float scale = (p.g ? p.g[0] : 1.f) / (float)R;
  for (int k = tid; k < RT * C; k += P3_BT) {                                // dlogits = g (softmax - onehot) / R
    const int i = k / C, c = k - i * C;
    dlg[k] = i < R ? scale * (expf(p.logp[k]) - (c == ys[i] ? 1.f : 0.f)) : 0.f;
  }
  for (int k = tid; k < RT * D2; k += P3_BT) a2s[k] = k < R * D2 ? p.a2[k] : 0.f;
  for (int k = tid; k < RT * D1; k += P3_BT) a1s[k] = k < R * D1 ? p.a1[k] : 0.f;
  __syncthreads();
  rows_chain<RT, P3_BT>(dlg, C, p.w3, D2, a2s, 1.f, dz2, part);               // dz2 = [a2 > 0] dlogits W3
  rows_chain<RT, P3_BT>(dz2, D2, p.w2, D1, a1s, p.keep_scale, dz1, part);     // dz1 = keep_scale [a1 > 0] dz2 W2
  rows_input_columns<RT, P3_BT>(p.r, p.ldr, R, D0, p.w1, D0, D1, dz1, p.dr, p.lddr, p.dw1, D0, part);
  // dW2 = dz2^T a1, dW3 = dlogits^T a2 and the bias gradients: outer products of LDS vectors, dealt out over the grid.  This is
  // rows_outer_tail's loop, kept here: as a call it costs the RT = 4 instantiation two vector registers (66) and with them the eighth
  // wave per SIMD (-Rpass-analysis=kernel-resource-usage)
  const int n2 = D2 * D1, n3 = C * D2;
  const int total = n2 + n3 + D1 + D2 + C;
  for (int idx = (int)blockIdx.x * P3_BT + tid; idx < total; idx += (int)gridDim.x * P3_BT) {
    float s = 0.f;
    if (idx < n2) {
      const int k = idx / D1, o = idx - k * D1;
#pragma unroll
      for (int i = 0; i < RT; ++i) s = fmaf(dz2[i * D2 + k], a1s[i * D1 + o], s);
      p.dw2[idx] = s;
    } else if (idx < n2 + n3) {
      const int t = idx - n2, c = t / D2, k = t - c * D2;
#pragma unroll
      for (int i = 0; i < RT; ++i) s = fmaf(dlg[i * C + c], a2s[i * D2 + k], s);
      p.dw3[t] = s;
    } else if (idx < n2 + n3 + D1) {
      const int o = idx - n2 - n3;
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dz1[i * D1 + o];
      if (p.db1) p.db1[o] = s;
    } else if (idx < n2 + n3 + D1 + D2) {
      const int k = idx - n2 - n3 - D1;
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dz2[i * D2 + k];
      if (p.db2) p.db2[k] = s;
    } else {
      const int c = idx - n2 - n3 - D1 - D2;
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dlg[i * C + c];
      if (p.db3) p.db3[c] = s;
    }
  }
}

// ================================================================================================ EigenGCN: mlp2 + cross-entropy
constexpr int P2_MAX = 512;                  // H, C
constexpr int P2_MAXD = 2048;

struct P2Fwd {
  const float* r; int64_t ldr;
  const float *w1, *b1, *w2, *b2;
  const int *ids, *labels;
  int n_labels, R, D, H, C;
  float *h, *z, *p, *loss;
};

struct P2Bwd {
  const float* r; int64_t ldr;
  const float *w1, *w2, *h, *p;
  const int *ids, *labels;
  const float* g;
  int n_labels, R, D, H, C;
  float* dr; int64_t lddr;
  float *dw1, *db1, *dw2, *db2;
};

template <int RT>
__global__ __launch_bounds__(1024) void posttrain_mlp2_ce_fwd_kernel(const P2Fwd a) {
  __shared__ float hs[RT][P2_MAX];
  __shared__ float zs[RT][P2_MAX];
  __shared__ float li[ROWS_MAXR];
  constexpr int RPW = RT <= 2 ? 8 : 4;                                      // weight rows per wave and pass
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int R = a.R, D = a.D, H = a.H, C = a.C;
  rows_dense16<RT, RPW, 16, true>(a.r, a.ldr, R, D, a.w1, D, a.b1, H, &hs[0][0], P2_MAX, a.h, R);
  __syncthreads();
  // W2's rows are H floats: scalar loads, lanes along the row
  rows_dense1<RT, RPW, 16>(&hs[0][0], P2_MAX, H, a.w2, a.b2, C, R, false, 0.f, a.z, &zs[0][0], P2_MAX);
  __syncthreads();
  if (wid < R) {                                                            // soft-max and the row's loss: one wave per row
    const float* row = zs[wid];
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(row[c] - m);
    s = wave_sum(s);
    const float inv = 1.f / s;
    for (int c = lane; c < C; c += 64) a.p[wid * C + c] = expf(row[c] - m) * inv;
    if (lane == 0) li[wid] = (m + logf(s)) - row[row_label(a.ids, a.labels, a.n_labels, C, wid)];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < R; ++i) s += li[i];
    a.loss[0] = s / (float)R;
  }
}

template <int RT>
__global__ __launch_bounds__(P3_BT) void posttrain_mlp2_ce_bwd_kernel(const P2Bwd a) {
  __shared__ float dz[RT * P2_MAX];          // [RT][C]
  __shared__ float dh[RT * P2_MAX];          // [RT][H]
  __shared__ float hs[RT * P2_MAX];          // [RT][H]
  __shared__ float part[RT * 256];
  __shared__ int ys[ROWS_MAXR];
  const int tid = threadIdx.x;
  const int R = a.R, D = a.D, H = a.H, C = a.C;
  if (tid < RT) ys[tid] = tid < R ? row_label(a.ids, a.labels, a.n_labels, C, tid) : -1;
  __syncthreads();
  const float scale = (a.g ? a.g[0] : 1.f) / (float)R;
  for (int k = tid; k < RT * C; k += P3_BT) {                                // dz = g (softmax - onehot) / R
    const int i = k / C, c = k - i * C;
    dz[k] = i < R ? scale * (a.p[k] - (c == ys[i] ? 1.f : 0.f)) : 0.f;
  }
  for (int k = tid; k < RT * H; k += P3_BT) hs[k] = k < R * H ? a.h[k] : 0.f;
  __syncthreads();
  rows_dh1<RT, P3_BT>(dz, C, a.w2, H, hs, dh);                                // dh = [h > 0] dz W2
  __syncthreads();
  rows_input_columns<RT, P3_BT>(a.r, a.ldr, R, D, a.w1, D, H, dh, a.dr, a.lddr, a.dw1, D, part);
  rows_outer_tail<RT, P3_BT>(dh, dz, nullptr, hs, nullptr, H, C, 0, a.dw2, nullptr, a.db1, a.db2, nullptr);   // dW2 = dz^T h | db1 | db2
}

}  // namespace

extern "C" {

int tsgnn_posttrain_mlp3_nll_supported(int D0, int D1, int D2, int C, int R) {
  return (tsgnn_mlp3_triplet_supported(D0, D1, D2, C) && C >= 2 && R >= 1 && R <= ROWS_MAXR) ? 1 : 0;
}

int tsgnn_posttrain_mlp3_nll_fwd_f32(const float* r, int64_t ldr, int R, const float* w1, const float* b1, float p, uint64_t seed,
                                     unsigned long long* state, unsigned long long* used, const float* w2, const float* b2,
                                     const float* w3, const float* b3, int D0, int D1, int D2, int C, const int32_t* ids,
                                     const int32_t* labels, int64_t n_labels, float* a1, float* a2, float* logp, float* loss,
                                     tsgnn_stream_t stream) {
  if (!r || !w1 || !w2 || !w3 || !ids || !labels || !a1 || !a2 || !logp || !loss || n_labels < 1 || n_labels > 0x7fffffff || R < 1 ||
      R > ROWS_MAXR || D0 < 1 || D1 < 1 || D2 < 1 || C < 2 || ldr < D0 || !(p >= 0.f) || !(p < 1.f) || (p > 0.f && (!state || !used)))
    return TSGNN_EINVAL;
  if (!tsgnn_posttrain_mlp3_nll_supported(D0, D1, D2, C, R) || (ldr % 4) ||
      ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(w2) | reinterpret_cast<uintptr_t>(w3)) & 15))
    return TSGNN_EUNSUPPORTED;
  const int rt = rt_of(R);
  P3Fwd a;
  a.r = r; a.ldr = ldr;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3;
  a.ids = ids; a.labels = labels; a.n_labels = (int)n_labels;
  a.R = R; a.D0 = D0; a.D1 = D1; a.D2 = D2; a.C = C;
  a.keep_scale = 1.0f / (1.0f - p);
  a.drop = Mlp3Drop{};
  if (p > 0.f) a.drop = Mlp3Drop{mlp3_thresh(p), (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), state, used};
  a.a1 = a1; a.a2 = a2; a.logp = logp; a.loss = loss;
  const size_t lds = sizeof(float) * rt * ((size_t)D1 + D2 + C);                 // <= 64 KB inside _supported
  TSGNN_ROWS_DISPATCH(posttrain_mlp3_nll_fwd_kernel, R, 1, 64 * P3_WAVES, lds);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_posttrain_mlp3_nll_bwd_f32(const float* r, int64_t ldr, int R, const float* w1, const float* w2, const float* w3, int D0, int D1,
                                     int D2, int C, float keep_scale, const int32_t* ids, const int32_t* labels, int64_t n_labels,
                                     const float* a1, const float* a2, const float* logp, const float* g_loss, float* dr, int64_t lddr,
                                     float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, tsgnn_stream_t stream) {
  if (!r || !w1 || !w2 || !w3 || !ids || !labels || !a1 || !a2 || !logp || !dw1 || !dw2 || !dw3 || n_labels < 1 || n_labels > 0x7fffffff ||
      R < 1 || R > ROWS_MAXR || D0 < 1 || D1 < 1 || D2 < 1 || C < 2 || ldr < D0 || (dr && lddr < D0))
    return TSGNN_EINVAL;
  if (!tsgnn_posttrain_mlp3_nll_supported(D0, D1, D2, C, R)) return TSGNN_EUNSUPPORTED;
  const int rt = rt_of(R);
  P3Bwd a;
  a.r = r; a.ldr = ldr;
  a.w1 = w1; a.w2 = w2; a.w3 = w3; a.a1 = a1; a.a2 = a2; a.logp = logp;
  a.ids = ids; a.labels = labels; a.g = g_loss; a.n_labels = (int)n_labels;
  a.R = R; a.D0 = D0; a.D1 = D1; a.D2 = D2; a.C = C;
  a.keep_scale = keep_scale;
  a.dr = dr; a.lddr = lddr;
  a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2; a.dw3 = dw3; a.db3 = db3;
  const size_t lds = sizeof(float) * rt * ((size_t)C + 2 * D2 + 2 * D1 + 256);   // <= 124 KB inside _supported
  TSGNN_ROWS_DISPATCH(posttrain_mlp3_nll_bwd_kernel, R, (unsigned)((D0 + 31) / 32), P3_BT, lds);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_posttrain_mlp2_ce_supported(int D, int H, int C, int R) {
  return (tsgnn_mlp2_triplet_supported(D, H, C) && C >= 2 && R >= 1 && R <= ROWS_MAXR) ? 1 : 0;
}

int tsgnn_posttrain_mlp2_ce_fwd_f32(const float* r, int64_t ldr, int R, const float* w1, const float* b1, const float* w2, const float* b2,
                                    int D, int H, int C, const int32_t* ids, const int32_t* labels, int64_t n_labels, float* h, float* z,
                                    float* p, float* loss, tsgnn_stream_t stream) {
  if (!r || !w1 || !w2 || !ids || !labels || !h || !z || !p || !loss || n_labels < 1 || n_labels > 0x7fffffff || R < 1 || R > ROWS_MAXR ||
      D < 1 || H < 1 || C < 2 || ldr < D)
    return TSGNN_EINVAL;
  if (!tsgnn_posttrain_mlp2_ce_supported(D, H, C, R) || (ldr % 4) ||
      ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(w1)) & 15))
    return TSGNN_EUNSUPPORTED;
  P2Fwd a;
  a.r = r; a.ldr = ldr;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.ids = ids; a.labels = labels; a.n_labels = (int)n_labels;
  a.R = R; a.D = D; a.H = H; a.C = C;
  a.h = h; a.z = z; a.p = p; a.loss = loss;
  TSGNN_ROWS_DISPATCH(posttrain_mlp2_ce_fwd_kernel, R, 1, 1024, 0);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_posttrain_mlp2_ce_bwd_f32(const float* r, int64_t ldr, int R, const float* w1, const float* w2, int D, int H, int C,
                                    const int32_t* ids, const int32_t* labels, int64_t n_labels, const float* h, const float* p,
                                    const float* g_loss, float* dr, int64_t lddr, float* dw1, float* db1, float* dw2, float* db2,
                                    tsgnn_stream_t stream) {
  if (!r || !w1 || !w2 || !ids || !labels || !h || !p || !dw1 || !dw2 || n_labels < 1 || n_labels > 0x7fffffff || R < 1 || R > ROWS_MAXR ||
      D < 1 || H < 1 || C < 2 || ldr < D || (dr && lddr < D))
    return TSGNN_EINVAL;
  if (!tsgnn_posttrain_mlp2_ce_supported(D, H, C, R)) return TSGNN_EUNSUPPORTED;
  P2Bwd a;
  a.r = r; a.ldr = ldr;
  a.w1 = w1; a.w2 = w2; a.h = h; a.p = p;
  a.ids = ids; a.labels = labels; a.g = g_loss; a.n_labels = (int)n_labels;
  a.R = R; a.D = D; a.H = H; a.C = C;
  a.dr = dr; a.lddr = lddr;
  a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2;
  TSGNN_ROWS_DISPATCH(posttrain_mlp2_ce_bwd_kernel, R, (unsigned)((D + 31) / 32), P3_BT, 0);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
